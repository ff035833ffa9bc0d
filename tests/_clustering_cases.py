"""Clustering (Davies-Bouldin) rewards at every cluster count and degeneracy (TEST INFRASTRUCTURE ONLY).

Two halves.  The first draws GEOMETRIES: sprite positions and cluster labels of one family each -- large clusters beside
singletons, k = n - 1, k = 2, a given k, collapsed clusters, shared centroids, near-coincident points, the label failures.
tests/test_davies_bouldin_cpu.py runs them through the oracle, the numpy model of tests/_davies_bouldin_model.py and
scikit-learn.  The second half puts one geometry into each environment of an engine and holds the engine to the oracle on all
four state paths (the tuned cover kernel, swb_ms_state_kernel, swb_rollout_kernel, swb_evaluate); it is written against an
engine factory, so that tests/test_emulated_clustering.py and tests/test_gpu_clustering.py run the same checks."""
import contextlib
import os

import numpy as np

LO, HI = 0.05, 0.9                 # sprites of scale 0.01 inside this square are not under a click at (0.99, 0.99)
LABEL_VALUES = 128                 # int8 cluster labels 0 .. 127 (task_scratch_t::pres[4]: four words of presence bits)

# Scenes whose Davies-Bouldin score is exactly 0.0 through scikit-learn's REGULAR path (float64 positions, found by the
# near-coincident sweep of tests/test_davies_bouldin_cpu.py): neither np.allclose early-out fires, every pair of clusters
# with a non-zero intra sum has centroid distance exactly 0 (-> inf), and the score is mean(max(0)) = 0.0.  The reference
# raises ZeroDivisionError at `1. / score` (tasks.py:215).  (x, y) as hex floats, one label per sprite.
ZERO_SCORE_FIXTURES = (
    ((('0x1.6e93297a482e5p-1', '0x1.92b9bfee22ddbp-2'), ('0x1.6e9329603cee3p-1', '0x1.92b9bfbf9c273p-2'),
      ('0x1.6e932973769d7p-1', '0x1.92b9bff8ddb79p-2'), ('0x1.6e93296789321p-1', '0x1.92b9bfce29defp-2'),
      ('0x1.6e93296dbf96bp-1', '0x1.92b9bfc695239p-2'), ('0x1.6e932963998f4p-1', '0x1.92b9bfd37935dp-2'),
      ('0x1.6e93296f84f79p-1', '0x1.92b9bfba07fdcp-2')), (44, 5, 44, 48, 58, 8, 92)),
    ((('0x1.53ba76a5289a5p-1', '0x1.7b9a43c626f72p-2'), ('0x1.53ba772f02abep-1', '0x1.7b9a4513e2c87p-2'),
      ('0x1.53ba77708d95dp-1', '0x1.7b9a456890905p-2'), ('0x1.53ba770082417p-1', '0x1.7b9a443ac09eep-2'),
      ('0x1.53ba76ca14e0ep-1', '0x1.7b9a43f2ffc26p-2')), (28, 111, 28, 99, 82)),
    ((('0x1.30076b730d91dp-1', '0x1.55878facfc909p-1'), ('0x1.30076b8e21d72p-1', '0x1.55878f9ae7d5bp-1'),
      ('0x1.30076b89aa54bp-1', '0x1.55878fa39c15ep-1'), ('0x1.30076b91e2b66p-1', '0x1.55878f8ebc9a0p-1'),
      ('0x1.30076b82101dap-1', '0x1.55878fa57827bp-1'), ('0x1.30076b70f71dcp-1', '0x1.55878fa4fe872p-1')),
     (127, 41, 127, 52, 41, 52)),
    ((('0x1.62e75cf7055cfp-1', '0x1.d7da5dbdd2b67p-2'), ('0x1.62e75dbcc32d1p-1', '0x1.d7da5d3798a77p-2'),
      ('0x1.62e75d754a173p-1', '0x1.d7da5cfde8e8ep-2'), ('0x1.62e75db235f33p-1', '0x1.d7da5d232280bp-2'),
      ('0x1.62e75d522e675p-1', '0x1.d7da5de788371p-2')), (66, 66, 43, 43, 34)),
)


def _cast(pos, f32):
  """Positions as the engine holds them: float64 arrays, of float32 values where the position dtype is float32."""
  return pos.astype(np.float32).astype(np.float64) if f32 else np.ascontiguousarray(pos, dtype=np.float64)


def _scene(rng, family, f32, sizes, unassigned=0, place=None, values=None):
  """One geometry: clusters of `sizes` members under distinct label values drawn from 0 .. 127, `unassigned` sprites of label
  -1, uniform positions that `place(pos, label)` may overwrite, the sprites in a random order."""
  sizes = [int(c) for c in sizes]
  values = rng.choice(LABEL_VALUES, len(sizes), replace=False) if values is None else values
  label = np.concatenate([np.full(c, v) for c, v in zip(sizes, values)] + [np.full(int(unassigned), -1)]).astype(np.int8)
  pos = rng.uniform(LO, HI, size=(len(label), 2))
  if place is not None:
    place(pos, label)
  order = rng.permutation(len(label))
  return dict(family=family, f32=bool(f32), pos=_cast(pos[order], f32), label=label[order])


def _split(rng, total, k):
  """k cluster sizes of at least one member that add up to `total`."""
  return 1 + rng.multinomial(total - k, np.full(k, 1.0 / k))


def fixture_geometry(i):
  xy, label = ZERO_SCORE_FIXTURES[i]
  pos = np.array([[float.fromhex(x), float.fromhex(y)] for x, y in xy])
  return dict(family='zero_score_fixture', f32=False, pos=pos, label=np.asarray(label, np.int8))


def geometry(rng, family, f32, n_max, k=None, e=None):
  """A geometry of `family` with at most `n_max` sprites (16: what the tuned state phase holds, 64: the ABI's limit).
  `k`: the cluster count of 'every_k'; `e`: the exponent of 'near_point' (all sprites within 10**e of one point)."""
  if family == 'random':            # n = 3 .. n_max, k = 2 .. n - 1, label values without replacement, some sprites unassigned
    n = int(rng.integers(3, n_max + 1))
    kk = int(rng.integers(2, n))
    u = int(rng.binomial(n - kk, 0.15))
    return _scene(rng, family, f32, _split(rng, n - u, kk), unassigned=u)
  if family == 'big_and_singletons':   # numpy's pairwise sum leaves its sequential branch at 8 members, and unrolls by 8
    big = int(rng.choice([8, 9, 16, 17, int(rng.integers(40, 57))] if n_max >= 64 else [8, 9, 12, 15]))
    singles = int(rng.integers(1, min(n_max - big, 7) + 1))
    sizes = [big] + [1] * singles
    if n_max - big - singles >= 8 and rng.random() < 0.5:
      sizes.append(8)
    return _scene(rng, family, f32, sizes)
  if family == 'k_n_minus_1':       # the most clusters check_number_of_labels lets through: one pair, the rest singletons
    n = int(rng.integers(3, n_max + 1))
    return _scene(rng, family, f32, [2] + [1] * (n - 2))
  if family == 'k2':
    n = int(rng.integers(3, n_max + 1))
    a = int(rng.integers(1, n))
    return _scene(rng, family, f32, [a, n - a])
  if family == 'every_k':
    n = int(rng.integers(k + 1, n_max + 1))
    return _scene(rng, family, f32, _split(rng, n, k))
  if family in ('all_collapsed', 'one_point', 'one_collapsed', 'near_point'):
    n = int(rng.integers(4, min(n_max, 24) + 1))
    kk = int(rng.integers(2, min(n - 1, 6) + 1))
    sizes = _split(rng, n, kk)
    if family == 'one_collapsed':   # cluster 0 on a point, cluster 1 spread out (both of two members or more)
      sizes = [2 + int(rng.integers(0, 3)), 2 + int(rng.integers(0, 3))] + [1 + int(c) for c in rng.integers(0, 3, size=kk - 2)]

    def place(pos, label):
      first = {}
      for i, v in enumerate(label):
        first.setdefault(int(v), i)
      if family == 'all_collapsed':
        for i, v in enumerate(label):
          pos[i] = pos[first[int(v)]]
      elif family == 'one_point':
        pos[:] = pos[0]
      elif family == 'one_collapsed':
        pos[label == label[0]] = pos[0]
      else:
        pos[:] = rng.uniform(0.2, 0.8, size=2) + rng.uniform(-1.0, 1.0, size=pos.shape) * 10.0 ** e
    return _scene(rng, family, f32, sizes, place=place)
  if family == 'quarter_grid':      # clusters 0 and 1 share the centroid (0.5, 0.5) exactly; the others stand on the grid too
    extra = int(rng.integers(0, 4))
    sizes = [2, 2] + list(1 + rng.integers(0, 3, size=extra))

    def place(pos, label):
      pos[:] = rng.integers(1, 4, size=pos.shape) * 0.25
      pos[0], pos[1], pos[2], pos[3] = (0.25, 0.5), (0.75, 0.5), (0.5, 0.25), (0.5, 0.75)
    return _scene(rng, family, f32, sizes, place=place)
  if family == 'k1':                # one cluster: ValueError
    return _scene(rng, family, f32, [int(rng.integers(1, n_max + 1))], unassigned=int(rng.integers(0, 2)))
  if family == 'k_equals_m':        # as many clusters as assigned sprites: ValueError
    kk = int(rng.integers(2, n_max))
    return _scene(rng, family, f32, [1] * kk, unassigned=int(rng.integers(0, n_max - kk + 1)))
  if family == 'none_assigned':
    return _scene(rng, family, f32, [], unassigned=int(rng.integers(1, n_max + 1)))
  if family == 'empty':             # an episode of no sprites
    return _scene(rng, family, f32, [])
  raise ValueError(family)


def oracle_score(g):
  """(error, score) of the oracle's davies_bouldin on a geometry."""
  from oracle import oracle
  return oracle.davies_bouldin(g['f32'], g['pos'][:, 0], g['pos'][:, 1], g['label'])


def facts(g):
  """What a geometry holds, for the floors every sweep asserts: assigned sprites m, clusters k, the largest cluster, the
  number of singletons, the largest label value."""
  lab = g['label'][g['label'] >= 0]
  values, counts = np.unique(lab, return_counts=True)
  return dict(n=len(g['label']), m=len(lab), k=len(values), largest=int(counts.max()) if len(counts) else 0,
              singletons=int((counts == 1).sum()), top_label=int(values.max()) if len(values) else -1)


# ---------------------------------------------------------------------------------------------------------------------
# Engines: one geometry per environment
# ---------------------------------------------------------------------------------------------------------------------
MISS = (0.99, 0.99)                # a click no sprite is under
PATHS = ('tuned', 'many_s64', 'many_s16_forced')      # the state kernels: the tuned step's, swb_ms_state_kernel at 64 / at 16 sprites


@contextlib.contextmanager
def _path_env(path):
  """SWB_MANY_SPRITES=1 (read when the handle is created) for the forced path, absent otherwise; restored on the way out."""
  old = os.environ.pop('SWB_MANY_SPRITES', None)
  if path == 'many_s16_forced':
    os.environ['SWB_MANY_SPRITES'] = '1'
  try:
    yield
  finally:
    os.environ.pop('SWB_MANY_SPRITES', None)
    if old is not None:
      os.environ['SWB_MANY_SPRITES'] = old


def sprites_of(path):
  return 64 if path == 'many_s64' else 16


def _classes(n_max):
  """(family, arguments) of one geometry of each class: large clusters beside singletons, the cluster counts at which the kernel
  takes another path (rows_per_pass = 64 / k: 3 at k = 21, 2 from 22, 1 from 33; the most a scene can hold), the degeneracies,
  the failures."""
  ks = (12, 21, 22, 32, 33, 47, 62, 63) if n_max >= 64 else (8, 9, 12, 15)
  spec = [('big_and_singletons', {})] * 4 + [('k_n_minus_1', {})] * 2 + [('k2', {})] * 2 + [('every_k', dict(k=k)) for k in ks]
  spec += [('random', {})] * 4 + [('all_collapsed', {}), ('one_point', {}), ('one_collapsed', {})] + [('quarter_grid', {})] * 2
  spec += [('near_point', dict(e=e)) for e in range(-12, -5)]
  return spec + [('k1', {}), ('k_equals_m', {}), ('none_assigned', {}), ('empty', {})]


def geometry_list(n_envs, n_max, f32, seed=0):
  """`n_envs` geometries: for float64 the recorded zero-score scenes, then one of each class, then the classes again with fresh
  draws."""
  rng = np.random.default_rng(1000 * seed + n_max + int(f32))
  spec = _classes(n_max)
  out = [] if f32 else [fixture_geometry(i) for i in range(len(ZERO_SCORE_FIXTURES))]
  assert n_envs >= len(out) + len(spec), 'n_envs = %d holds no geometry of each class (%d)' % (n_envs, len(out) + len(spec))
  for i in range(n_envs - len(out)):
    family, kw = spec[i % len(spec)]
    out.append(geometry(rng, family, f32, n_max, **kw))
  return out


def min_envs(path, f32):
  """The smallest batch that holds one geometry of each class."""
  return len(_classes(sprites_of(path))) + (0 if f32 else len(ZERO_SCORE_FIXTURES))


def scene(geoms, S, f32, sub_goals=0, aggregator='sum', seed=0, healthy_positions=False):
  """(cfg, pool) of len(geoms) environments, environment i replaying the one episode that holds geoms[i]: a pool of
  synthetic.make_pool with x, y, label and n_sprites overwritten.  SelectMove without motion cost on a small frame, sprites of
  scale 0.01; the Clustering's threshold (a metric of 0.6) lies amid the metrics of the geometries, so success flags and episode ends
  are mixed.  sub_goals > 0: a MetaAggregated of the Clustering and that many FindGoalPosition tasks whose filters match no
  sprite in every third environment (a NaN reward without an error).  healthy_positions: the sprites stand where make_pool put
  them (uniform over the frame) instead of on the geometry."""
  from spriteworld_amd import action_spaces, lowering, renderers, synthetic, tasks
  rng = np.random.default_rng(seed)
  n_envs, n_tasks = len(geoms), 1 + sub_goals
  clustering = tasks.Clustering([None, None], termination_threshold=0.6, terminate_bonus=1., reward_range=6.)
  if sub_goals:
    goals = [tasks.FindGoalPosition(filter_distrib=None, goal_position=(0.1 + 0.1 * j, 0.8 - 0.1 * j), terminate_distance=0.3,
                                    raw_reward_multiplier=20. + j) for j in range(sub_goals)]
    task = tasks.MetaAggregated([clustering] + goals, reward_aggregator=aggregator, termination_criterion='any', terminate_bonus=0.5)
  else:
    task = clustering
  rend = {'image': renderers.PILRenderer(image_size=(16, 16), anti_aliasing=2, bg_color=(7, 30, 110), color_to_rgb=renderers.hsv_to_rgb)}
  pool = synthetic.make_pool(rng, n_envs, S, [(0.0, 1.0)] * S, [[-1] * n_tasks] * S, n_tasks=n_tasks, scales=(0.01,), xy_range=(LO, HI))
  if not f32:
    pool.x[:] = rng.uniform(LO, HI, size=pool.x.shape)
    pool.y[:] = rng.uniform(LO, HI, size=pool.y.shape)
  pool.label[:] = 0
  for i, g in enumerate(geoms):
    n = len(g['label'])
    assert n <= S and g['f32'] == f32
    pool.n_sprites[i] = n
    pool.label[i, 0, :n] = g['label']
    if not healthy_positions:
      pool.x[i, :n], pool.y[i, :n] = g['pos'][:, 0], g['pos'][:, 1]
    for j in range(1, n_tasks):
      pool.label[i, j, :n] = 0 if i % 3 == 0 else (rng.random(n) < 0.4)
  cfg = lowering.lower_config(task, action_spaces.SelectMove(scale=0.3, motion_cost=0.), rend, True, 10, n_envs, S, f32)
  pool.assign_round_robin(n_envs, 1)
  return cfg, pool


def expected_errors(geoms):
  return np.array([oracle_score(g)[0] for g in geoms], np.uint8)


def assert_coverage(geoms, errors, n_sprites, n_max, what):
  """What a case claims to hold, from the oracle's flags and state: flagged and unflagged environments, both error codes, a
  cluster of 8 members or more, an empty episode and -- where 64 sprites fit -- 33 clusters or more and a label value of 96 or
  more in an environment that is not flagged."""
  from spriteworld_amd import _abi
  f = [facts(g) for g in geoms]
  ok = errors == 0
  assert ok.any() and (errors == _abi.ENV_ERR_DB_ZERO).any() and (errors == _abi.ENV_ERR_DB_LABELS).any(), (what, errors)
  assert (n_sprites == 0).any(), what
  assert any(o and v['largest'] >= 8 and v['singletons'] > 0 for o, v in zip(ok, f)), what
  assert any(o and v['top_label'] >= 32 for o, v in zip(ok, f)), what
  if n_max >= 64:
    assert any(o and v['k'] >= 33 for o, v in zip(ok, f)) and any(o and v['k'] == 63 for o, v in zip(ok, f)), what
    assert any(o and v['top_label'] >= 96 for o, v in zip(ok, f)), what


def _engines(make_engine, path, cfg, pool):
  from oracle import oracle
  with _path_env(path):
    eng = make_engine(cfg, pool)
  assert eng.variant()['many_sprites'] == int(path != 'tuned'), (path, eng.variant())
  return oracle.Engine(cfg, pool), eng


def _actions(n_envs, rng, st=None):
  """Clicks at MISS with a random motion; given a state, every second environment's click lands on its sprite 0."""
  a = np.empty((n_envs, 4))
  a[:, 0], a[:, 1] = MISS
  a[:, 2:] = rng.uniform(0.0, 1.0, size=(n_envs, 2))
  if st is not None:
    for i in range(0, n_envs, 2):
      if st['n_sprites'][i]:
        a[i, 0], a[i, 1] = st['x'][i, 0], st['y'][i, 0]
  return a


def step_case(make_engine, path, f32, n_envs):
  """FIRST; a click that misses (the reward is the crafted geometry's: the oracle's positions are the pool's, its flags the
  geometry's own); a click on sprite 0 of every second environment (moved geometries).  Every step to the bar of
  _parity.compare with the sticky OR of the oracle's flags as the expected error buffer; the second step rendered, +-0."""
  from tests import _parity
  S = sprites_of(path)
  geoms = geometry_list(n_envs, S, f32)
  cfg, pool = scene(geoms, S, f32)
  ora, eng = _engines(make_engine, path, cfg, pool)
  rng = np.random.default_rng(5)
  sticky = np.zeros(n_envs, np.uint8)
  what = '%s, %s' % (path, 'float32' if f32 else 'float64')
  st, moved = None, 0
  for t in range(3):
    a = _actions(n_envs, rng, st if t == 2 else None)
    want = ora.step(a, render=(t == 1))
    eng.step(a, render=(t == 1))
    sticky |= want['error']
    new = _parity.compare(t, ora, eng, want, eng.outputs_host(), frames=(t == 1), errors=sticky, what=what)
    if t == 1:
      so = ora.state()
      for i, g in enumerate(geoms):               # nothing moved: the rewards of this step are the crafted geometries'
        n = len(g['label'])
        assert so['n_sprites'][i] == n and np.array_equal(so['x'][i, :n], g['pos'][:, 0]) and np.array_equal(so['y'][i, :n], g['pos'][:, 1])
      np.testing.assert_array_equal(want['error'], expected_errors(geoms), err_msg=what)
      assert (want['step_type'] != 0).all() and np.array_equal(np.isnan(want['reward']), want['error'] != 0)
      assert want['success'][want['error'] != 0].max() == 0 and np.isfinite(want['reward'][want['error'] == 0]).all()
      assert_coverage(geoms, want['error'], so['n_sprites'], S, what)
    if t == 2:
      mid = want['step_type'] != 0
      moved = int(((new['x'][mid] != st['x'][mid]) | (new['y'][mid] != st['y'][mid])).any(axis=1).sum())
    st = new
  eng.close()
  assert moved > 0, 'no sprite was moved: the third step covers no moved geometry'


def rollout_case(make_engine, path, f32, n_envs):
  """swb_rollout_kernel on the same pools: M = 2 candidates of K = 2 steps from the state after FIRST, candidate 0 missing,
  candidate 1 clicking sprite 0; rewards, flags (error [N, M] included) and end positions against the oracle."""
  from tests import _rollout_cases
  S = sprites_of(path)
  geoms = geometry_list(n_envs, S, f32)
  cfg, pool = scene(geoms, S, f32)
  ora, eng = _engines(make_engine, path, cfg, pool)
  rng = np.random.default_rng(6)
  live = [_actions(n_envs, rng)]
  eng.step(live[0], render=False)
  st = eng.state()
  acts = np.stack([np.stack([_actions(n_envs, rng), _actions(n_envs, rng)], axis=1) for _ in range(2)], axis=0)      # [K, N, M, 4]
  has = st['n_sprites'] > 0
  acts[0, has, 1, 0], acts[0, has, 1, 1] = st['x'][has, 0], st['y'][has, 0]
  want = _rollout_cases.reference(cfg, pool, live, acts)
  what = 'rollout, %s, %s' % (path, 'float32' if f32 else 'float64')
  np.testing.assert_array_equal(want['error'][:, 0], expected_errors(geoms), err_msg=what)      # (candidate 0 never moves a sprite)
  assert_coverage(geoms, want['error'][:, 0], want['n_sprites'][:, 0], S, what)
  assert (_rollout_cases._bits(want['x'][:, 0]) != _rollout_cases._bits(want['x'][:, 1])).any(), what
  _rollout_cases.assert_equal(_rollout_cases.rollout(eng, acts), want, what)
  eng.close()


def evaluate_case(make_engine, path, f32, n_envs):
  """swb_evaluate: a healthy scene (the geometries' labels on sprites spread over the frame), then set_positions moves every
  environment onto its geometry; evaluate() equals the oracle's both times, and is 0 where the reward would be NaN."""
  S = sprites_of(path)
  geoms = geometry_list(n_envs, S, f32)
  cfg, pool = scene(geoms, S, f32, healthy_positions=True)
  ora, eng = _engines(make_engine, path, cfg, pool)
  a = _actions(n_envs, np.random.default_rng(7))
  ora.step(a, render=False)
  eng.step(a, render=False)
  as_numpy = lambda t: t.cpu().numpy() if hasattr(t, 'cpu') else np.asarray(t)
  before = ora.evaluate()
  np.testing.assert_array_equal(as_numpy(eng.evaluate()), before)
  st = ora.state()
  x, y = st['x'].copy(), st['y'].copy()
  for i, g in enumerate(geoms):
    n = len(g['label'])
    x[i, :n], y[i, :n] = g['pos'][:, 0], g['pos'][:, 1]
  ora.set_positions(x, y)
  eng.set_positions(x, y)
  after = ora.evaluate()
  np.testing.assert_array_equal(as_numpy(eng.evaluate()), after)
  errors = expected_errors(geoms)
  assert (after[errors != 0] == 0).all() and after.any() and (after[errors == 0] == 0).any() and (after != before).any()
  assert_coverage(geoms, errors, st['n_sprites'], S, 'evaluate, ' + path)
  eng.close()


META = [(n_sub, agg) for n_sub in (2, 7, 8) for agg in ('sum', 'mean', 'max', 'min')]


def meta_case(make_engine, path, f32, n_envs, n_sub, aggregator):
  """MetaAggregated of `n_sub` sub-tasks (the kernel sums eight in another order than fewer): a Clustering that errors in
  some environments, FindGoalPosition tasks whose filter matches no sprite in every third one (NaN without an error), an
  environment where every sub-reward is NaN."""
  from tests import _parity
  S = sprites_of(path)
  geoms = geometry_list(n_envs, S, f32)
  cfg, pool = scene(geoms, S, f32, sub_goals=n_sub - 1, aggregator=aggregator)
  assert cfg.n_tasks == n_sub and cfg.is_meta
  errors = expected_errors(geoms)
  no_match = ~pool.label[:, 1:, :].any(axis=(1, 2))
  assert (no_match & (errors != 0)).any() and (no_match & (errors == 0)).any() and (~no_match & (errors != 0)).any()
  ora, eng = _engines(make_engine, path, cfg, pool)
  rng = np.random.default_rng(8)
  sticky = np.zeros(n_envs, np.uint8)
  what = 'meta %d %s, %s, %s' % (n_sub, aggregator, path, 'float32' if f32 else 'float64')
  st = None
  for t in range(3):
    a = _actions(n_envs, rng, st if t == 2 else None)
    want = ora.step(a, render=False)
    eng.step(a, render=False)
    sticky |= want['error']
    st = _parity.compare(t, ora, eng, want, eng.outputs_host(), frames=False, errors=sticky, what=what)
    if t == 1:
      np.testing.assert_array_equal(want['error'], errors, err_msg=what)
      assert np.isfinite(want['reward'][~no_match]).all()
  eng.close()
