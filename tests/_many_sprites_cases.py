"""Scenarios of the many-sprite path (handles of more than 16 sprites, up to 64), written against an engine factory so that
the emulated suite (tests/test_emulated_many_sprites.py) and the GPU suite (tests/test_gpu_many_sprites.py) run the same
checks against the oracle: state, rewards, step types and discounts bit-exact, frames +-0."""
import numpy as np

from spriteworld_amd import _abi
from spriteworld_amd import workloads
from tests import _parity


def _np(a):
  return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def run_parity(make_engine, name, n_envs, steps, aa, seed=0, episodes_per_env=2, frame_every=1):
  """Steps `name` on the engine and the oracle; returns (FIRST steps seen, the most sprites an episode had)."""
  return _parity.run(make_engine, name, n_envs, steps, aa, seed=seed, episodes_per_env=episodes_per_env, frame_every=frame_every,
                     expect={'many_sprites': 1, 'large_frames': 1})


def setters_case(make_engine, name='ragged_s64', n_envs=4, steps=5, aa=3, seed=1, built=None):
  """sprite.py:152-175 setters on sprites 16 .. 63 of live episodes against swo_set_sprite_attr, then steps and
  observation() of the modified scenes.  `built`: a (cfg, pool, sample) triple (e.g. of scene()) instead of workload `name`."""
  from oracle import oracle
  from spriteworld_amd import shapes
  cfg, pool, sample = built or workloads.build(name, n_envs, episodes_per_env=3, seed=seed, anti_aliasing=aa)
  pool.n_sprites[:] = np.maximum(pool.n_sprites, 20)       # every episode has sprites beyond index 16
  ora, eng = oracle.Engine(cfg, pool), make_engine(cfg, pool)
  rng = np.random.default_rng(seed + 100)
  srng = np.random.RandomState(seed + 5)
  applied = 0
  for t in range(steps):
    a = sample(rng)
    want = ora.step(a)
    eng.step(a)
    st = _parity.compare(t, ora, eng, want, eng.outputs_host())
    live = np.flatnonzero(st['reset_next'] == 0)
    for env in live[:3]:
      k = int(srng.randint(16, st['n_sprites'][env]))
      attr = int(srng.randint(0, 3))
      value = (float(srng.randint(0, len(shapes.SHAPES))) if attr == _abi.ATTR_SHAPE else
               float(srng.choice([17., 45., 133.5, 270.])) if attr == _abi.ATTR_ANGLE else float(srng.choice([0.05, 0.12, 0.2])))
      ora.set_sprite_attr(int(env), k, attr, value)
      eng.set_sprite_attr(int(env), k, attr, value)
      applied += 1
      so, sg = ora.get_sprite(int(env), k), eng.get_sprite(int(env), k)
      assert (so['shape'], so['angle'], so['scale']) == (sg['shape'], sg['angle'], sg['scale'])
      assert np.array_equal(_parity.bits(so['path']), _parity.bits(sg['path'])), (t, env, k, attr, value)
    np.testing.assert_array_equal(_np(eng.render()), ora.render(), err_msg='render t=%d' % t)
  assert applied > 0
  eng.close()


def render_and_evaluate_case(make_engine, name='cluster_s40', n_envs=3, aa=5, seed=2, built=None):
  """observation() (swb_render: the render kernels alone) equals the step's frame and the oracle's; success() of the
  sprites after swb_set_positions (swb_evaluate) equals the oracle's; neither advances the state.  `built`: a
  (cfg, pool, sample) triple (e.g. of scene()) instead of workload `name`."""
  from oracle import oracle
  cfg, pool, sample = built or workloads.build(name, n_envs, episodes_per_env=2, seed=seed, anti_aliasing=aa)
  ora, eng = oracle.Engine(cfg, pool), make_engine(cfg, pool)
  rng = np.random.default_rng(seed + 100)
  for t in range(2):
    a = sample(rng)
    want = ora.step(a)
    eng.step(a)
    _parity.compare(t, ora, eng, want, eng.outputs_host())
  frame = eng.outputs_host()['obs'].copy()
  before = eng.state()
  np.testing.assert_array_equal(_np(eng.render()), frame)
  np.testing.assert_array_equal(ora.render(), frame)
  # move every sprite: success() follows the sprites as they are now
  st = ora.state()
  x, y = st['x'].copy(), st['y'].copy()
  x[:, ::2] = np.float32(0.5)
  ora.set_positions(x, y)
  eng.set_positions(x, y)
  np.testing.assert_array_equal(_np(eng.evaluate()), ora.evaluate())
  after = eng.state()
  for k in ('step_count', 'reset_next', 'episode', 'pool_entry', 'n_sprites'):
    np.testing.assert_array_equal(after[k], before[k])
  np.testing.assert_array_equal(_np(eng.render()), ora.render())
  eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# Scenes of 17 to 64 sprites on frames of any geometry (the many-sprite state kernel x the large-frame render kernels)
# ---------------------------------------------------------------------------------------------------------------------
BG = (7, 30, 110)


def default_scales(image_size, aa):
  """Three scales for a canvas: a sprite of a few pixels, a small one, and one that crosses several blocks of canvas rows and
  hangs over the edge when it stands near one."""
  return (1.5 / (aa * max(image_size)), 0.04, 0.3)


def aimed(cfg, n_envs):
  """sample(rng, st=None): uniform actions; given the state before the step, every second environment's click (SelectMove /
  DragAndDrop) lands on the centre of one of its sprites, so that hit tests hit."""
  if cfg.action_space == _abi.ACTION_EMBODIED:
    def sample(r, st=None):
      return np.stack([r.integers(0, 2, n_envs), r.integers(0, 4, n_envs)], 1).astype(np.int32)
    return sample

  def sample(r, st=None):
    a = r.uniform(0.0, 1.0, size=(n_envs, 4))
    if st is not None:
      for env in range(0, n_envs, 2):
        n = int(st['n_sprites'][env])
        if n:
          k = int(r.integers(0, n))
          a[env, 0], a[env, 1] = st['x'][env, k], st['y'][env, k]
    return a.astype(np.float32) if cfg.action_is_f32 else a
  return sample


def scene(S, image_size, aa, n_envs, task='goal', space='select', f32=True, seed=0, episodes_per_env=2, scales=None,
          shape_names=('square', 'triangle', 'circle', 'star_5', 'spoke_4'), max_len=3, ragged=True, bg=BG, pool_entries=None):
  """(cfg, pool, sample) like workloads.build, for `S` sprites on a PILRenderer(image_size=(w, h), anti_aliasing=aa) with a
  non-black background.  task: 'goal' (FindGoalPosition), 'cluster' (Clustering of S // 3 clusters of three; every episode has
  S sprites: Davies-Bouldin wants 1 < k < m), 'meta' (MetaAggregated of four FindGoalPosition).  space: 'select', 'drag',
  'embodied'.  f32=False: float64 positions with full mantissas, and velocities.  Positions cover the whole frame, so sprites
  of the largest scale hang over every edge; `ragged`: episodes of 0 .. S sprites, the first four of S, 0, 17 and 1.  `pool_entries`: a pool of that many episodes, environment i replaying
  episode i modulo that (a large batch need not draw an episode per environment)."""
  from spriteworld_amd import action_spaces, lowering, renderers, synthetic, tasks
  rng = np.random.default_rng(seed)
  P = pool_entries or n_envs * episodes_per_env
  n_tasks = 1
  if task == 'goal':
    tk = tasks.FindGoalPosition(filter_distrib=None, terminate_distance=0.05)
    labels = [[int(i % 3 == 0)] for i in range(S)]
  elif task == 'cluster':
    k = S // 3
    tk = tasks.Clustering([None] * k, termination_threshold=1.5, terminate_bonus=1., reward_range=6.)
    labels = [[i] for i in range(k) for _ in range(3)] + [[-1]] * (S - 3 * k)
    ragged = False
  elif task == 'meta':
    goals = [(0.75, 0.75), (0.75, 0.25), (0.25, 0.75), (0.25, 0.25)]
    subs = [tasks.FindGoalPosition(filter_distrib=None, goal_position=g, terminate_distance=0.05, raw_reward_multiplier=20.)
            for g in goals]
    tk = tasks.MetaAggregated(subs, reward_aggregator='mean', termination_criterion='any', terminate_bonus=1.)
    labels = [[int(i % 4 == j) for j in range(4)] for i in range(S)]
    n_tasks = 4
  else:
    raise ValueError(task)
  aspace = {'select': lambda: action_spaces.SelectMove(scale=0.3, motion_cost=0.5),
            'drag': lambda: action_spaces.DragAndDrop(scale=0.3),
            'embodied': lambda: action_spaces.Embodied(step_size=0.1)}[space]()
  rend = {'image': renderers.PILRenderer(image_size=tuple(image_size), anti_aliasing=aa, bg_color=bg,
                                         color_to_rgb=renderers.hsv_to_rgb)}
  pool = synthetic.make_pool(rng, P, S, [(0.0, 1.0)] * S, labels, n_tasks=n_tasks, shape_names=shape_names,
                             scales=scales or default_scales(image_size, aa), angles=tuple(range(0, 360, 23)), xy_range=(0.0, 1.0))
  if not f32:
    pool.x[:] = rng.uniform(0.0, 1.0, size=pool.x.shape)
    pool.y[:] = rng.uniform(0.0, 1.0, size=pool.y.shape)
    pool.x_vel[:] = rng.uniform(-0.01, 0.01, size=pool.x.shape)
    pool.y_vel[:] = rng.uniform(-0.01, 0.01, size=pool.x.shape)
  if ragged:
    pool.n_sprites[:] = rng.integers(0, S + 1, size=P)
    pool.n_sprites[:min(P, 4)] = (S, 0, 17, 1)[:min(P, 4)]
    if space == 'embodied':                       # (Embodied moves sprites[-1]: an episode has a body)
      pool.n_sprites[:] = np.maximum(pool.n_sprites, 1)
  # what every case claims (run_scene asserts it) does not hang on the draw: in episodes of six sprites or more, four sprites of
  # the largest scale stand at the four edges, and sprite 4 / 5 have the smallest / the largest scale
  sc = sorted(scales or default_scales(image_size, aa))
  num = np.float32 if f32 else np.float64
  for e in np.flatnonzero(pool.n_sprites >= 6):
    for s, (x, y) in enumerate(((0.02, 0.4), (0.97, 0.6), (0.45, 0.03), (0.55, 0.98))):
      pool.x[e, s], pool.y[e, s] = float(num(x + rng.uniform(-0.02, 0.02))), float(num(y + rng.uniform(-0.02, 0.02)))
    pool.scale[e, :4] = sc[-1]
    pool.scale[e, 4], pool.scale[e, 5] = sc[0], sc[-1]
  cfg = lowering.lower_config(tk, aspace, rend, True, max_len, n_envs, S, f32)
  pool.assign_round_robin(n_envs, None if pool_entries else episodes_per_env)
  return cfg, pool, aimed(cfg, n_envs)


def scene_claims(cfg, pool):
  """What the sprites of `pool`, where its episodes start, do on the canvas: how many cross a boundary between blocks of 64 /
  of 16 canvas rows (swb_lf_args::rows_per_block), how many are at most 4 x 4 pixels, how many hang over each edge."""
  from oracle import oracle
  Wc, Hc = cfg.anti_aliasing * cfg.image_h, cfg.anti_aliasing * cfg.image_w
  c = dict(blocks64=0, blocks16=0, few_pixels=0, left=0, right=0, bottom=0, top=0)
  for e in range(pool.n_entries):
    for s in range(int(pool.n_sprites[e])):
      v = oracle.vertices(int(pool.shape[e, s]), pool.scale[e, s], pool.angle[e, s], pool.x[e, s], pool.y[e, s])
      px, py = np.trunc(Wc * v[:, 0]).astype(np.int64), np.trunc(Hc * v[:, 1]).astype(np.int64)
      lo, hi = max(int(py.min()), 0), min(int(py.max()), Hc - 1)
      if lo <= hi:
        c['blocks64'] += int(hi // 64 > lo // 64)
        c['blocks16'] += int(hi // 16 > lo // 16)
      c['few_pixels'] += int(px.max() - px.min() < 4 and py.max() - py.min() < 4)
      c['left'] += int(px.min() < 0)
      c['right'] += int(px.max() >= Wc)
      c['bottom'] += int(py.min() < 0)
      c['top'] += int(py.max() >= Hc)
  return c


def run_scene(make_engine, built, steps, many=True, check_claims=True, want_most=17, want_reset=True):
  """Steps a (cfg, pool, sample) triple on the engine and the oracle, every step to the bar of _parity.compare(); asserts what the
  case claims to exercise: the kernel path, more than 16 sprites seen, a reset seen, sprites moved by a hit (SelectMove /
  DragAndDrop), sprites across row blocks, of a few pixels and over each canvas edge."""
  from oracle import oracle
  cfg, pool, sample = built
  n_envs = cfg.n_envs
  if check_claims:
    c = scene_claims(cfg, pool)
    rows = 64 if n_envs >= 64 else 16                # (lf_render: rows_per_block)
    assert c['few_pixels'] > 0 and (c['blocks%d' % rows] > 0 or cfg.anti_aliasing * cfg.image_w <= rows), c
    assert min(c['left'], c['right'], c['bottom'], c['top']) > 0, c
  ora, eng = oracle.Engine(cfg, pool), make_engine(cfg, pool)
  v = eng.variant()
  assert v['large_frames'] == 1 and v['many_sprites'] == int(many), v
  rng = np.random.default_rng(1234)
  firsts, most, moved = 0, 0, 0
  st = None
  for t in range(steps):
    a = sample(rng, st)
    want = ora.step(a)
    eng.step(a)
    new = _parity.compare(t, ora, eng, want, eng.outputs_host())
    if st is not None:
      mid = want['step_type'] != 0                  # (a FIRST step installs a new episode: not a move)
      moved += int(((new['x'][mid] != st['x'][mid]) | (new['y'][mid] != st['y'][mid])).any(axis=1).sum())
    st = new
    firsts += int((want['step_type'] == 0).sum())
    most = max(most, int(st['n_sprites'].max()))
  eng.close()
  assert most >= want_most, most
  assert firsts > n_envs or not want_reset, 'no reset seen'
  if cfg.action_space != _abi.ACTION_EMBODIED:
    assert moved > 0, 'no sprite was moved: the hit test never hit'
  return dict(firsts=firsts, most=most, moved=moved)


def refusals_case(make_engine, error):
  """One step past each limit of the large-frame path: refused where the handle is created, the message naming the limit.
  (The height-only case has 20 sprites: with up to 16 sprites a 256 px wide canvas of 4100 rows is no large frame -- the tuned
  kernels take it, whose limit is 65535 rows.)"""
  import pytest
  for S, size, aa, what in ((4, (516, 16), 8, 'canvas 4128x128 too large: at most 4096 px'),      # the width alone
                            (20, (64, 1025), 4, 'canvas 256x4100 too large: at most 4096 px'),     # the height alone
                            (4, (1028, 16), 1, 'image width 1028 too large: at most 1024 columns'),
                            (20, (260, 260), 16, 'canvas 4160x4160 too large: at most 4096 px')):
    cfg, pool, _ = scene(S, size, aa, 1, episodes_per_env=1, ragged=False)
    with pytest.raises(error, match=what):
      make_engine(cfg, pool)
  cfg, pool, _ = scene(64, (64, 64), 2, 1, episodes_per_env=1)
  for s in (65, 99):
    cfg.max_sprites = s
    with pytest.raises(error, match='at most 64 sprites per environment'):
      make_engine(cfg, None)


def _shapes_of(total, most=_abi.SWB_MAX_SPRITES):
  """Shape indices (at most `most` sprites) whose vertex counts add up to `total`, with 'circle' holding a 64-gon: as many
  64-gons as leave a remainder of at least 3, the remainder from the built-in shapes of 3 .. 18 vertices (fewest sprites)."""
  from spriteworld_amd import shapes
  small = {}
  for name in shapes.SHAPE_NAMES:
    if name != 'circle':
      small.setdefault(len(shapes.SHAPES[name]), shapes.shape_index(name))
  k = min((total - 3) // 64, most - 2)
  r = total - 64 * k
  best = {0: []}
  for v in range(1, r + 1):
    c = [best[v - n] + [n] for n in small if v - n in best]
    if c:
      best[v] = min(c, key=len)
  assert r in best and k + len(best[r]) <= most, (total, k, r)
  return [small[n] for n in best[r]] + [shapes.shape_index('circle')] * k      # (small shapes first: sprite 0 can grow)


def vertex_budget_case(make_engine, error, image_size, aa, n_envs=2):
  """The vertex budget of the raster kernel's LDS as a boundary: the budget B is read from the refusal of an oversized pool; a
  scene of exactly B vertices is accepted and renders +-0; B + 1 vertices are refused by swb_set_pool; a setter that would take
  the live scene of B vertices above B is refused by swb_set_sprite_attr and changes nothing.  Returns B."""
  import re
  import pytest
  from oracle import oracle
  from spriteworld_amd import shapes
  from tests import _util
  with _util.swapped_shape('circle', shapes.polygon(64)):
    circle = shapes.shape_index('circle')
    cfg, pool, sample = scene(64, image_size, aa, n_envs, episodes_per_env=1, ragged=False, max_len=2, scales=(0.03, 0.08))
    pool.shape[:] = circle
    with pytest.raises(error, match='swb_set_pool: a scene of 4096 polygon vertices exceeds the vertex budget') as info:
      make_engine(cfg, pool)
    m = re.search(r'raster kernel, ([0-9]+) vertices per scene at a ([0-9]+) px canvas', str(info.value))
    B = int(m.group(1))
    assert int(m.group(2)) == aa * image_size[0] and 64 * 3 < B < 4096, str(info.value)

    def install(total):
      idx = _shapes_of(total)
      pool.n_sprites[:] = 6                       # every other episode: a light one
      pool.shape[:] = shapes.shape_index('square')
      pool.n_sprites[0] = len(idx)
      pool.shape[0, :len(idx)] = idx
      assert sum(len(shapes.SHAPES[shapes.SHAPE_NAMES[i]]) for i in pool.shape[0, :len(idx)]) == total
      return idx

    install(B + 1)
    with pytest.raises(error, match='swb_set_pool: a scene of [0-9]+ polygon vertices exceeds the vertex budget'):
      make_engine(cfg, pool)
    idx = install(B)
    ora, eng = oracle.Engine(cfg, pool), make_engine(cfg, pool)
    assert eng.variant()['many_sprites'] == 1 and eng.variant()['large_frames'] == 1
    rng = np.random.default_rng(3)
    a = sample(rng)
    _parity.compare(0, ora, eng, ora.step(a), (eng.step(a), eng.outputs_host())[1])
    # sprite 0 of environment 0 (an episode of B vertices) has one of the small shapes: as a 64-gon the scene exceeds B
    assert idx[0] != circle and eng.state()['n_sprites'][0] == len(idx)
    before = eng.get_sprite(0, 0)
    with pytest.raises(error, match='swb_set_sprite_attr: a scene of [0-9]+ polygon vertices exceeds the vertex budget'):
      eng.set_sprite_attr(0, 0, _abi.ATTR_SHAPE, float(circle))
    after = eng.get_sprite(0, 0)
    assert after['shape'] == before['shape'] and np.array_equal(_parity.bits(after['path']), _parity.bits(before['path']))
    np.testing.assert_array_equal(_np(eng.render()), ora.render())
    # ... and one that keeps the scene at B vertices (an angle) is accepted: the scene renders at its budget through the setters' tables
    ora.set_sprite_attr(0, 0, _abi.ATTR_ANGLE, 33.0)
    eng.set_sprite_attr(0, 0, _abi.ATTR_ANGLE, 33.0)
    np.testing.assert_array_equal(_np(eng.render()), ora.render())
    a = sample(rng)
    _parity.compare(1, ora, eng, ora.step(a), (eng.step(a), eng.outputs_host())[1])
    eng.close()
  return B


FACTOR_COLUMNS = ('x', 'y', 'shape', 'angle', 'scale', 'c0', 'c1', 'c2', 'x_vel', 'y_vel')


def _want_factors(st, pool, shape, angle, scale):
  e = st['pool_entry']
  want = np.stack([st['x'], st['y'], shape + 1.0, angle, scale, pool.color[e][:, :, 0], pool.color[e][:, :, 1],
                   pool.color[e][:, :, 2], pool.x_vel[e], pool.y_vel[e]], axis=2)
  want[np.arange(want.shape[1])[None, :] >= st['n_sprites'][:, None]] = 0.0
  return want


def factors_case(make_engine, n_envs=3):
  """factors() -- all ten columns -- and sprite_types() of sprites beyond index 16, from the pool and, after a setter on such
  a sprite, from the setters' tables (the `ov` branch of swb_factors_kernel)."""
  from spriteworld_amd import shapes
  cfg, pool, sample = scene(40, (64, 64), 2, n_envs, f32=False, max_len=30, ragged=False, seed=3)
  pool.attr_f32[:] = np.random.default_rng(5).integers(0, 4, size=pool.attr_f32.shape)
  eng = make_engine(cfg, pool)
  eng.step(sample(np.random.default_rng(0)))
  st = eng.state()
  e = st['pool_entry']
  shape, angle, scale = pool.shape[e].astype(np.float64), pool.angle[e].copy(), pool.scale[e].copy()
  assert (pool.x_vel[e] != 0).all() and (angle[:, 16:] != 0).any()
  f = _np(eng.factors())
  assert f.shape == (n_envs, 40, 10)
  want = _want_factors(st, pool, shape, angle, scale)
  for c, name in enumerate(FACTOR_COLUMNS):
    np.testing.assert_array_equal(_parity.bits(f[:, :, c]), _parity.bits(want[:, :, c]), err_msg=name)
  for env, k in ((0, 16), (1, 39), (n_envs - 1, 27)):
    assert eng.sprite_types(env, k) == (bool(pool.attr_f32[e[env], k] & 1), bool(pool.attr_f32[e[env], k] & 2)), (env, k)
  # setters on sprites beyond 16 of environment 1: its factors come from the setters' tables, the others' from the pool
  for k, attr, value in ((39, _abi.ATTR_SHAPE, float(shapes.shape_index('star_6'))), (17, _abi.ATTR_ANGLE, 133.5),
                         (30, _abi.ATTR_SCALE, 0.12)):
    eng.set_sprite_attr(1, k, attr, value)
    (shape, angle, scale)[attr][1, k] = value
  f = _np(eng.factors())
  want = _want_factors(eng.state(), pool, shape, angle, scale)
  for c, name in enumerate(FACTOR_COLUMNS):
    np.testing.assert_array_equal(_parity.bits(f[:, :, c]), _parity.bits(want[:, :, c]), err_msg=name + ' after setters')
  assert eng.sprite_types(1, 39) == (bool(pool.attr_f32[e[1], 39] & 1), bool(pool.attr_f32[e[1], 39] & 2))
  eng.close()


def device_sampler_case(total, num_envs=4, episodes_per_env=3):
  """swb_sample_pool with groups that add up to `total` sprites (40 or 64; shuffled): the pool equals the wide-slot model bit
  for bit, and the environment steps like the oracle on it.  (Sampler seed 12: among its 12 episodes of 54 .. 64 sprites one
  has 64; seed 11, the 40-sprite case's, draws none.)"""
  from oracle import oracle
  from spriteworld_amd import device_sampler, environment, lowering, shapes, sprite as sprite_lib, tasks
  from spriteworld_amd import action_spaces
  from spriteworld_amd import factor_distributions as distribs
  from spriteworld_amd import renderers as renderer_lib
  from tests import _sampler_model_wide
  first, rest, seed = {40: (10, (20, 31), 11), 64: (24, (30, 41), 12)}[total]
  common = [distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9),
            distribs.Discrete('shape', ['square', 'triangle', 'circle']), distribs.Discrete('scale', [0.05]),
            distribs.Continuous('c1', 0.3, 1.), distribs.Continuous('c2', 0.9, 1.)]
  target = distribs.Product(common + [distribs.Continuous('c0', 0., 0.4)])
  distractor = distribs.Product(common + [distribs.Continuous('c0', 0.5, 0.9)])
  sampler = device_sampler.DeviceSampler([(target, first), (distractor, rest)], shuffle=True, seed=seed)
  task = tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0., 0.4), terminate_distance=0.1)
  rend = {'image': renderer_lib.PILRenderer(image_size=(32, 32), anti_aliasing=3, color_to_rgb=renderer_lib.color_maps.hsv_to_rgb)}
  env = environment.BatchedEnvironment(task=task, action_space=action_spaces.SelectMove(scale=0.25), renderers=rend,
                                       init_sprites=sampler, max_episode_length=6, num_envs=num_envs,
                                       episodes_per_env=episodes_per_env, refresh_every=0)
  assert env._max_sprites == total
  sampler._draws -= 1
  seed = sampler.next_seed()
  label_fns = [(lambda f, sub=sub: lowering._label_of(sub, sprite_lib.Sprite(**f))) for sub in lowering.subtasks_of(task)]
  P = num_envs * episodes_per_env
  want = _sampler_model_wide.sample_pool(env._sampler_spec, P, total, seed, rend['image']._color_to_rgb, label_fns, shapes.SHAPE_NAMES)
  got = env.engine.get_pool()
  assert (got.n_sprites >= total - 10).all() and got.n_sprites.max() > total - 4
  if total == 64:
    assert got.n_sprites.max() == 64              # (every slot of the kernel's slot[SWB_MAX_SPRITES] in use)
  for name in ('n_sprites', 'x', 'y', 'x_vel', 'y_vel', 'scale', 'cos_a', 'sin_a', 'angle', 'shape', 'rgb', 'color', 'label'):
    np.testing.assert_array_equal(getattr(got, name), want[name], err_msg=name)
  ora = oracle.Engine(env.engine.cfg, got)
  rng = np.random.default_rng(5)
  for t in range(4):
    a = rng.uniform(0, 1, size=(num_envs, 4))
    want_o = ora.step(a)
    env.engine.step(a)
    _parity.compare(t, ora, env.engine, want_o, env.engine.outputs_host())
  env.close()


def wide_shapes_case(make_engine, n_vertices, embodied, n_envs, steps, aa=3):
  """ragged_s64 with the circle swapped for a regular polygon of 33 or 64 vertices: the hit test of the many-sprite state
  kernel builds such a path with lanes = vertices.  Episodes are capped at 60 sprites (60 x 64 = 3840 vertices fit the
  raster kernel's vertex budget at this canvas)."""
  from spriteworld_amd import shapes
  from tests import _util
  with _util.swapped_shape('circle', shapes.polygon(n_vertices)):
    cfg, pool, _ = workloads.build('ragged_s64_embodied' if embodied else 'ragged_s64', n_envs, episodes_per_env=2, anti_aliasing=aa)
    pool.n_sprites[:] = np.minimum(pool.n_sprites, 60)
    assert (pool.shape[0, :60] == shapes.shape_index('circle')).any()
    return run_scene(make_engine, (cfg, pool, aimed(cfg, n_envs)), steps, check_claims=False, want_most=60)
