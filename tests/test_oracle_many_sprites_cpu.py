"""Pins the oracle at more than 16 sprites per environment (up to the engine's 64) against the UNMODIFIED reference imported
from /root/reference (build container only; skipped where the reference tree is absent), as
test_oracle_vs_reference.py::test_ragged_episodes_from_empty_to_sixteen_sprites does up to 16: every action space, every task
kind, float32 and float64 positions; step types, rewards (as bits), positions and frames +-0."""
import copy

import numpy as np
import pytest

from oracle import ref_harness

pytestmark = pytest.mark.skipif(not ref_harness.reference_available(),
                                reason='the reference tree is not present on this machine')

COUNTS = [17, 0, 64, 1, 33, 20, 64, 2, 40, 17, 50, 5]


def _fresh_episodes(episodes):
  yield copy.deepcopy(episodes[0])
  while True:
    for e in episodes:
      yield copy.deepcopy(e)


def _bits(v):
  return np.float64(v).view(np.uint64)


@pytest.mark.parametrize('space,task_kind,f32', [('select', 'goal', True), ('drag', 'cluster', True), ('embodied', 'goal', False),
                                                 ('select', 'meta', False), ('drag', 'cluster', False), ('embodied', 'meta', True),
                                                 ('select', 'cluster', True)])
def test_ragged_episodes_of_17_to_64_sprites(space, task_kind, f32):
  _ragged_episodes(space, task_kind, f32)


def test_ragged_episodes_of_17_to_64_sprites_on_a_1280_pixel_canvas():
  """The reference's own renderer at 256 x 256, anti_aliasing 5: the scene the GPU tests of the many-sprite path on large frames
  hold the kernels to."""
  _ragged_episodes('select', 'goal', True, image_size=(256, 256), steps=24)


def _ragged_episodes(space, task_kind, f32, image_size=(64, 64), steps=60):
  ref_harness.load_reference()
  from spriteworld import action_spaces, environment, renderers, sprite, tasks
  from spriteworld import factor_distributions as distribs
  from oracle import oracle
  from spriteworld_amd import lowering
  rng = np.random.RandomState(23)
  num = np.float32 if f32 else float

  def gen(n):
    return [sprite.Sprite(x=num(rng.uniform(0.05, 0.95)), y=num(rng.uniform(0.05, 0.95)),
                          shape=str(rng.choice(['square', 'triangle', 'circle', 'star_4'])),
                          scale=float(rng.choice([0.04, 0.08])), c0=np.float32(rng.uniform(0, 1)),
                          c1=np.float32(0.8), c2=np.float32(1.0)) for _ in range(n)]

  # Clustering with 12 clusters (bands of hue): a 12 x 12 Davies-Bouldin ratio matrix; 8 with float64 positions (from about 12
  # clusters on, scikit-learn's float64 distances take BLAS paths whose FMA order the oracle does not model: DESIGN.md section 13)
  kc = 12 if f32 else 8
  clusters = [distribs.Continuous('c0', i / float(kc), (i + 1) / float(kc)) for i in range(kc)]
  counts = COUNTS if task_kind == 'goal' else [c for c in COUNTS if c >= 17]     # (Davies-Bouldin needs 1 < k < m)
  if task_kind == 'goal':
    task = tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0., 0.3), terminate_distance=0.1)
  elif task_kind == 'cluster':
    task = tasks.Clustering(clusters, termination_threshold=1.5, terminate_bonus=1., reward_range=6.)
  else:
    task = tasks.MetaAggregated([tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0., 0.3), goal_position=(0.2, 0.8),
                                                        terminate_distance=0.1),
                                 tasks.Clustering(clusters, termination_threshold=1.5, reward_range=6.),
                                 tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0.5, 1.), terminate_distance=0.1)],
                                reward_aggregator='mean', termination_criterion='any', terminate_bonus=2.)
  aspace = {'select': action_spaces.SelectMove(scale=0.4, motion_cost=0.3),
            'drag': action_spaces.DragAndDrop(scale=0.5),
            'embodied': action_spaces.Embodied(step_size=0.1)}[space]
  if space == 'embodied':       # Embodied needs a body: the reference indexes sprites[-1] (action_spaces.py:195)
    counts = [c for c in counts if c]
  episodes = [gen(n) for n in counts]
  rends = {'image': renderers.PILRenderer(image_size=image_size, anti_aliasing=5, color_to_rgb=renderers.color_maps.hsv_to_rgb),
           'success': renderers.Success()}
  cfg = lowering.lower_config(task, aspace, rends, True, 6, 1, 64, pos_is_f32=f32)
  pool = lowering.lower_episodes(episodes, task, rends, max_sprites=64).assign_round_robin(1)
  eng = oracle.Engine(cfg, pool)
  it = _fresh_episodes(episodes)
  env = environment.Environment(task=task, action_space=aspace, renderers=rends, init_sprites=lambda: next(it),
                                max_episode_length=6)
  arng = np.random.RandomState(3)
  most = 0
  for t in range(steps):
    if space == 'embodied':
      a = np.array([arng.randint(0, 2), arng.randint(0, 4)])
      ts = env.step([int(a[0]), int(a[1])])
    else:
      a = arng.uniform(0, 1, 4)
      ts = env.step(a)
    out = eng.step(a[None])
    assert int(ts.step_type) == int(out['step_type'][0]), t
    r = np.nan if ts.reward is None else float(ts.reward)
    assert (np.isnan(r) and np.isnan(out['reward'][0])) or _bits(r) == _bits(out['reward'][0]), (t, r, out['reward'][0])
    assert bool(ts.observation['success']) == bool(out['success'][0]), t
    st = eng.state()
    pos = np.array([sp.position for sp in env._sprites], dtype=np.float64).reshape(-1, 2)
    n = st['n_sprites'][0]
    assert n == len(pos)
    most = max(most, n)
    assert np.array_equal(pos[:, 0], st['x'][0, :n]) and np.array_equal(pos[:, 1], st['y'][0, :n]), t
    assert np.array_equal(ts.observation['image'], out['obs'][0]), t
  assert most > 16


def test_davies_bouldin_of_64_points_equals_sklearn():
  """Up to 64 points in up to 63 clusters with float32 positions, up to 9 clusters with float64 positions (see above)."""
  metrics = pytest.importorskip('sklearn.metrics')
  from oracle import oracle
  rng = np.random.default_rng(8)
  for _ in range(300):
    n = int(rng.integers(17, 65))
    f32 = rng.random() < 0.5
    k = int(rng.integers(2, min(n, 64 if f32 else 10)))
    labels = rng.integers(-1, k, size=n).astype(np.int8)
    pos = rng.uniform(0, 1, size=(n, 2)).astype(np.float32 if f32 else np.float64)
    keep = labels >= 0
    uniq = np.unique(labels[keep])
    err, score = oracle.davies_bouldin(f32, pos[:, 0].astype(np.float64), pos[:, 1].astype(np.float64), labels)
    if not (1 < len(uniq) < keep.sum()):
      assert err == 2
      continue
    ref = metrics.davies_bouldin_score(pos[keep], labels[keep])
    assert err == 0
    assert np.float64(ref).view(np.uint64) == np.float64(score).view(np.uint64), (n, k, ref, score)
