"""The general device sampler's scenarios (TEST INFRASTRUCTURE ONLY): generators and tasks DeviceSampler refuses, and the test
bodies that run on `environment.BatchedEnvironment` -- tests/test_gpu_sampler_tree.py calls them on the GPU,
tests/test_emulated_sampler_tree.py after putting the emulated engine in `environment._engine.Engine`'s place."""
import numpy as np

from spriteworld_amd import _abi
from spriteworld_amd import action_spaces
from spriteworld_amd import device_sampler
from spriteworld_amd import environment
from spriteworld_amd import factor_distributions as distribs
from spriteworld_amd import renderers as renderer_lib
from spriteworld_amd import sprite_generators
from spriteworld_amd import tasks

from tests import _parity
from tests import _sampler_tree_model

D = distribs
SHAPES3 = ['square', 'triangle', 'circle']


def _rend(aa=2):
  return {'image': renderer_lib.PILRenderer(image_size=(64, 64), anti_aliasing=aa, color_to_rgb=renderer_lib.color_maps.hsv_to_rgb)}


def _common():
  return [D.Continuous('x', 0.1, 0.9), D.Continuous('y', 0.1, 0.9), D.Discrete('shape', SHAPES3), D.Discrete('scale', [0.13]),
          D.Continuous('c1', 0.3, 1.), D.Continuous('c2', 0.9, 1.)]


def _hue_filter():
  """One wide generator, the task selects by the value drawn (a sprite_generators closure: device_reset='tree' lowers it)."""
  gen = sprite_generators.shuffle(sprite_generators.generate_sprites(
      D.Product(_common() + [D.Continuous('c0', 0., 1.)]), num_sprites=lambda: np.random.randint(2, 6)))
  task = tasks.FindGoalPosition(filter_distrib=D.Continuous('c0', 0., 0.4), terminate_distance=0.1)
  return gen, task, _rend()


def _hue_clusters():
  group = D.Product(_common() + [D.Continuous('c0', 0., 1.)])
  clusters = [D.Continuous('c0', 0., 0.2), D.Continuous('c0', 0.3, 0.5), D.Continuous('c0', 0.6, 0.8)]
  task = tasks.Clustering(clusters, terminate_bonus=0., reward_range=10.)
  return device_sampler.TreeSampler([(group, 4)], seed=2), task, _rend()


def _edge_f32():
  """np.float32(0.7) >= 0.7 holds in float32 and fails in float64; np.float32(0.7) in [0.7] holds."""
  group = D.Product([D.Continuous('x', 0.1, 0.9), D.Continuous('y', 0.1, 0.9), D.Continuous('c0', 0.7, 0.7),
                     D.Continuous('c1', 0.7, 0.7), D.Discrete('c2', [0.7, 1.]), D.Continuous('scale', 0.1, 0.2)])
  subs = [tasks.FindGoalPosition(filter_distrib=D.Continuous('c0', 0.7, 1.), terminate_distance=0.1),
          tasks.FindGoalPosition(filter_distrib=D.Discrete('c1', [0.7]), terminate_distance=0.1),
          tasks.FindGoalPosition(filter_distrib=D.Continuous('c2', 0.7, 0.8), terminate_distance=0.1)]    # Python floats: float64
  return device_sampler.TreeSampler([(group, 2)], seed=3), tasks.MetaAggregated(subs, reward_aggregator='sum'), _rend()


def _position_group():
  return D.Product([D.Continuous('x', 0.05, 0.95), D.Continuous('y', 0.05, 0.95), D.Discrete('shape', ['square', 'triangle', 'star_5', 'circle']),
                    D.Continuous('angle', 0, 360, dtype='int32'), D.Discrete('scale', [0.12, 0.2]), D.Continuous('c0', 0., 1.),
                    D.Discrete('c1', [0.9]), D.Discrete('c2', [1.0])])


def _pos_goal():
  task = tasks.FindGoalPosition(filter_distrib=D.Continuous('x', 0., 0.5), goal_position=(0.75, 0.5), terminate_distance=0.2)
  return device_sampler.TreeSampler([(_position_group(), (3, 6))], shuffle=True, seed=4), task, _rend()


def _meta_swap():
  left = tasks.FindGoalPosition(filter_distrib=D.Continuous('x', 0., 0.5), goal_position=(0.75, 0.5), terminate_distance=0.3)
  right = tasks.FindGoalPosition(filter_distrib=D.Continuous('x', 0.5, 1.5), goal_position=(0.25, 0.5), terminate_distance=0.3)
  task = tasks.MetaAggregated([left, right], reward_aggregator='sum', termination_criterion='any', terminate_bonus=1.)
  return device_sampler.TreeSampler([(_position_group(), 4)], seed=5), task, _rend()


def mixture_distribution():
  warm = D.Product([D.Continuous('c0', 0., 0.2), D.Discrete('scale', [0.1, 0.15, 0.2], probs=[0.6, 0.3, 0.1])])
  cold = D.Product([D.Continuous('c0', 0.5, 0.7), D.Discrete('scale', [0.12])])
  return D.Product([D.Continuous('x', 0.1, 0.9), D.Continuous('y', 0.1, 0.9), D.Mixture([warm, cold], probs=[0.2, 0.8]),
                    D.Discrete('shape', SHAPES3, probs=[0.5, 0.25, 0.25]), D.Continuous('c1', 0.3, 1.), D.Continuous('c2', 0.9, 1.)])


def _mixture():
  """A weighted Mixture, weighted Discrete factors (shape too) and a weighted sample_generator, as closures."""
  dist = mixture_distribution()
  gen = sprite_generators.sample_generator([sprite_generators.generate_sprites(dist, 2), sprite_generators.generate_sprites(dist, 3)],
                                           p=[0.7, 0.3])
  task = tasks.FindGoalPosition(filter_distrib=D.Continuous('c0', 0., 0.2), terminate_distance=0.1)
  return gen, task, _rend()


def nested_distribution():
  base = D.Product([D.Continuous('x', 0.1, 0.9), D.Continuous('y', 0.1, 0.9), D.Discrete('shape', SHAPES3), D.Continuous('scale', 0.05, 0.2)])
  inner = D.SetMinus(base, D.Product([D.Continuous('x', 0.3, 0.9), D.Continuous('y', 0.3, 0.9)]))
  outer = D.SetMinus(inner, D.Product([D.Discrete('shape', ['circle', 'triangle']), D.Continuous('scale', 0.05, 0.15)]))
  hue = D.Intersection([D.Continuous('c0', 0., 0.6), D.Continuous('c0', 0.4, 1.)], index_for_sampling=1)
  rest = D.Selection(D.Product([D.Continuous('c1', 0., 1.), D.Continuous('c2', 0.5, 1.)]), D.Continuous('c1', 0.6, 1.))
  return D.Product([outer, hue, rest]), inner, outer


def _nested():
  dist, _, _ = nested_distribution()
  task = tasks.FindGoalPosition(filter_distrib=D.Continuous('c0', 0.4, 0.5), terminate_distance=0.1)
  return device_sampler.TreeSampler([(dist, (1, 4))], shuffle=True, seed=6), task, _rend()


def _exhaust():
  group = D.Product([D.Continuous('x', 0.1, 0.9), D.Continuous('y', 0.1, 0.9),
                     D.Selection(D.Continuous('c0', 0., 1.), D.Continuous('c0', 2., 3.)), D.Discrete('c1', [1.]), D.Discrete('c2', [1.])])
  return device_sampler.TreeSampler([(group, (1, 4))], seed=7, max_tries=50), tasks.NoReward(), _rend()


CASES = {'hue_filter': _hue_filter, 'hue_clusters': _hue_clusters, 'edge_f32': _edge_f32, 'pos_goal': _pos_goal, 'meta_swap': _meta_swap,
         'mixture': _mixture, 'nested': _nested, 'exhaust': _exhaust}
FIELDS = ('n_sprites', 'x', 'y', 'x_vel', 'y_vel', 'scale', 'cos_a', 'sin_a', 'angle', 'shape', 'rgb', 'color', 'label', 'attr_f32')


def make_env(case, num_envs=16, episodes_per_env=3, seed=11, **kwargs):
  """(environment, its TreeSampler, task, renderers).  Generators go through device_reset='tree', samplers as they are."""
  init, task, rend = CASES[case]()
  kwargs.setdefault('action_space', action_spaces.SelectMove(scale=0.6, motion_cost=0.1))
  env = environment.BatchedEnvironment(task=task, renderers=rend, init_sprites=init, max_episode_length=12, num_envs=num_envs,
                                       episodes_per_env=episodes_per_env, refresh_every=0, device_reset='tree', seed=seed,
                                       check_errors=0, **kwargs)
  assert isinstance(env._sampler, device_sampler.TreeSampler), type(env._sampler)
  return env, env._sampler, task, rend


def model_pool(env, sampler, task, rend, seed, n_entries=None, first_entry=0):
  return _sampler_tree_model.sample_pool(sampler, task, rend['image']._color_to_rgb, n_entries or env.num_envs * env._episodes_per_env,
                                         env._max_sprites, seed, first_entry=first_entry)


def assert_pool_equals(got, want, what=''):
  for name in FIELDS:
    np.testing.assert_array_equal(getattr(got, name), want[name], err_msg='%s %s' % (name, what))
  if got.cell_label is not None:
    np.testing.assert_array_equal(got.cell_label, want['cell_label'], err_msg='cell_label ' + what)
  else:
    assert not want['cell_label'].any()


def last_seed(sampler):
  sampler._draws -= 1
  return sampler.next_seed()   # the key the last (re)sample call used


def assert_model_exercises(case, want, loops):
  """What the issue asks of the MODEL's pool, so that a case cannot pass by never reaching its subject."""
  n, lab = want['n_sprites'], want['label']
  live = np.arange(lab.shape[2])[None, :] < n[:, None]
  if case == 'hue_filter':
    assert any(set(lab[e, 0, :n[e]]) == {0, 1} for e in range(len(n)))
  elif case == 'hue_clusters':
    assert set(lab[:, 0][live]) == {-1, 0, 1, 2}
  elif case == 'edge_f32':
    assert (lab[:, 0][live] == 1).all() and (lab[:, 1][live] == 1).all() and set(lab[:, 2][live]) == {0, 1}
    assert np.float64(np.float32(0.7)) < 0.7          # (a float64 compare gives 0)
  elif case in ('pos_goal', 'meta_swap'):
    assert set(lab[:, 0][live]) == {0, 1}
    cells = want['cell_label'][:, 0][live]
    assert (cells[:, :3] == [0, 1, 0]).all() and not cells[:, 3:].any()      # x < 0, [0, 0.5), >= 0.5: both used
  elif case == 'nested':
    per_loop = {}       # (the four rejection loops: inner and outer SetMinus, Intersection, Selection)
    for d in loops:
      for k, v in d.items():
        per_loop.setdefault(k, []).append(v)
    assert len(per_loop) == 4 and all(max(v) >= 2 for v in per_loop.values()), {k: max(v) for k, v in per_loop.items()}


def pool_matches_the_model_case(case, num_envs=16, episodes_per_env=3):
  env, sampler, task, rend = make_env(case, num_envs, episodes_per_env)
  for refill in range(2):
    want, exhausted, loops = model_pool(env, sampler, task, rend, last_seed(sampler))
    if refill == 0:
      assert_model_exercises(case, want, loops)
    assert_pool_equals(env.engine.get_pool(), want, '(%s, refill %d)' % (case, refill))
    assert env.engine.sampler_exhausted() == exhausted
    if case == 'exhaust':
      assert exhausted == want['n_sprites'].sum() > 0
      try:
        env.check()
      except environment.EnvironmentError_ as e:
        assert 'max_tries = 50' in str(e)
      else:
        raise AssertionError('check() did not raise')
    else:
      assert exhausted == 0
      env.check()
    env.refill_pool()
  env.close()


def odd_sizes_case():
  """P = 257: a second block with one live thread; a first_entry with a non-zero high word."""
  env, sampler, task, rend = make_env('nested', num_envs=4)
  spec = env._sampler_spec
  for P, first in ((257, 0), (5, (3 << 32) + 0xFFFFFFFE)):     # (the second: entries whose low word wraps)
    env.engine.sample_pool_tree(spec, P, np.zeros(4, np.int32), np.full(4, P, np.int32), 99, first_entry=first)
    want, _, _ = model_pool(env, sampler, task, rend, 99, n_entries=P, first_entry=first)
    assert_pool_equals(env.engine.get_pool(), want, '(P = %d)' % P)
  env.close()


def shards_case():
  """global_env_offset: two 8-env shards hold the same pool as one 16-env process."""
  whole, _, _, _ = make_env('mixture', num_envs=16)
  want = whole.engine.get_pool()
  for rank in range(2):
    shard, _, _, _ = make_env('mixture', num_envs=8, global_env_offset=8 * rank)
    got = shard.engine.get_pool()
    for name in FIELDS:
      np.testing.assert_array_equal(getattr(got, name), getattr(want, name)[24 * rank:24 * (rank + 1)], err_msg=name)
    shard.close()
  whole.close()


def refresh_case():
  """swb_resample_pool after a tree fill: all but the live entries are redrawn, by the tree kernel (the model's pool)."""
  env, sampler, task, rend = make_env('pos_goal', num_envs=16, episodes_per_env=4)
  env.reset()
  for _ in range(15):                     # max_episode_length = 12: every environment is in its 2nd episode
    env.step(env.sample_actions())
  before, st = env.engine.get_pool(), env.state()
  env.refresh_pool()
  after = env.engine.get_pool()
  want, _, _ = model_pool(env, sampler, task, rend, last_seed(sampler))
  live = st['pool_entry']
  assert np.array_equal(live // 4, np.arange(16))
  idle = np.setdiff1d(np.arange(64), live)
  for name in FIELDS + ('cell_label',):
    np.testing.assert_array_equal(getattr(after, name)[idle], want[name][idle], err_msg=name)
    np.testing.assert_array_equal(getattr(after, name)[live], getattr(before, name)[live], err_msg=name)
  assert (before.x[idle] != after.x[idle]).any(axis=1).all()
  st2 = env.state()
  assert np.array_equal(st2['step_count'], st['step_count']) and np.array_equal(st2['x'], st['x'])
  env.check()
  env.close()


def parity_case(case, click, seed, steps=40, num_envs=6):
  """An environment on a tree-sampled pool steps bit-equal to an engine given the same pool through swb_set_pool, and to the
  oracle (tests/_parity.py).  Keyed cases: on the oracle, some sprite changes cell inside an episode."""
  from oracle import oracle
  env, _, task, _ = make_env(case, num_envs=num_envs)
  pool = env.engine.get_pool()
  twin, ora = environment._engine.Engine(env._cfg, pool), oracle.Engine(env._cfg, pool)
  env.seed_actions(seed)
  keyed = any(t.n_xcuts for t in env._cfg.tasks[:env._cfg.n_tasks])       # (both keyed cases cut x at 0.5)
  crossed, prev = 0, None
  for t in range(steps):
    a = env.sample_actions(where='device', click=click)
    env.engine.step(a)
    a = a.cpu().numpy()
    twin.step(a)
    want = ora.step(a)
    _parity.compare(t, ora, env.engine, want, env.engine.outputs_host(), what=case + ' sampled')
    st = _parity.compare(t, ora, twin, want, twin.outputs_host(), what=case + ' set_pool')
    if prev is not None and keyed:
      same = (st['episode'] == prev['episode']) & (st['step_count'] == prev['step_count'] + 1)
      live = np.arange(st['x'].shape[1])[None, :] < st['n_sprites'][:, None]
      crossed += int((((st['x'] >= 0.5) != (prev['x'] >= 0.5)) & live & same[:, None]).sum())
    prev = st
  if keyed:
    assert crossed > 0
  twin.close()
  env.close()


def setter_keeps_cell_labels_case():
  """A setter on a keyed, tree-sampled handle copies the entry's cell labels into the environment's overrides: an angle
  change (which no label depends on) leaves every reward as it is in a twin environment without it."""
  envs = [make_env('pos_goal', num_envs=4)[0] for _ in range(2)]
  for env in envs:
    env.seed_actions(5)
    env.reset()
  pool, st = envs[0].engine.get_pool(), envs[0].state()
  e, k = [(e, k) for e in range(4) for k in range(st['n_sprites'][e]) if st['x'][e, k] < 0.3][0]     # a sprite of label 1 where it stands
  assert pool.cell_label[st['pool_entry'][e], 0, k, :3].tolist() == [0, 1, 0]
  envs[0].engine.set_sprite_attr(e, k, _abi.ATTR_ANGLE, 30.)
  seen = set()
  for _ in range(10):
    steps = [env.step(env.sample_actions(where='device', click='sprite')) for env in envs]
    _parity.assert_rewards_equal(steps[0].reward.cpu().numpy(), steps[1].reward.cpu().numpy(), 'after the setter')
    st = envs[0].state()
    if st['episode'][e] == 1:
      seen.add(bool(st['x'][e, k] >= 0.5))
  assert False in seen                # (the sprite stood in the cell of label 1 while the override was live)
  for env in envs:
    env.close()
