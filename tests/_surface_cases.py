"""The host-surface scenarios that run on `environment.Environment` / `BatchedEnvironment` (TEST INFRASTRUCTURE ONLY): the
dm_env conformance checks, the reference's gym-wrapper episode pattern, the example run loop and the SpriteFactors observation.
tests/test_env_spec_conformance.py, test_gym_wrapper.py and test_host_api.py call them on the GPU, tests/test_emulated_kernel.py
after putting the emulated engine in `environment._engine.Engine`'s place."""
import numpy as np

from spriteworld_amd import action_spaces, gym_wrapper, renderers, sprite_generators, tasks
from spriteworld_amd import dm_env_compat as dm_env
from spriteworld_amd import factor_distributions as distribs
from spriteworld_amd.sprite import Sprite


def _cobra_like_config(n_targets=2, n_distractors=1):
  shared = distribs.Product([
      distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9),
      distribs.Discrete('shape', ['square', 'triangle', 'circle']), distribs.Discrete('scale', [0.13]),
      distribs.Continuous('c1', 0.3, 1.), distribs.Continuous('c2', 0.9, 1.)])
  target_hue, distractor_hue = distribs.Continuous('c0', 0., 0.4), distribs.Continuous('c0', 0.5, 0.9)
  gen = sprite_generators.shuffle(sprite_generators.chain_generators(
      sprite_generators.generate_sprites(distribs.Product([target_hue, shared]), num_sprites=n_targets),
      sprite_generators.generate_sprites(distribs.Product([distractor_hue, shared]), num_sprites=n_distractors)))
  return {
      'task': tasks.FindGoalPosition(filter_distrib=target_hue, terminate_distance=0.075),
      'action_space': action_spaces.SelectMove(scale=0.25),
      'renderers': {'image': renderers.PILRenderer(image_size=(64, 64), anti_aliasing=5,
                                                   color_to_rgb=renderers.hsv_to_rgb)},
      'init_sprites': gen,
      'max_episode_length': 20,
      'metadata': {'name': 'test', 'mode': 'train'},
  }


def _conforms(value, spec):
  """dm_env.test_utils.EnvironmentTestMixin.assertConformsToSpec (spec.validate)."""
  a = np.asarray(value)
  assert a.shape == tuple(spec.shape), (a.shape, spec.shape)
  assert a.dtype == np.dtype(spec.dtype), (a.dtype, spec.dtype)
  if hasattr(spec, 'minimum'):
    assert np.all(a >= spec.minimum) and np.all(a <= spec.maximum), (a, spec.minimum, spec.maximum)


def _valid_step(env, ts):
  assert isinstance(ts, dm_env.TimeStep)
  assert isinstance(ts.step_type, dm_env.StepType)
  if ts.step_type == dm_env.StepType.FIRST:
    assert ts.reward is None and ts.discount is None
  else:
    _conforms(ts.reward, env.reward_spec())
    _conforms(ts.discount, env.discount_spec())
  spec = env.observation_spec()
  assert set(ts.observation) == set(spec)
  for k, v in ts.observation.items():
    _conforms(v, spec[k])


def _reference_test_env():
  """make_object_under_test of tests/environment_test.py:42-51."""
  from spriteworld_amd import environment
  return environment.Environment(task=tasks.NoReward(), action_space=action_spaces.SelectMove(), renderers={},
                                 init_sprites=lambda: [Sprite(c0=255)], max_episode_length=7)


def _rendered_env():
  from spriteworld_amd import environment
  rend = {'image': renderers.PILRenderer(image_size=(64, 64), anti_aliasing=5, color_to_rgb=renderers.hsv_to_rgb),
          'success': renderers.Success()}
  return environment.Environment(task=tasks.FindGoalPosition(terminate_distance=0.2), action_space=action_spaces.SelectMove(scale=0.5),
                                 renderers=rend, init_sprites=lambda: [Sprite(x=0.2, y=0.3, c0=0.3, c1=0.8, c2=0.9),
                                                                       Sprite(x=0.7, y=0.6, shape='circle', c0=0.6, c1=0.9, c2=1.0)],
                                 max_episode_length=9)


def reset_and_step_protocol_case(make):
  env = make()                                        # test_reset / test_reset_on_new_env
  ts = env.reset()
  assert ts.first()
  _valid_step(env, ts)
  env.close()
  env = make()                                        # test_step_on_fresh_environment: the first step is a reset
  a = env.action_space.sample()
  ts = env.step(a)
  assert ts.first()
  _valid_step(env, ts)
  ts = env.step(a)                                    # test_step_after_reset
  assert not ts.first()
  _valid_step(env, ts)
  env.close()


def longer_action_sequence_case(make):
  env = make()
  np.random.seed(5)
  ts = env.reset()
  prev_last = False
  seen = set()
  for _ in range(40):
    a = env.action_space.sample()
    spec = env.action_spec()
    assert np.asarray(a).shape == tuple(spec.shape) and np.asarray(a).dtype.kind == 'f'
    assert np.all(np.asarray(a) >= spec.minimum) and np.all(np.asarray(a) <= spec.maximum)
    ts = env.step(a)
    _valid_step(env, ts)
    assert ts.first() == prev_last                    # auto-reset: FIRST exactly after a LAST step
    prev_last = ts.last()
    seen.add(int(ts.step_type))
  assert seen == {0, 1, 2}
  env.close()


def specs_are_specs_case():
  env = _rendered_env()
  obs = env.observation_spec()
  assert tuple(obs['image'].shape) == (64, 64, 3) and obs['image'].dtype == np.uint8
  assert tuple(obs['success'].shape) == () and obs['success'].dtype == np.bool_
  assert tuple(env.reward_spec().shape) == () and np.dtype(env.reward_spec().dtype).kind == 'f'
  d = env.discount_spec()
  assert float(d.minimum) == 0.0 and float(d.maximum) == 1.0
  env.close()


def reference_gym_wrapper_episode_pattern_case(embodied):
  """tests/gym_wrapper_test.py:38-111: spaces, then 3 episodes of max_episode_length = 5 with the
  done flag only on the last step and a not-done (auto-reset) step after it."""
  from spriteworld_amd import environment
  spaces = gym_wrapper.spaces
  space = action_spaces.Embodied() if embodied else action_spaces.SelectMove()
  env = gym_wrapper.GymWrapper(environment.Environment(
      tasks.NoReward(), space, {'image': renderers.PILRenderer(image_size=(64, 64))},
      lambda: [Sprite(c0=255)], max_episode_length=5))
  assert env.observation_space == spaces.Dict({'image': spaces.Box(-np.inf, np.inf, shape=(64, 64, 3), dtype=np.uint8)})
  if embodied:
    assert env.action_space == spaces.Tuple([spaces.Discrete(2), spaces.Discrete(4)])
  else:
    assert env.action_space == spaces.Box(0., 1., shape=(4,), dtype=np.float32)
  np.random.seed(0)
  for _ in range(3):
    env.reset()
    for _ in range(4):
      obs, reward, done, _ = env.step(env.action_space.sample())
      assert obs['image'].dtype == np.uint8 and not done and reward == 0.
    _, _, done, _ = env.step(env.action_space.sample())
    assert done
    _, _, done, _ = env.step(env.action_space.sample())
    assert not done


def single_environment_run_loop_case():
  """example_run_loop.py:62-80: reset(), step(action_space.sample()) until last(), log success."""
  from spriteworld_amd import environment
  np.random.seed(3)
  config = _cobra_like_config()
  config['renderers']['success'] = renderers.Success()
  env = environment.Environment(**config)
  for _ in range(3):
    timestep = env.reset()
    assert timestep.first() and timestep.reward is None and timestep.discount is None
    rewards, n = [], 0
    while not timestep.last():
      timestep = env.step(env.action_space.sample())
      rewards.append(timestep.reward)
      n += 1
    assert n <= 20 and timestep.discount == 0.0
    assert isinstance(timestep.observation['success'], bool)
    assert timestep.observation['image'].shape == (64, 64, 3) and np.isfinite(np.nanmean(rewards))
  env.close()


def sprite_factors_and_action_noise_case():
  """handcrafted.SpriteFactors as a batched tensor, and SelectMove(noise_scale=...) noise."""
  from spriteworld_amd import environment
  np.random.seed(4)
  config = _cobra_like_config()
  config['renderers'] = {'factors': renderers.SpriteFactors(), 'xy': renderers.SpriteFactors(factors=('y', 'x', 'shape'))}
  config['action_space'] = action_spaces.SelectMove(scale=0.25, noise_scale=0.05)
  env = environment.BatchedEnvironment(num_envs=32, episodes_per_env=2, device_reset=False, **config)   # host pool: compared below
  env.seed_noise(0)
  ts = env.reset()
  f = ts.observation['factors'].cpu().numpy()
  assert f.shape == (32, 3, 10) and ts.observation['xy'].shape == (32, 3, 3)
  pool, st = env.engine.pool, env.state()
  for n in range(32):
    e = st['pool_entry'][n]
    assert np.array_equal(f[n, :, 0], st['x'][n]) and np.array_equal(f[n, :, 1], st['y'][n])
    assert np.array_equal(f[n, :, 2], pool.shape[e] + 1) and np.array_equal(f[n, :, 4], pool.scale[e])
    assert np.array_equal(f[n, :, 5:8], pool.color[e]) and np.array_equal(f[n, :, 3], pool.angle[e])
  assert np.array_equal(ts.observation['xy'].cpu().numpy(), f[:, :, [1, 0, 2]])
  # noise: the same clean action moves sprites by different amounts in different environments
  a = np.tile(np.array([[0.5, 0.5, 0.9, 0.9]]), (32, 1))
  env.engine.set_positions(np.full((32, 3), 0.5), np.full((32, 3), 0.5))
  ts = env.step(a)
  moved = ts.observation['factors'][:, 2, 0].cpu().numpy() - 0.5
  hit = moved != 0                      # a noised click may miss the sprite
  assert hit.sum() >= 8 and np.all(np.abs(moved[hit] - 0.1) < 0.1) and np.std(moved[hit]) > 1e-3
  env.close()
