"""The UNMODIFIED reference `Environment` stepped beside an engine on the same lowered episodes and the same actions (TEST
INFRASTRUCTURE ONLY): tests/test_oracle_vs_reference.py (the oracle), tests/test_emulated_kernel.py (the kernel source on the
host) and tests/test_gpu_vs_reference.py (the HIP engine) call it with seeds and lengths of their own.  The reference is loaded
through oracle.ref_harness; the callers skip where it is not available."""
import copy
import importlib

import numpy as np

from tests import _parity

_MODULES = ['spriteworld.configs.' + m for m in (
    'cobra.goal_finding_new_position', 'cobra.goal_finding_new_shape', 'cobra.goal_finding_more_distractors',
    'cobra.goal_finding_more_targets', 'cobra.clustering', 'cobra.sorting', 'cobra.exploration',
    'examples.goal_finding_embodied', 'examples.goal_finding_clustering')]
# every shipped config in both modes (tests/configs/configs_test.py:33-58 runs the same grid)
CONFIGS = [(m, mode) for m in _MODULES for mode in ('train', 'test')]


def fresh_episodes(episodes):
  """What the reference's init_sprites must return to follow the pool: the constructor's own draw (environment.py:68), then the
  episodes in order, wrapping around, as NEW sprite objects every time."""
  yield copy.deepcopy(episodes[0])
  while True:
    for e in episodes:
      yield copy.deepcopy(e)


def side_by_side(make_stepper, module, mode, seed, n_eps, n_steps):
  """Config `module` in `mode`: `n_eps` episodes drawn under np.random.seed(seed), lowered for `make_stepper(cfg, pool)` (the
  engine's step / outputs_host / state / close) and replayed by the reference; `n_steps` random actions -- no error flag, step
  types, rewards, success and sprite positions bit-exact, frames +-0, across resets."""
  from oracle import ref_harness
  ref_harness.load_reference()
  from spriteworld import environment
  from spriteworld import renderers as ref_renderers
  from spriteworld_amd import lowering
  np.random.seed(seed)
  config = importlib.import_module(module).get_config(mode)
  episodes = [config['init_sprites']() for _ in range(n_eps)]
  task, aspace, rends = config['task'], config['action_space'], config['renderers']
  S = max(len(e) for e in episodes)
  cfg = lowering.lower_config(task, aspace, rends, True, config['max_episode_length'], 1, S,
                              pos_is_f32=(lowering.position_dtype(episodes) == np.float32))
  pool = lowering.lower_episodes(episodes, task, rends, max_sprites=S).assign_round_robin(1)
  eng = make_stepper(cfg, pool)
  it = fresh_episodes(episodes)
  config = dict(config, init_sprites=lambda: next(it))
  config['renderers'] = dict(rends, success=ref_renderers.Success())
  env = environment.Environment(**config)
  rng = np.random.RandomState(seed + 1)
  for t in range(n_steps):
    if cfg.action_space == 2:
      a = np.array([rng.randint(0, 2), rng.randint(0, 4)])
      ts = env.step([int(a[0]), int(a[1])])
    else:
      a = rng.uniform(0, 1, 4)
      ts = env.step(a)
    eng.step(a[None])
    out = eng.outputs_host()
    assert not out['error'][0], t
    assert int(ts.step_type) == int(out['step_type'][0]), t
    r = np.nan if ts.reward is None else float(ts.reward)
    assert (np.isnan(r) and np.isnan(out['reward'][0])) or _parity.bits(r) == _parity.bits(out['reward'][0]), (t, r, out['reward'][0])
    assert bool(ts.observation['success']) == bool(out['success'][0]), t
    assert np.array_equal(ts.observation['image'], out['obs'][0]), t
    st = eng.state()
    pos = np.array([s.position for s in env._sprites], dtype=np.float64).reshape(-1, 2)
    n = st['n_sprites'][0]
    assert n == len(pos)
    assert np.array_equal(pos[:, 0], st['x'][0, :n]) and np.array_equal(pos[:, 1], st['y'][0, :n]), t
  eng.close()
