"""`BatchedEnvironment.step(active=...)`, `reset(envs=...)` and `run_episodes` against the oracle: on the
emulated engine (CPU) and, marked `gpu`, on the device.  The environments draw their episodes on the host (an opaque
`init_sprites`), so the oracle plays the very pool the engine holds."""
import numpy as np
import pytest
import torch

from spriteworld_amd import _abi
from tests import _masked_step_cases as cases
from tests import _parity

BACKENDS = [pytest.param('emu'), pytest.param('gpu', marks=pytest.mark.gpu)]
MAX_LEN = 6


def _environment(monkeypatch, backend, n_envs):
  from spriteworld_amd import action_spaces, environment, renderers, sprite_generators, tasks
  from spriteworld_amd import factor_distributions as distribs
  if backend == 'emu':
    from tests import _emu_engine
    monkeypatch.setattr(environment._engine, 'Engine', _emu_engine.EmuTorchEngine)
  np.random.seed(7)
  common = [distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9),
            distribs.Discrete('shape', ['square', 'triangle', 'circle']), distribs.Discrete('scale', [0.2]),
            distribs.Continuous('c1', 0.3, 1.), distribs.Continuous('c2', 0.9, 1.)]
  gen = sprite_generators.chain_generators(
      sprite_generators.generate_sprites(distribs.Product(common + [distribs.Continuous('c0', 0., 0.4)]), num_sprites=2),
      sprite_generators.generate_sprites(distribs.Product(common + [distribs.Continuous('c0', 0.5, 0.9)]), num_sprites=2))
  task = tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0., 0.4), terminate_distance=0.25)
  rend = {'image': renderers.PILRenderer(image_size=(64, 64), anti_aliasing=5, color_to_rgb=renderers.color_maps.hsv_to_rgb)}
  env = environment.BatchedEnvironment(task=task, action_space=action_spaces.SelectMove(scale=0.25), renderers=rend,
                                       init_sprites=gen, max_episode_length=MAX_LEN, num_envs=n_envs, episodes_per_env=4,
                                       device_reset=False, check_errors=1)
  assert env.engine.pool is not None
  return env


def _runner(monkeypatch, env, bank=False):
  """tests/_masked_step_cases.Runner around the environment's own engine: its oracle and its record of the held outputs."""
  return cases.Runner(lambda cfg, pool: env.engine, monkeypatch, env._cfg, env.engine.pool, 'environment', bank=bank)


def _check(r, env, ts, want):
  e = env.engine
  assert ts.step_type is e.step_type and ts.reward is e.reward and ts.discount is e.discount and ts.observation['image'] is e.obs
  _parity.compare(r.t, r.ora, e, want, e.outputs_host(), what='environment')
  r.held = want
  r.t += 1


@pytest.mark.parametrize('backend', BACKENDS)
def test_step_with_a_mask(monkeypatch, backend):
  n = 7 if backend == 'emu' else 33
  env = _environment(monkeypatch, backend, n)
  r = _runner(monkeypatch, env)
  null = env.null_actions().cpu().numpy()
  _check(r, env, env.reset(), r.expected(null, None))
  rng = np.random.default_rng(3)
  for t in range(16):
    active = rng.random(n) < 0.6
    if t == 5:
      active[:] = False
    a = rng.uniform(0., 1., size=(n, 4))
    want = r.expected(a, active)
    mask = active if t % 2 else torch.as_tensor(active.astype(np.uint8))      # (bool array, uint8 tensor)
    _check(r, env, env.step(cases.poison(env._cfg, a, active), active=mask), want)
  assert r.saw_inactive_pending and r.saw_first_after_hold
  env.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_reset_of_some_environments(monkeypatch, backend):
  n = 6 if backend == 'emu' else 33
  env = _environment(monkeypatch, backend, n)
  r = _runner(monkeypatch, env, bank=True)
  null = env.null_actions().cpu().numpy()
  _check(r, env, env.reset(), r.expected(null, None))
  rng = np.random.default_rng(4)
  for _ in range(2):
    a = rng.uniform(0., 1., size=(n, 4))
    _check(r, env, env.step(a), r.expected(a, None))
  marked = (np.arange(n) % 3) == 1
  before = env.state()
  r.ora.reset(marked)
  want = r.expected(null, marked)
  ts = env.reset(envs=marked)
  _check(r, env, ts, want)
  st = env.state()
  assert (ts.step_type.cpu().numpy()[marked] == _abi.STEP_FIRST).all()
  assert (st['episode'] == before['episode'] + marked).all() and (st['step_count'][~marked] == before['step_count'][~marked]).all()
  for _ in range(4):
    a = rng.uniform(0., 1., size=(n, 4))
    _check(r, env, env.step(a), r.expected(a, None))
  env.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_bad_masks_raise(monkeypatch, backend):
  n = 4
  env = _environment(monkeypatch, backend, n)
  env.reset()
  a = env.null_actions()
  for bad in (np.ones(n), np.ones(n, np.int64), np.ones(n + 1, bool), np.ones((n, 1), bool), torch.ones(n, dtype=torch.float32), 'all',
              [object()] * n):
    with pytest.raises(ValueError):
      env.step(a, active=bad)
    with pytest.raises(ValueError):
      env.reset(envs=bad)
    with pytest.raises(ValueError):
      env.engine.reset_envs(bad)
  with pytest.raises(ValueError):
    env.run_episodes(lambda ts, active: a, episodes_per_env=0)
  env.step(a, active=np.ones(n, bool))          # (and a good one still steps)
  env.close()


def _policy_action(i, k):
  """The policy of the run_episodes tests: a pure function of the environment and its own count of active steps."""
  return np.random.default_rng([i, k]).uniform(0., 1., size=4)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('E', [1, 2])
def test_run_episodes(monkeypatch, backend, E):
  from oracle import oracle
  n = 7 if backend == 'emu' else 33
  env = _environment(monkeypatch, backend, n)
  ora = oracle.Engine(env._cfg, env.engine.pool)
  taken = np.zeros(n, np.int64)

  def policy(ts, active):
    assert ts.step_type.shape == (n,) and active.dtype == torch.bool
    act = active.cpu().numpy()
    a = np.full((n, 4), np.nan)
    for i in np.flatnonzero(act):
      a[i] = _policy_action(i, taken[i])
    taken[act] += 1
    return a

  stats = env.run_episodes(policy, episodes_per_env=E)
  ret, length, episodes, success = (v.cpu().numpy() for v in stats)
  assert stats.episode_return.dtype == torch.float64
  st = env.state()
  assert (st['episode'] == E).all() and (st['reset_next'] == 1).all()
  assert (episodes == E).all()
  # every environment alone on the oracle until its E-th LAST
  a = np.zeros((n, 4))
  for i in range(n):
    out = ora.step(a, render=False, env_range=(i, i + 1))
    assert out['step_type'][i] == _abi.STEP_FIRST
    total, steps, ends, k, ok = 0.0, 0, 0, 0, 0
    while ends < E:
      a[i] = _policy_action(i, k)
      k += 1
      out = ora.step(a, render=False, env_range=(i, i + 1))
      if out['step_type'][i] != _abi.STEP_FIRST:
        total += float(out['reward'][i])
        steps += 1
      if out['step_type'][i] == _abi.STEP_LAST:
        ends += 1
        ok = int(out['success'][i])
    assert _parity.bits(ret[i:i + 1]) == _parity.bits(np.array([total])), (i, ret[i], total)
    assert (int(length[i]), bool(success[i]), int(taken[i])) == (steps, bool(ok), k), i
  # (no environment ran on after its last episode: the episodes ended at different steps)
  assert len(set(length.tolist())) > 1
  env.close()
