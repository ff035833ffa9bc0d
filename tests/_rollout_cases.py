"""Scenarios of swb_rollout (candidate action sequences scored without stepping the batch), written against an engine factory so
that the emulated suite (tests/test_emulated_rollout.py) and the GPU suite (tests/test_gpu_rollout.py) run the same checks.

The reference value for candidate m is a fresh oracle.Engine on the same cfg and pool, replayed through the live steps taken so
far and then stepped K times (render=False) with actions[:, :, m]: rewards, discounts and positions bit-exact, step types,
success flags and sprite counts equal -- the bar of tests/_many_sprites_cases.py.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from spriteworld_amd import _abi
from spriteworld_amd import workloads
from tests import _parity

N_ENVS, M, T0, K, MAX_LEN = 16, 3, 3, 6, 4
PARITY = ('goal_s5', 'cluster_s5', 'sorting_s4', 'embodied_s12', 'f64_drag', 'cluster_s5_f32a', 'pos:goal_x_lt_half', 'ragged_s64')
_bits = _parity.bits


def built(name, n_envs=N_ENVS, seed=0, max_len=MAX_LEN, episodes_per_env=2):
  """(cfg, pool, sample) of a workload with episodes of at most `max_len` steps; 'pos:<case>' is a case of
  tests/_position_cases.py (a task whose filter keys on position), anything else a name of workloads.build."""
  if name.startswith('pos:'):
    from spriteworld_amd import lowering
    from tests import _position_cases as pc
    ns = pc.namespace_of_mirrors()
    task, aspace, rends, keep, _ = pc.environment_parts(ns, name[4:])
    episodes = pc.episodes_of(ns, name[4:], True, n_episodes=episodes_per_env * n_envs, seed=seed)
    cfg = lowering.lower_config(task, aspace, rends, keep, max_len, n_envs, pc.N_SPRITES, pos_is_f32=True)
    pool = lowering.lower_episodes(episodes, task, rends, max_sprites=pc.N_SPRITES).assign_round_robin(n_envs, episodes_per_env)
    assert pool.cell_label is not None
    return cfg, pool, lambda r: r.uniform(0.0, 1.0, size=(n_envs, 4))
  cfg, pool, sample = workloads.build(name, n_envs, episodes_per_env=episodes_per_env, seed=seed, anti_aliasing=2)
  cfg.max_episode_length = max_len
  return cfg, pool, sample


def candidates(cfg, sample, rng, st, n_cand, n_steps):
  """actions [K, N, M, A]; candidate 1's first click (SelectMove / DragAndDrop) lands on sprite 0 of its environment."""
  a = np.stack([np.stack([sample(rng) for _ in range(n_cand)], axis=1) for _ in range(n_steps)], axis=0)
  if cfg.action_space != _abi.ACTION_EMBODIED and n_cand > 1 and st is not None:
    a[0, :, 1, 0], a[0, :, 1, 1] = st['x'][:, 0], st['y'][:, 0]
  return np.ascontiguousarray(a)


def rollout(eng, actions, positions=True):
  """swb_rollout through the engine under test -> dict of numpy arrays in the C layout: Engine.rollout on the device; on the
  emulated library (its buffers are host memory) through the handle, into outputs filled with garbage first."""
  if eng.device.type != 'cpu':
    return {k: v.cpu().numpy() for k, v in eng.rollout(actions, positions=positions).items()}
  return rollout_through_library(eng, actions, positions)


def rollout_through_library(eng, actions, positions=True):
  """swb_rollout on the handle of an emulated engine: numpy arrays in, numpy arrays (filled with garbage first) out."""
  n_steps, n, n_cand, _ = actions.shape
  if eng.cfg.action_space == _abi.ACTION_EMBODIED:
    a = np.ascontiguousarray(actions, dtype=np.int32)
  else:
    a = np.ascontiguousarray(actions, dtype=np.float32 if eng.cfg.action_is_f32 else np.float64)
  res = {'reward': np.full((n_steps, n, n_cand), -7.0), 'discount': np.full((n_steps, n, n_cand), -7.0, np.float32),
         'step_type': np.full((n_steps, n, n_cand), 9, np.uint8), 'success': np.full((n_steps, n, n_cand), 9, np.uint8),
         'error': np.zeros((n, n_cand), np.uint8)}
  if positions:
    res.update(x=np.full((n, n_cand, eng.S), -7.0), y=np.full((n, n_cand, eng.S), -7.0), n_sprites=np.full((n, n_cand), -7, np.int32))
  rc, msg = raw_call(eng, a, n_cand, n_steps, res)
  if rc != 0:
    raise RuntimeError('swb error %d: %s' % (rc, msg))
  return res


def raw_call(eng, actions, n_cand, n_steps, res=None):
  """(status, message) of swb_rollout called on the engine's handle as given: `actions` a numpy array, a device tensor or
  None (NULL), `res` a dict of numpy arrays / tensors for the output struct."""
  lib = eng.lib
  addr = lambda t: None if t is None else (t.data_ptr() if hasattr(t, 'data_ptr') else t.ctypes.data)
  o = _abi.SwbRolloutOutputs()
  for k, t in (res or {}).items():
    setattr(o, k, addr(t))
  rc = lib.swb_rollout(eng._h, addr(actions), int(n_cand), int(n_steps), C.byref(o), eng._stream())
  return rc, lib.swb_last_error().decode() if rc else ''


def reference(cfg, pool, live, actions, reset_after_live=False):
  """The oracle's outputs for every candidate: dict of [K, N, M] arrays, error [N, M], x, y [N, M, S], n_sprites [N, M]."""
  from oracle import oracle
  n_steps, n, n_cand, _ = actions.shape
  want = {'reward': np.zeros((n_steps, n, n_cand)), 'discount': np.zeros((n_steps, n, n_cand), np.float32),
          'step_type': np.zeros((n_steps, n, n_cand), np.uint8), 'success': np.zeros((n_steps, n, n_cand), np.uint8),
          'error': np.zeros((n, n_cand), np.uint8), 'x': np.zeros((n, n_cand, cfg.max_sprites)),
          'y': np.zeros((n, n_cand, cfg.max_sprites)), 'n_sprites': np.zeros((n, n_cand), np.int32)}
  for m in range(n_cand):
    ora = oracle.Engine(cfg, pool)
    for a in live:
      ora.step(a, render=False)
    if reset_after_live:
      ora.reset_all()
    for k in range(n_steps):
      out = ora.step(actions[k, :, m], render=False)
      for key in ('reward', 'discount', 'step_type', 'success'):
        want[key][k, :, m] = out[key]
      want['error'][:, m] |= out['error']
    st = ora.state()
    want['x'][:, m], want['y'][:, m], want['n_sprites'][:, m] = st['x'], st['y'], st['n_sprites']
  return want


def assert_equal(got, want, what=''):
  np.testing.assert_array_equal(got['step_type'], want['step_type'], err_msg='step_type ' + what)
  np.testing.assert_array_equal(got['success'], want['success'], err_msg='success ' + what)
  np.testing.assert_array_equal(got['discount'].view(np.uint32), want['discount'].view(np.uint32), err_msg='discount ' + what)
  _parity.assert_rewards_equal(got['reward'], want['reward'], what)
  np.testing.assert_array_equal(got['error'], want['error'], err_msg='error ' + what)
  if 'x' in got:
    np.testing.assert_array_equal(_bits(got['x']), _bits(want['x']), err_msg='x ' + what)
    np.testing.assert_array_equal(_bits(got['y']), _bits(want['y']), err_msg='y ' + what)
    np.testing.assert_array_equal(got['n_sprites'], want['n_sprites'], err_msg='n_sprites ' + what)


def started(make_engine, name, t0=T0, seed=0, n_envs=N_ENVS, **kw):
  """(cfg, pool, sample, engine, the live actions it has taken, rng): the engine `t0` live steps into workload `name`."""
  cfg, pool, sample = built(name, n_envs=n_envs, seed=seed, **kw)
  eng = make_engine(cfg, pool)
  rng = np.random.default_rng(seed + 100)
  live = [sample(rng) for _ in range(t0)]
  for a in live:
    eng.step(a, render=False)
  return cfg, pool, sample, eng, live, rng


def _same_state(a, b):
  for k in ('x', 'y'):
    np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)
  for k in ('n_sprites', 'pool_entry', 'step_count', 'reset_next', 'episode'):
    np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---------------------------------------------------------------------------------------------------------------------
def parity_case(make_engine, name, seed=0):
  """1. t0 = 3 live steps, then K = 6 with episodes of at most 4 steps: every candidate ends an episode (LAST), restarts from
  the pool (FIRST) and plays on, inside the rollout."""
  cfg, pool, sample, eng, live, rng = started(make_engine, name, seed=seed)
  assert eng.variant()['many_sprites'] == int(cfg.max_sprites > _abi.SWB_TUNED_SPRITES)
  before = eng.state()
  acts = candidates(cfg, sample, rng, before, M, K)
  want = reference(cfg, pool, live, acts)
  # coverage: the auto-reset happens inside the rollout, and some candidates differ
  assert (want['step_type'][1:] == _abi.STEP_LAST).any() and (want['step_type'][1:] == _abi.STEP_FIRST).any(), name
  assert (_bits(want['x'][:, 0]) != _bits(want['x'][:, 1])).any() or cfg.action_space == _abi.ACTION_EMBODIED, name
  got = rollout(eng, acts)
  assert_equal(got, want, name)
  _same_state(eng.state(), before)
  eng.close()


def live_state_case(make_engine, name='goal_s5'):
  """2. The handle is as it was: state() bit-equal, the engine's sticky error buffer unchanged, and the next K real steps equal
  the oracle's (frames +-0) and candidate 0, which carries the same actions."""
  from oracle import oracle
  cfg, pool, sample, eng, live, rng = started(make_engine, name)
  ora = oracle.Engine(cfg, pool)
  for a in live:
    ora.step(a, render=False)
  acts = candidates(cfg, sample, rng, eng.state(), M, K)
  marks = (np.arange(cfg.n_envs) % 3 == 0).astype(np.uint8) * 0x40        # a caller's unread flags (no bit the engine sets)
  _set_error(eng, marks)
  before = eng.state()
  got = rollout(eng, acts)
  _same_state(eng.state(), before)
  np.testing.assert_array_equal(eng.outputs_host()['error'], marks)
  _set_error(eng, np.zeros_like(marks))
  for k in range(K):
    a = acts[k, :, 0]
    want = ora.step(a)
    eng.step(a)
    out = eng.outputs_host()
    _parity.compare(k, ora, eng, want, out)
    np.testing.assert_array_equal(out['step_type'], got['step_type'][k, :, 0])
    np.testing.assert_array_equal(out['success'], got['success'][k, :, 0])
    np.testing.assert_array_equal(out['discount'].view(np.uint32), got['discount'][k, :, 0].view(np.uint32))
    np.testing.assert_array_equal(_bits(out['reward']), _bits(got['reward'][k, :, 0]))
  st = eng.state()
  np.testing.assert_array_equal(_bits(st['x']), _bits(got['x'][:, 0]))
  np.testing.assert_array_equal(_bits(st['y']), _bits(got['y'][:, 0]))
  np.testing.assert_array_equal(st['n_sprites'], got['n_sprites'][:, 0])
  eng.close()


def _set_error(eng, values):
  import torch
  eng.error.copy_(torch.as_tensor(values))


EDGES = ('one_step', 'sixty_four_candidates', 'forty_steps', 'after_reset_all', 'scratch_grows')


def edge_case(make_engine, which, name='goal_s5'):
  """3. The corners of (M, K) and of the state a rollout starts from."""
  cfg, pool, sample, eng, live, rng = started(make_engine, name)
  st = eng.state()
  if which == 'one_step':                       # M = 1, K = 1: one step
    acts = candidates(cfg, sample, rng, st, 1, 1)
    assert_equal(rollout(eng, acts), reference(cfg, pool, live, acts), which)
  elif which == 'sixty_four_candidates':        # M = 64, K = 1
    acts = candidates(cfg, sample, rng, st, 64, 1)
    assert_equal(rollout(eng, acts), reference(cfg, pool, live, acts), which)
  elif which == 'forty_steps':                  # K = 40: eight episodes of five steps over a pool of two per environment
    assert (pool.pool_len == 2).all()
    acts = candidates(cfg, sample, rng, st, M, 40)
    want = reference(cfg, pool, live, acts)
    assert ((want['step_type'] == _abi.STEP_FIRST).sum(axis=0) >= 2 * 2 + 1).all(), 'episode mod pool_len does not wrap'
    assert_equal(rollout(eng, acts), want, which)
  elif which == 'after_reset_all':              # every k = 0 is FIRST
    eng.reset_all()
    acts = candidates(cfg, sample, rng, st, M, K)
    want = reference(cfg, pool, live, acts, reset_after_live=True)
    assert (want['step_type'][0] == _abi.STEP_FIRST).all()
    assert_equal(rollout(eng, acts), want, which)
  elif which == 'scratch_grows':                # two rollouts back to back, the second with more candidates
    small, large = candidates(cfg, sample, rng, st, 2, K), candidates(cfg, sample, rng, st, 5, K)
    got_small, got_large = rollout(eng, small), rollout(eng, large)
    assert_equal(got_small, reference(cfg, pool, live, small), which + ' M=2')
    assert_equal(got_large, reference(cfg, pool, live, large), which + ' M=5')
    assert_equal(rollout(eng, small), got_small, which + ' M=2 again')
  else:
    raise ValueError(which)
  _same_state(eng.state(), st if which != 'after_reset_all' else dict(st, reset_next=np.ones_like(st['reset_next'])))
  eng.close()


def refusals_case(make_engine, name='goal_s5'):
  """4. K = 0, M = 0 and NULL actions: SWB_ERR_INVALID; after a sprite setter: SWB_ERR_STATE; each with a message."""
  cfg, pool, sample, eng, live, rng = started(make_engine, name)
  acts = candidates(cfg, sample, rng, None, M, K)
  import torch
  dev = torch.as_tensor(acts, device=eng.device)      # (a device buffer for the real engine)
  for n_cand, n_steps, a, what in ((M, 0, dev, 'M and K must be positive'), (0, K, dev, 'M and K must be positive'),
                                   (M, -1, dev, 'M and K must be positive'), (M, K, None, 'actions is NULL')):
    rc, msg = raw_call(eng, a, n_cand, n_steps)
    assert rc == -1 and what in msg, (n_cand, n_steps, rc, msg)
  rc, msg = raw_call(eng, dev, M, K)            # (accepted with every output NULL)
  assert rc == 0, msg
  env = int(np.flatnonzero(eng.state()['reset_next'] == 0)[0])
  eng.set_sprite_attr(env, 0, _abi.ATTR_ANGLE, 45.0)
  rc, msg = raw_call(eng, dev, M, K)
  assert rc == -4 and 'sprite setters' in msg and 'not supported' in msg, (rc, msg)
  eng.close()


def episode_return_numpy(step_type, reward):
  """[N, M] from [N, M, K] arrays: rewards from step 0 through the first LAST, FIRST steps left out."""
  n, n_cand, n_steps = step_type.shape
  out = np.zeros((n, n_cand))
  for i in range(n):
    for m in range(n_cand):
      for k in range(n_steps):
        if step_type[i, m, k] != _abi.STEP_FIRST:
          out[i, m] += reward[i, m, k]
        if step_type[i, m, k] == _abi.STEP_LAST:
          break
  return out


def surface_case(n_envs=N_ENVS):
  """5. BatchedEnvironment.rollout ([N, M, K, A] in, [N, M, K] views out) against Engine.rollout and the oracle -- with a
  SelectMove noise_scale, which a rollout does not apply -- and Rollout.episode_return() against a numpy loop.  The engine
  class is environment._engine.Engine: the caller has patched the emulated one in, or runs on the GPU."""
  import torch
  from spriteworld_amd import action_spaces, environment, renderers, sprite_generators, tasks
  from spriteworld_amd import factor_distributions as distribs
  common = [distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9),
            distribs.Discrete('shape', ['square', 'triangle', 'circle']), distribs.Discrete('scale', [0.2]),
            distribs.Continuous('c1', 0.3, 1.), distribs.Continuous('c2', 0.9, 1.)]
  gen = sprite_generators.chain_generators(
      sprite_generators.generate_sprites(distribs.Product(common + [distribs.Continuous('c0', 0., 0.4)]), num_sprites=2),
      sprite_generators.generate_sprites(distribs.Product(common + [distribs.Continuous('c0', 0.5, 0.9)]), num_sprites=2))
  task = tasks.FindGoalPosition(filter_distrib=distribs.Continuous('c0', 0., 0.4), terminate_distance=0.2)
  rend = {'image': renderers.PILRenderer(image_size=(16, 16), anti_aliasing=1, color_to_rgb=renderers.color_maps.hsv_to_rgb)}
  env = environment.BatchedEnvironment(task=task, action_space=action_spaces.SelectMove(scale=0.25, noise_scale=0.1), renderers=rend,
                                       init_sprites=gen, max_episode_length=MAX_LEN, num_envs=n_envs, episodes_per_env=2,
                                       refresh_every=0, seed=5)
  env.seed_noise(1)
  env.reset()
  cfg, pool = env.engine.cfg, env.engine.get_pool()
  rng = np.random.default_rng(8)
  a = rng.uniform(0.0, 1.0, size=(n_envs, M, K, 4))                       # the planner's layout
  st = env.state()
  a[:, 1, 0, 0], a[:, 1, 0, 1] = st['x'][:, 0], st['y'][:, 0]
  r = env.rollout(torch.as_tensor(a))
  assert isinstance(r, environment.Rollout)
  for f in ('step_type', 'reward', 'discount', 'success'):
    assert tuple(getattr(r, f).shape) == (n_envs, M, K), f
  assert tuple(r.x.shape) == tuple(r.y.shape) == (n_envs, M, cfg.max_sprites) and tuple(r.n_sprites.shape) == tuple(r.error.shape) == (n_envs, M)
  assert (r.step_type.dtype, r.reward.dtype, r.discount.dtype, r.success.dtype) == (torch.uint8, torch.float64, torch.float32, torch.uint8)
  kn = np.ascontiguousarray(a.transpose(2, 0, 1, 3))                      # [K, N, M, A]
  direct = env.engine.rollout(kn, positions=True)
  got = {f: getattr(r, f).cpu().numpy() for f in r._fields}
  for f in ('step_type', 'reward', 'discount', 'success'):
    assert tuple(direct[f].shape) == (K, n_envs, M)
    np.testing.assert_array_equal(got[f], direct[f].cpu().numpy().transpose(1, 2, 0), err_msg=f)
    got[f] = got[f].transpose(2, 0, 1)
  for f in ('x', 'y', 'n_sprites', 'error'):
    np.testing.assert_array_equal(got[f], direct[f].cpu().numpy(), err_msg=f)
  # the noiseless dynamics: the oracle stepping the candidates exactly as given (reset() was one live step: FIRST, its action unused)
  want = reference(cfg, pool, [np.zeros((n_envs, 4))], kn)
  assert_equal(got, want, 'BatchedEnvironment.rollout')
  assert (want['step_type'] == _abi.STEP_LAST).any() and (_bits(want['x'][:, 0]) != _bits(want['x'][:, 1])).any()
  # episode_return(): float64 sums of at most K terms in whatever order torch takes -- off the loop's by at most K roundings
  ret = r.episode_return()
  assert tuple(ret.shape) == (n_envs, M) and ret.dtype == torch.float64
  loop = episode_return_numpy(want['step_type'].transpose(1, 2, 0), want['reward'].transpose(1, 2, 0))
  bound = K * 2.0 ** -52 * np.nansum(np.abs(want['reward']), axis=0) + 1e-300
  assert (np.abs(ret.cpu().numpy() - loop) <= bound).all()
  ends = (want['step_type'] == _abi.STEP_LAST).any(axis=0)
  assert ends.any() and (np.abs(loop[ends] - np.nansum(want['reward'], axis=0)[ends]) > 0).any(), 'no candidate is cut at its LAST'
  env.close()
