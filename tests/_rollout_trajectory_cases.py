"""Scenarios of swb_rollout_trajectory (a rollout that keeps the state after every step) and swb_rollout_step_frames (the frames
of those states), written against an engine factory so that the emulated suite (tests/test_emulated_rollout_trajectory.py) and
the GPU suite (tests/test_gpu_rollout_trajectory.py) run the same checks.  Sizes are those of tests/_rollout_cases.py: N = 16,
M = 3, K = 6 after T0 = 3 live steps with episodes of at most 4 steps, so that every rollout crosses a LAST and a FIRST.

The expected values for candidate m are a fresh oracle.Engine on the same cfg and pool, replayed through the live steps taken so
far and then stepped K times with actions[:, :, m], EVERY step rendered and its state() read: positions and rewards bit for bit,
frames +-0.  One replay serves every test of a process that asks for the same actions (`reference_steps` keeps them).  Output
buffers are filled with garbage first (0x5A / -7), so that a word never written shows.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import hashlib

import numpy as np
import torch

from spriteworld_amd import _abi
from tests import _parity
from tests._rollout_cases import (K, M, MAX_LEN, N_ENVS, PARITY, assert_equal, candidates, raw_call, reference, rollout,
                                  started)
from tests._rollout_frames_cases import (ERR_INVALID, ERR_STATE, ROUTES, _same_state, _violations, assert_frames_equal, frames,
                                         raw_frames, start)

_bits = _parity.bits
ALL = _abi.SWB_ALL_STEPS
PER_STEP = ('reward', 'discount', 'step_type', 'success')


def _ptr(t):
  return None if t is None else C.c_void_p(t.data_ptr())


def _actions_for(eng, actions):
  if eng.cfg.action_space == _abi.ACTION_EMBODIED:
    a = np.ascontiguousarray(actions, dtype=np.int32)
  else:
    a = np.ascontiguousarray(actions, dtype=np.float32 if eng.cfg.action_is_f32 else np.float64)
  return torch.as_tensor(a, device=eng.device)


def raw_trajectory(eng, actions, n_cand=None, n_steps=None, out=True, steps=True):
  """(status, message, outputs, per-step outputs) of swb_rollout_trajectory called on the engine's handle as given: `actions`
  [K, N, M, A] (numpy) or None (NULL); `out` / `steps` False pass NULL structs.  The buffers are tensors on the engine's device
  filled with garbage first (error: zeros, it is ORed into)."""
  if actions is not None:
    n_steps = actions.shape[0] if n_steps is None else n_steps
    n_cand = actions.shape[2] if n_cand is None else n_cand
  n, s = eng.N, eng.S
  kk, mm = max(n_steps, 1), max(n_cand, 1)
  full = lambda shape, value, dtype: torch.full(shape, value, dtype=dtype, device=eng.device)
  res = {'reward': full((kk, n, mm), -7.0, torch.float64), 'discount': full((kk, n, mm), -7.0, torch.float32),
         'step_type': full((kk, n, mm), 9, torch.uint8), 'success': full((kk, n, mm), 9, torch.uint8),
         'error': full((n, mm), 0, torch.uint8), 'x': full((n, mm, s), -7.0, torch.float64), 'y': full((n, mm, s), -7.0, torch.float64),
         'n_sprites': full((n, mm), -7, torch.int32)}
  per = {'x': full((kk, n, mm, s), -7.0, torch.float64), 'y': full((kk, n, mm, s), -7.0, torch.float64),
         'n_sprites': full((kk, n, mm), -7, torch.int32)}
  o, so = _abi.SwbRolloutOutputs(), _abi.SwbRolloutStepOutputs()
  for k, t in res.items():
    setattr(o, k, t.data_ptr())
  for k, t in per.items():
    setattr(so, k, t.data_ptr())
  a = None if actions is None else (actions if isinstance(actions, torch.Tensor) else _actions_for(eng, actions))
  rc = eng.lib.swb_rollout_trajectory(eng._h, _ptr(a), int(n_cand), int(n_steps), C.byref(o) if out else None,
                                      C.byref(so) if steps else None, eng._stream())
  eng._sync()
  return rc, (eng.lib.swb_last_error().decode() if rc else ''), res, per


def trajectory(eng, actions):
  """swb_rollout_trajectory through the handle -> (outputs, per-step outputs) as dicts of numpy arrays in the C layout."""
  rc, msg, res, per = raw_trajectory(eng, actions)
  assert rc == 0, msg
  return {k: v.cpu().numpy() for k, v in res.items()}, {k: v.cpu().numpy() for k, v in per.items()}


def raw_step_frames(eng, n_cand, step, cand=None, obs='new', error='new', n_steps=K):
  """(status, message, obs, error) of swb_rollout_step_frames called on the engine's handle as given: `cand` None or int values
  per environment; `obs` / `error`: 'new' (a buffer of the documented shape, filled with 0x5A / zeros), a tensor, or None."""
  lead = (eng.N,) if cand is not None else (eng.N, max(n_cand, 1))
  if step == ALL:
    lead = (n_steps,) + lead
  if isinstance(obs, str):
    obs = torch.full(lead + tuple(eng.obs_shape), 0x5A, dtype=torch.uint8, device=eng.device)
  if isinstance(error, str):
    error = torch.zeros(lead, dtype=torch.uint8, device=eng.device)
  c = None if cand is None else torch.as_tensor(np.asarray(cand, dtype=np.int32), device=eng.device)
  rc = eng.lib.swb_rollout_step_frames(eng._h, int(n_cand), int(step), _ptr(c), _ptr(obs), _ptr(error), eng._stream())
  eng._sync()
  return rc, (eng.lib.swb_last_error().decode() if rc else ''), obs, error


def step_frames(eng, n_cand, step, cand=None, n_steps=K):
  """The frames (numpy) of `step` of the last trajectory rollout; no error flag, no violation of the run lists."""
  rc, msg, obs, error = raw_step_frames(eng, n_cand, step, cand, n_steps=n_steps)
  assert rc == 0, msg
  assert not error.cpu().numpy().any(), 'error flags'
  assert _violations(eng) == 0
  return obs.cpu().numpy()


_REFERENCES = {}


def reference_steps(cfg, pool, live, actions, reset_after_live=False, render=True):
  """The oracle's (outputs as tests/_rollout_cases.reference returns them, per-step states {x, y [K, N, M, S], n_sprites
  [K, N, M]}, frames [K, N, M, H, W, 3] or None) for every candidate, every step rendered.  Kept per process, keyed on the
  configuration, the pool, the live steps and the actions; the arrays handed out are read-only."""
  from oracle import oracle
  h = hashlib.sha256()
  for part in [bytes(cfg), pool.x.tobytes(), pool.y.tobytes(), pool.shape.tobytes(), pool.rgb.tobytes(), pool.pool_base.tobytes(),
               actions.tobytes(), repr((actions.shape, bool(reset_after_live), bool(render))).encode()] + [np.asarray(a).tobytes() for a in live]:
    h.update(part)
  key = h.hexdigest()
  if key in _REFERENCES:
    return _REFERENCES[key]
  n_steps, n, n_cand, _ = actions.shape
  s = cfg.max_sprites
  want = {'reward': np.zeros((n_steps, n, n_cand)), 'discount': np.zeros((n_steps, n, n_cand), np.float32),
          'step_type': np.zeros((n_steps, n, n_cand), np.uint8), 'success': np.zeros((n_steps, n, n_cand), np.uint8),
          'error': np.zeros((n, n_cand), np.uint8), 'x': np.zeros((n, n_cand, s)), 'y': np.zeros((n, n_cand, s)),
          'n_sprites': np.zeros((n, n_cand), np.int32)}
  per = {'x': np.zeros((n_steps, n, n_cand, s)), 'y': np.zeros((n_steps, n, n_cand, s)), 'n_sprites': np.zeros((n_steps, n, n_cand), np.int32)}
  obs = None
  for m in range(n_cand):
    ora = oracle.Engine(cfg, pool)
    for a in live:
      ora.step(a, render=False)
    if reset_after_live:
      ora.reset_all()
    for k in range(n_steps):
      out = ora.step(actions[k, :, m], render=render)
      for f in PER_STEP:
        want[f][k, :, m] = out[f]
      want['error'][:, m] |= out['error']
      st = ora.state()
      per['x'][k, :, m], per['y'][k, :, m], per['n_sprites'][k, :, m] = st['x'], st['y'], st['n_sprites']
      if render:
        if obs is None:
          obs = np.zeros((n_steps, n, n_cand) + out['obs'].shape[1:], np.uint8)
        obs[k, :, m] = out['obs']
    want['x'][:, m], want['y'][:, m], want['n_sprites'][:, m] = per['x'][-1, :, m], per['y'][-1, :, m], per['n_sprites'][-1, :, m]
  for a in list(want.values()) + list(per.values()) + ([obs] if obs is not None else []):
    a.setflags(write=False)
  _REFERENCES[key] = (want, per, obs)
  return _REFERENCES[key]


def assert_steps_equal(got, want, what=''):
  np.testing.assert_array_equal(_bits(got['x']), _bits(want['x']), err_msg='x per step ' + what)
  np.testing.assert_array_equal(_bits(got['y']), _bits(want['y']), err_msg='y per step ' + what)
  np.testing.assert_array_equal(got['n_sprites'], want['n_sprites'], err_msg='n_sprites per step ' + what)


def _crosses_an_episode(step_type, what):
  assert (step_type[1:] == _abi.STEP_LAST).any() and (step_type[1:] == _abi.STEP_FIRST).any(), what


# ---------------------------------------------------------------------------------------------------------------------
# 1. and 2. scores unchanged, per-step states
def parity_case(make_engine, name, seed=0):
  """The swb_rollout_outputs of swb_rollout_trajectory equal the oracle's and those of swb_rollout on a twin engine; x, y,
  n_sprites [k] equal the oracle's state() after every step and the end state a plain swb_rollout of K' = k + 1 steps returns
  on the twin, for every k."""
  cfg, pool, sample, eng, live, rng = started(make_engine, name, seed=seed)
  before = eng.state()
  acts = candidates(cfg, sample, rng, before, M, K)
  want, want_steps, _ = reference_steps(cfg, pool, live, acts, render=False)
  _crosses_an_episode(want['step_type'], name)
  assert_equal(want, reference(cfg, pool, live, acts), name + ': the two oracle replays')
  got, got_steps = trajectory(eng, acts)
  assert_equal(got, want, name)
  assert_steps_equal(got_steps, want_steps, name)
  for f in ('x', 'y', 'n_sprites'):       # the last slot is the end state
    np.testing.assert_array_equal(_bits(got_steps[f][-1]) if f != 'n_sprites' else got_steps[f][-1],
                                  _bits(got[f]) if f != 'n_sprites' else got[f], err_msg=f)
  assert (_bits(got_steps['x'][0]) != _bits(got_steps['x'][-1])).any(), 'every step holds the same state'
  _same_state(eng.state(), before)
  twin = make_engine(cfg, pool)
  for a in live:
    twin.step(a, render=False)
  for k in range(K):
    plain = rollout(twin, np.ascontiguousarray(acts[:k + 1]))
    for f in ('x', 'y'):
      np.testing.assert_array_equal(_bits(got_steps[f][k]), _bits(plain[f]), err_msg='%s after step %d against swb_rollout K = %d' % (f, k + 1, k + 1))
    np.testing.assert_array_equal(got_steps['n_sprites'][k], plain['n_sprites'], err_msg='n_sprites, step %d' % (k + 1))
  assert_equal(got, plain, name + ': swb_rollout on a twin engine')
  # NULL per-step outputs, and NULL outputs: accepted, the scores the same
  rc, msg, res, per = raw_trajectory(eng, acts, steps=False)
  assert rc == 0, msg
  assert_equal({k: v.cpu().numpy() for k, v in res.items()}, want, name + ': steps NULL')
  assert (per['n_sprites'].cpu().numpy() == -7).all()
  rc, msg, _, _ = raw_trajectory(eng, acts, out=False, steps=False)
  assert rc == 0, msg
  twin.close()
  eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. per-step frames, every render route
def route_case(make_engine, monkeypatch, route):
  """For every k, swb_rollout_step_frames(step = k) of all candidates equals the oracle stepping with render=True, on the render
  route the handle takes; step = K - 1 equals swb_rollout_frames; no error flags, no violation of the run lists."""
  name, aa, switches, expect = ROUTES[route]
  for k, v in switches.items():
    monkeypatch.setenv(k, v)
  cfg, pool, sample, eng, live, rng = start(make_engine, name, aa=aa)
  v = eng.variant()
  for k, value in expect.items():
    assert v[k] == value, (route, k, v)
  acts = candidates(cfg, sample, rng, eng.state(), M, K)
  want, _, want_obs = reference_steps(cfg, pool, live, acts)
  _crosses_an_episode(want['step_type'], route)
  got, _ = trajectory(eng, acts)
  np.testing.assert_array_equal(got['step_type'], want['step_type'])
  for k in range(K):
    assert_frames_equal(step_frames(eng, M, k), want_obs[k], '%s step %d' % (route, k))
  assert_frames_equal(frames(eng, M), want_obs[K - 1], route + ': swb_rollout_frames after a trajectory rollout')
  # a step that was LAST shows the terminal sprites, one that was FIRST the fresh episode: both are among the frames compared
  assert any((want_obs[k, n, 0] != want_obs[k, n, m]).any() for k in range(K) for n in range(cfg.n_envs) for m in range(1, M)), route
  eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. picked candidates
def picked_case(make_engine, name='goal_s5'):
  """A single step with cand[N], values below 0 and at or above M clamped; SWB_ALL_STEPS with cand equals the matching slices
  of the all-candidates frames of every step; error [N] / [K, N] is ORed into."""
  cfg, pool, sample, eng, live, rng = start(make_engine, name)
  acts = candidates(cfg, sample, rng, eng.state(), M, K)
  _, _, want_obs = reference_steps(cfg, pool, live, acts)
  trajectory(eng, acts)
  every = np.stack([step_frames(eng, M, k) for k in range(K)])
  assert_frames_equal(every, want_obs, 'all candidates, every step')
  n = np.arange(cfg.n_envs)
  mixed = (n * 2 + 1) % M
  assert set(mixed) == set(range(M))
  wild = np.where(n % 2 == 0, -3, M + 2)
  clamped = np.where(n % 2 == 0, 0, M - 1)
  for k in (0, 2, K - 1):
    assert_frames_equal(step_frames(eng, M, k, mixed), every[k][n, mixed], 'mixed, step %d' % k)
    assert_frames_equal(step_frames(eng, M, k, wild), every[k][n, clamped], 'clamped, step %d' % k)
  assert_frames_equal(step_frames(eng, M, ALL, mixed), every[:, n, mixed], 'every step, mixed')
  assert_frames_equal(step_frames(eng, M, ALL, wild), every[:, n, clamped], 'every step, clamped')
  assert any((every[k, i, 0] != every[k, i, M - 1]).any() for k in range(K) for i in n)
  marks = torch.full((K, cfg.n_envs), 0x40, dtype=torch.uint8, device=eng.device)
  rc, msg, obs, error = raw_step_frames(eng, M, ALL, mixed, error=marks)
  assert rc == 0 and (error.cpu().numpy() == 0x40).all(), (rc, msg)            # ORed into: marks survive
  rc, msg, obs, error = raw_step_frames(eng, M, 1, mixed, error=None)          # (accepted without an error buffer)
  assert rc == 0, msg
  assert_frames_equal(obs.cpu().numpy(), every[1][n, mixed], 'without an error buffer')
  assert_frames_equal(step_frames(eng, M, 3), every[3], 'all candidates again, after the picks')
  assert_frames_equal(frames(eng, M, mixed), every[K - 1][n, mixed], 'swb_rollout_frames, picked')
  eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the handle is left as it was
def handle_case(make_engine, name='goal_s5'):
  """Live state bit-equal, a caller's marks in the sticky error buffer, the pool and the engine's own obs unchanged, no counted
  step of swb_timing_enable; the next K real steps equal the oracle, frames included, and candidate 0's frames, which carries
  the same actions."""
  from oracle import oracle
  cfg, pool, sample, eng, live, rng = start(make_engine, name, rendered=1)
  ora = oracle.Engine(cfg, pool)
  for a in live:
    ora.step(a, render=False)
  acts = candidates(cfg, sample, rng, eng.state(), M, K)
  marks = (np.arange(cfg.n_envs) % 3 == 0).astype(np.uint8) * 0x40        # a caller's unread flags (no bit the engine sets)
  eng.error.copy_(torch.as_tensor(marks))
  eng.timing(True)
  before, obs_before, launches, pool_before = eng.state(), eng.outputs_host()['obs'], eng.step_time_ms()[1], eng.get_pool()
  got, got_steps = trajectory(eng, acts)
  every = np.stack([step_frames(eng, M, k) for k in range(K)])
  picked = step_frames(eng, M, ALL, np.zeros(cfg.n_envs, np.int32))
  assert eng.step_time_ms()[1] == launches, 'a counted step of swb_timing_enable'
  _same_state(eng.state(), before)
  host = eng.outputs_host()
  np.testing.assert_array_equal(host['error'], marks)
  np.testing.assert_array_equal(host['obs'], obs_before)
  pool_after = eng.get_pool()
  for f in ('n_sprites', 'x', 'y', 'shape', 'rgb', 'label', 'pool_base', 'pool_len'):
    np.testing.assert_array_equal(getattr(pool_after, f), getattr(pool_before, f), err_msg='pool ' + f)
  eng.error.zero_()
  for k in range(K):
    a = acts[k, :, 0]
    want = ora.step(a)
    eng.step(a)
    out = eng.outputs_host()
    _parity.compare(k, ora, eng, want, out, what='after a trajectory rollout')
    assert_frames_equal(every[k][:, 0], out['obs'], 'candidate 0 against real step %d' % (k + 1))
    assert_frames_equal(picked[k], out['obs'], 'picked candidate 0 against real step %d' % (k + 1))
    st = eng.state()
    np.testing.assert_array_equal(_bits(st['x']), _bits(got_steps['x'][k][:, 0]))
    np.testing.assert_array_equal(_bits(st['y']), _bits(got_steps['y'][k][:, 0]))
    np.testing.assert_array_equal(st['n_sprites'], got_steps['n_sprites'][k][:, 0])
    _parity.assert_rewards_equal(out['reward'], got['reward'][k, :, 0], 'real step %d' % (k + 1))
  assert eng.step_time_ms()[1] == launches + K
  assert _violations(eng) == 0
  eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. edges
EDGES = ('one_candidate_one_step', 'trajectory_grows', 'after_reset_all', 'plain_rollout_afterwards')


def edge_case(make_engine, which, name='goal_s5'):
  cfg, pool, sample, eng, live, rng = start(make_engine, name)
  st = eng.state()

  def check(acts, reset=False):
    n_steps, n_cand = acts.shape[0], acts.shape[2]
    want, want_steps, want_obs = reference_steps(cfg, pool, live, acts, reset_after_live=reset)
    got, got_steps = trajectory(eng, acts)
    assert_equal(got, want, which)
    assert_steps_equal(got_steps, want_steps, which)
    for k in range(n_steps):
      assert_frames_equal(step_frames(eng, n_cand, k, n_steps=n_steps), want_obs[k], '%s K = %d M = %d step %d' % (which, n_steps, n_cand, k))
    pick = np.arange(cfg.n_envs) % n_cand
    assert_frames_equal(step_frames(eng, n_cand, ALL, pick, n_steps=n_steps), want_obs[:, np.arange(cfg.n_envs), pick], which + ' picked')
    return want, got

  if which == 'one_candidate_one_step':
    check(candidates(cfg, sample, rng, st, 1, 1))
  elif which == 'trajectory_grows':           # K = 2, then K = 6 (the block grows), then M = 5 (block and scratch grow), then K = 2 again
    small = candidates(cfg, sample, rng, st, M, 2)
    check(small)
    check(candidates(cfg, sample, rng, st, M, K))
    check(candidates(cfg, sample, rng, st, 5, K))
    check(small)
  elif which == 'after_reset_all':            # every k = 0 is FIRST: the frames of step 0 do not depend on the candidate
    eng.reset_all()
    acts = candidates(cfg, sample, rng, st, M, K)
    want, _ = check(acts, reset=True)
    assert (want['step_type'][0] == _abi.STEP_FIRST).all()
    first = step_frames(eng, M, 0)
    assert all((first[:, m] == first[:, 0]).all() for m in range(M))
    st = dict(st, reset_next=np.ones_like(st['reset_next']))
  elif which == 'plain_rollout_afterwards':   # a plain swb_rollout keeps no steps: it invalidates the trajectory
    acts = candidates(cfg, sample, rng, st, M, K)
    check(acts)
    plain = rollout(eng, acts)
    rc, msg, _, _ = raw_step_frames(eng, M, 0)
    assert rc == ERR_STATE and 'kept no steps' in msg and 'swb_rollout_trajectory' in msg, (rc, msg)
    assert_frames_equal(frames(eng, M), reference_steps(cfg, pool, live, acts)[2][K - 1], 'swb_rollout_frames still works')
    assert_equal(plain, reference_steps(cfg, pool, live, acts)[0], which)
    check(acts)
  else:
    raise ValueError(which)
  _same_state(eng.state(), st)
  eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. refusals
def refusals_case(make_engine, name='goal_s5'):
  """Every SWB_ERR_INVALID and SWB_ERR_STATE condition of the two calls, each with its message."""
  cfg, pool, sample, eng, live, rng = start(make_engine, name)
  rc, msg, _, _ = raw_step_frames(eng, M, 0)
  assert rc == ERR_STATE and 'no rollout has run' in msg, (rc, msg)
  for kw in ({'step': 0}, {'step': 'all', 'candidates': np.zeros(cfg.n_envs, np.int32)}):
    try:
      eng.rollout_frames(**kw)
      raise AssertionError('Engine.rollout_frames(%r) before any rollout did not raise' % (kw,))
    except AssertionError:
      raise
    except Exception as e:  # pylint: disable=broad-except
      assert 'no rollout has run' in str(e) and not isinstance(e, (ValueError, TypeError)), (type(e), e)
  acts = candidates(cfg, sample, rng, eng.state(), M, K)
  dev = _actions_for(eng, acts)
  # swb_rollout_trajectory: swb_rollout's refusals under its own name, and the product that does not fit an int
  for n_cand, n_steps, a, what in ((M, 0, dev, 'M and K must be positive'), (0, K, dev, 'M and K must be positive'),
                                   (M, -1, dev, 'M and K must be positive'), (M, K, None, 'actions is NULL'),
                                   (M, (1 << 16) + 1, dev, 'exceeds the limit of 65536 steps'),
                                   ((1 << 24) // cfg.n_envs + 1, K, dev, 'exceed the grid limit'),
                                   ((1 << 24) // cfg.n_envs, (1 << 31) // ((1 << 24) * cfg.max_sprites) + 1, dev, 'does not fit an int')):
    rc = eng.lib.swb_rollout_trajectory(eng._h, _ptr(a), n_cand, n_steps, None, None, eng._stream())
    msg = eng.lib.swb_last_error().decode()
    assert rc == ERR_INVALID and what in msg and 'swb_rollout_trajectory' in msg, (n_cand, n_steps, rc, msg)
  rc, msg, _, _ = raw_step_frames(eng, M, 0)       # (a refused rollout is none)
  assert rc == ERR_STATE and 'no rollout has run' in msg, (rc, msg)
  # after a plain rollout: it kept no steps
  rollout(eng, acts)
  rc, msg, _, _ = raw_step_frames(eng, M, 0)
  assert rc == ERR_STATE and 'plain swb_rollout, which kept no steps' in msg, (rc, msg)
  try:
    eng.rollout_frames(step=0)
    raise AssertionError('Engine.rollout_frames(step=0) after a plain rollout did not raise')
  except AssertionError:
    raise
  except Exception as e:  # pylint: disable=broad-except
    assert 'kept no steps' in str(e), e
  trajectory(eng, acts)
  for n_cand in (M + 1, M - 1):
    rc, msg, _, _ = raw_step_frames(eng, n_cand, 0)
    assert rc == ERR_INVALID and 'the last rollout of this handle had %d candidates' % M in msg, (rc, msg)
  rc, msg, _, _ = raw_step_frames(eng, M, 0, obs=None)
  assert rc == ERR_INVALID and 'obs is NULL' in msg, (rc, msg)
  for step in (K, K + 5, -2):
    rc, msg, _, _ = raw_step_frames(eng, M, step)
    assert rc == ERR_INVALID and 'step = %d is outside [0, %d)' % (step, K) in msg, (rc, msg)
  rc, msg, _, _ = raw_step_frames(eng, M, ALL)
  assert rc == ERR_INVALID and 'SWB_ALL_STEPS needs picked candidates' in msg, (rc, msg)
  try:
    eng.rollout_frames(step='all')
    raise AssertionError("Engine.rollout_frames(step='all') without candidates did not raise")
  except ValueError as e:
    assert "step='all' needs candidates" in str(e), e
  _, _, want_obs = reference_steps(cfg, pool, live, acts)
  assert_frames_equal(step_frames(eng, M, 2), want_obs[2], 'after the refused calls')
  eng.set_pool(pool)
  for step, cand in ((0, None), (ALL, np.zeros(cfg.n_envs, np.int32))):
    rc, msg, _, _ = raw_step_frames(eng, M, step, cand)
    assert rc == ERR_STATE and 'pool has changed' in msg and 'swb_set_pool' in msg, (rc, msg)
  for a in live:
    eng.step(a, render=False)
  trajectory(eng, acts)
  assert_frames_equal(step_frames(eng, M, 4), want_obs[4], 'after a new pool and a new rollout')
  env = int(np.flatnonzero(eng.state()['reset_next'] == 0)[0])
  eng.set_sprite_attr(env, 0, _abi.ATTR_ANGLE, 45.0)
  rc, msg, _, _ = raw_step_frames(eng, M, 0)
  assert rc == ERR_STATE and 'sprite setters' in msg and 'not supported' in msg, (rc, msg)
  rc, msg, _, _ = raw_trajectory(eng, acts)
  assert rc == ERR_STATE and 'swb_rollout_trajectory: sprite setters' in msg and 'not supported' in msg, (rc, msg)
  eng.close()


def refusals_after_device_sampling_case(case='hsv_mixed', n_envs=N_ENVS):
  """swb_sample_pool (refill_pool) and swb_resample_pool (refresh_pool) invalidate the trajectory: SWB_ERR_STATE until the next
  rollout.  A device-sampled workload of tests/_sampler_cases.py; the engine class is environment._engine.Engine: the caller has
  patched the emulated one in, or runs on the GPU."""
  from tests import _sampler_cases
  env, _, _, _ = _sampler_cases.make_env(case, num_envs=n_envs, episodes_per_env=2)
  eng = env.engine
  env.reset()
  acts = np.random.default_rng(3).uniform(0.0, 1.0, size=(n_envs, M, 2, 4))
  for redraw, call in ((env.refill_pool, 'swb_sample_pool'), (env.refresh_pool, 'swb_resample_pool')):
    env.rollout(acts, keep_steps=True)
    first = env.rollout_frames(step=0)
    assert tuple(first.shape) == (n_envs, M) + tuple(eng.obs_shape)
    redraw()
    rc, msg, _, _ = raw_step_frames(eng, M, 0)
    assert rc == ERR_STATE and 'pool has changed' in msg and call in msg, (call, rc, msg)
    try:
      env.rollout_frames(step=1)
      raise AssertionError('rollout_frames(step=1) after %s did not raise' % call)
    except AssertionError:
      raise
    except Exception as e:  # pylint: disable=broad-except
      assert 'pool has changed' in str(e), e
    env.reset()
  env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. the Python surface
def surface_case(n_envs=N_ENVS):
  """BatchedEnvironment.rollout(keep_steps=True), rollout_frames(step=...) and rollout_positions() on the environment of
  tests/_rollout_cases.surface_case, whose SelectMove action space is noisy (rollouts stay noiseless): shapes, layouts, values
  against the oracle and against Engine, and the documented raises.  The engine class is environment._engine.Engine: the caller
  has patched the emulated one in, or runs on the GPU."""
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
  eng = env.engine
  with_raises = lambda fn, exc, what: _raises(fn, exc, what)
  with_raises(env.rollout_positions, environment.EnvironmentError_, 'kept no steps')
  cfg, pool = eng.cfg, eng.get_pool()
  s = cfg.max_sprites
  a = np.random.default_rng(8).uniform(0.0, 1.0, size=(n_envs, M, K, 4))      # the planner's layout
  st = env.state()
  a[:, 1, 0, 0], a[:, 1, 0, 1] = st['x'][:, 0], st['y'][:, 0]
  plain = env.rollout(torch.as_tensor(a))
  with_raises(env.rollout_positions, environment.EnvironmentError_, 'kept no steps')
  with_raises(lambda: env.rollout_frames(step=0), Exception, 'kept no steps')
  r = env.rollout(torch.as_tensor(a), keep_steps=True)
  assert isinstance(r, environment.Rollout) and r._fields == plain._fields
  for f in r._fields:       # the same tuple, the same values (NaN rewards of FIRST steps: bits)
    g, p = getattr(r, f).cpu().numpy(), getattr(plain, f).cpu().numpy()
    assert g.shape == p.shape and g.dtype == p.dtype, f
    np.testing.assert_array_equal(_bits(g) if g.dtype == np.float64 else g, _bits(p) if p.dtype == np.float64 else p, err_msg=f)
  pos = env.rollout_positions()
  assert isinstance(pos, environment.RolloutSteps) and pos._fields == ('x', 'y', 'n_sprites')
  assert tuple(pos.x.shape) == tuple(pos.y.shape) == (n_envs, M, K, s) and tuple(pos.n_sprites.shape) == (n_envs, M, K)
  assert (pos.x.dtype, pos.y.dtype, pos.n_sprites.dtype) == (torch.float64, torch.float64, torch.int32) and pos.x.device == eng.device
  # against the oracle: reset() was one live step (FIRST, its action unused); the rollout is of the noiseless dynamics
  kn = np.ascontiguousarray(a.transpose(2, 0, 1, 3))
  want, want_steps, want_obs = reference_steps(cfg, pool, [np.zeros((n_envs, 4))], kn)
  assert (want['step_type'] == _abi.STEP_LAST).any()
  np.testing.assert_array_equal(_bits(pos.x.cpu().numpy()), _bits(want_steps['x'].transpose(1, 2, 0, 3)))
  np.testing.assert_array_equal(_bits(pos.y.cpu().numpy()), _bits(want_steps['y'].transpose(1, 2, 0, 3)))
  np.testing.assert_array_equal(pos.n_sprites.cpu().numpy(), want_steps['n_sprites'].transpose(1, 2, 0))
  assert torch.equal(pos.x[:, :, K - 1], r.x) and torch.equal(pos.n_sprites[:, :, K - 1], r.n_sprites)
  # frames
  end = env.rollout_frames()
  assert_frames_equal(end.cpu().numpy(), want_obs[K - 1], 'rollout_frames() after keep_steps')
  for k in (0, 3, K - 1):
    one = env.rollout_frames(step=k)
    assert tuple(one.shape) == (n_envs, M, 16, 16, 3) and one.dtype == torch.uint8 and one.device == eng.device
    assert_frames_equal(one.cpu().numpy(), want_obs[k], 'rollout_frames(step=%d)' % k)
  best = r.episode_return().argmax(1).int()
  idx = np.arange(n_envs)
  picked = env.rollout_frames(candidates=best, step=2)
  assert tuple(picked.shape) == (n_envs, 16, 16, 3)
  assert_frames_equal(picked.cpu().numpy(), want_obs[2][idx, best.cpu().numpy()], 'picked, step 2')
  plan = env.rollout_frames(candidates=best, step='all')
  assert tuple(plan.shape) == (n_envs, K, 16, 16, 3) and plan.dtype == torch.uint8 and plan.device == eng.device
  assert_frames_equal(plan.cpu().numpy(), want_obs[:, idx, best.cpu().numpy()].transpose(1, 0, 2, 3, 4), "step='all'")
  direct = eng.rollout_frames(best, step='all')
  assert sorted(direct) == ['error', 'obs'] and tuple(direct['obs'].shape) == (K, n_envs, 16, 16, 3)
  assert tuple(direct['error'].shape) == (K, n_envs) and not direct['error'].any() and torch.equal(direct['obs'].permute(1, 0, 2, 3, 4), plan)
  direct = eng.rollout(kn, positions=True, keep_steps=True)
  assert tuple(direct['x_steps'].shape) == (K, n_envs, M, s) and tuple(direct['n_sprites_steps'].shape) == (K, n_envs, M)
  assert torch.equal(direct['x_steps'].permute(1, 2, 0, 3), pos.x) and torch.equal(direct['y_steps'].permute(1, 2, 0, 3), pos.y)
  assert 'x_steps' not in eng.rollout(kn, keep_steps=True) and 'x_steps' not in eng.rollout(kn, positions=True)
  # the documented raises
  env.rollout(torch.as_tensor(a), keep_steps=True)
  with_raises(lambda: env.rollout_frames(step='all'), ValueError, "step='all' needs candidates")
  with_raises(lambda: env.rollout_frames(step='every', candidates=best), ValueError, "must be an int or 'all'")
  with_raises(lambda: env.rollout_frames(step=-1), ValueError, 'step must be in [0, K)')
  with_raises(lambda: env.rollout_frames(step=K), Exception, 'step = %d is outside [0, %d)' % (K, K))
  env.close()


def _raises(fn, exc, what):
  try:
    fn()
  except exc as e:
    assert what in str(e), (what, e)
    return
  raise AssertionError('did not raise: ' + what)
