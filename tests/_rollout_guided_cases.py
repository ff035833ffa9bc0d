"""Scenarios of swb_rollout_guided (a rollout that draws its candidates from a plan distribution: weighted sprites, a click
inside the chosen sprite, a bell-shaped motion), written against an engine factory so that the emulated suite
(tests/test_emulated_rollout_guided.py) and the GPU suite (tests/test_gpu_rollout_guided.py) run the same checks.

Sizes: N = 4 environments, M = 3 candidates, K = 6 steps after T0 = 3 live steps with episodes of at most 4 steps, so that every
candidate ends, resets and plays on inside the rollout -- the smallest at which the kernel can go wrong: more than one
workgroup per environment and per plan row, a stream that crosses Philox blocks, a FIRST and a LAST step inside.

The expected values are tests/_rollout_guided_model.py: actions, sprites and tries bit for bit, every output of the rollout
against the oracle stepped with the model's actions.  One model run per (workload, plan) serves every test of a process
(`modelled`).  Output buffers are filled with -7 / 9 first, so that a word never written shows.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np
import torch

from spriteworld_amd import _abi
from tests import _parity
from tests import _rollout_guided_model as model
from tests._rollout_cases import K, M, T0, assert_equal, built, rollout, started, _same_state
from tests._rollout_frames_cases import ERR_INVALID, ERR_STATE, assert_frames_equal, frames, start
from tests._rollout_trajectory_cases import assert_steps_equal, step_frames, trajectory

_bits = _parity.bits
N = 4
PARITY = ('goal_s5', 'cluster_s5_f32a', 'f64_drag', 'embodied_s12', 'ragged_s16', 'ragged_s64')
PLANS = ('weighted', 'uniform')                          # 'uniform': choice_cdf NULL
# the plan's width W per workload: max_sprites, below it (W < n: sprites at index >= W are never chosen), 8 for Embodied
WIDTH = {'goal_s5': 5, 'cluster_s5_f32a': 3, 'f64_drag': None, 'embodied_s12': 8, 'ragged_s16': 8, 'ragged_s64': 64}
SEED = 0x7A11C0DE5EED0A17
FAR_BELOW_CAP = 64                                       # (tests/_rollout_random_cases.FAR_BELOW_CAP)
# rows (k, n) of the weighted plan whose weights are all zero / hold a NaN: both take the uniform fallback
ZERO_ROW, NAN_ROW = (1, 1), (2, 1)


def _ptr(t):
  return None if t is None else C.c_void_p(t.data_ptr())


def _raw(a):
  a = np.ascontiguousarray(a)
  return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def action_layout(eng):
  if eng.cfg.action_space == _abi.ACTION_EMBODIED:
    return 2, torch.int32
  return 4, (torch.float32 if eng.cfg.action_is_f32 else torch.float64)


def make_plan(name, cfg, kind='weighted', n_steps=K, seed=5):
  """The plan of a case, numpy arrays in the C layout: dict(weights [K, N, W], cdf [K, N, W] or None, width, mean, std [K, N, 2]
  or None).  Weights: uniform draws with about four in ten set to exactly 0; ZERO_ROW all zero, NAN_ROW with a NaN.  Motion per
  environment: 0 -- mean 0.05, std 0.3 (clipped at 0); 1 -- mean 0.95, std 0.3 (clipped at 1); 2 -- std 0 (exactly the mean);
  3 -- mean 0.5, std 0.25."""
  rng = np.random.default_rng(seed)
  embodied = cfg.action_space == _abi.ACTION_EMBODIED
  width = WIDTH[name] or cfg.max_sprites
  n = cfg.n_envs
  weights = rng.uniform(0.0, 1.0, (n_steps, n, width)) * (rng.uniform(0.0, 1.0, (n_steps, n, width)) > 0.4)
  if n_steps > max(ZERO_ROW[0], NAN_ROW[0]):
    weights[ZERO_ROW] = 0.0
    weights[NAN_ROW][width // 2] = np.nan
  plan = {'weights': weights, 'cdf': np.cumsum(weights, axis=-1) if kind == 'weighted' else None, 'width': width, 'mean': None, 'std': None}
  if not embodied:
    mean, std = np.zeros((n_steps, n, 2)), np.zeros((n_steps, n, 2))
    rows = [(0.05, 0.3), (0.95, 0.3), (0.37, 0.0), (0.5, 0.25)]
    for e in range(n):
      mean[:, e], std[:, e] = rows[e % 4]
    mean[:, 2::4, 1] = 0.625                             # (another exact mean for the second component)
    plan['mean'], plan['std'] = mean, std
  return plan


def raw_guided(eng, plan, seed, n_cand, n_steps, first_env=0, keep=False, out=True, steps=None, sampled=('actions', 'sprite', 'tries'),
               null_plan=False):
  """(status, message, outputs, per-step outputs, drawn) of swb_rollout_guided called on the engine's handle as given.  The
  buffers are tensors on the engine's device filled with garbage first (error: zeros, it is ORed into).  plan: dict(cdf, width,
  mean, std) of numpy arrays or None each; `steps` defaults to `keep`; `sampled`: which pointers of
  swb_rollout_sampled_outputs are given, or None for a NULL struct."""
  n, s = eng.N, eng.S
  kk, mm = max(min(n_steps, 64), 1), max(min(n_cand, 64), 1)      # (a refused size gets small buffers: nothing is written)
  a_width, a_dtype = action_layout(eng)
  full = lambda shape, value, dtype: torch.full(shape, value, dtype=dtype, device=eng.device)
  res = {'reward': full((kk, n, mm), -7.0, torch.float64), 'discount': full((kk, n, mm), -7.0, torch.float32),
         'step_type': full((kk, n, mm), 9, torch.uint8), 'success': full((kk, n, mm), 9, torch.uint8),
         'error': full((n, mm), 0, torch.uint8), 'x': full((n, mm, s), -7.0, torch.float64), 'y': full((n, mm, s), -7.0, torch.float64),
         'n_sprites': full((n, mm), -7, torch.int32)}
  per = {'x': full((kk, n, mm, s), -7.0, torch.float64), 'y': full((kk, n, mm, s), -7.0, torch.float64),
         'n_sprites': full((kk, n, mm), -7, torch.int32)}
  drawn = {'actions': full((kk, n, mm, a_width), -7, a_dtype), 'sprite': full((kk, n, mm), -7, torch.int32),
           'tries': full((kk, n, mm), -7, torch.int32)}
  o, so, sa, pl = _abi.SwbRolloutOutputs(), _abi.SwbRolloutStepOutputs(), _abi.SwbRolloutSampledOutputs(), _abi.SwbRolloutPlan()
  for k, t in res.items():
    setattr(o, k, t.data_ptr())
  for k, t in per.items():
    setattr(so, k, t.data_ptr())
  for k in (sampled or ()):
    setattr(sa, k, drawn[k].data_ptr())
  held = {}
  for field, key in (('choice_cdf', 'cdf'), ('motion_mean', 'mean'), ('motion_std', 'std')):
    if plan.get(key) is not None:
      held[key] = torch.as_tensor(np.ascontiguousarray(plan[key], dtype=np.float64)).to(eng.device)
      setattr(pl, field, held[key].data_ptr())
  pl.width = int(plan['width'])
  steps = keep if steps is None else steps
  rc = eng.lib.swb_rollout_guided(eng._h, None if null_plan else C.byref(pl), C.c_uint64(seed), C.c_uint64(first_env), int(n_cand),
                                  int(n_steps), int(keep), C.byref(o) if out else None, C.byref(so) if steps else None,
                                  C.byref(sa) if sampled is not None else None, eng._stream())
  eng._sync()
  return rc, (eng.lib.swb_last_error().decode() if rc else ''), res, per, drawn


def guided(eng, plan, seed=SEED, n_cand=M, n_steps=K, first_env=0, keep=False):
  """swb_rollout_guided through the handle -> (outputs, per-step outputs, drawn) as dicts of numpy arrays in the C layout."""
  which = ('actions', 'sprite') if eng.cfg.action_space == _abi.ACTION_EMBODIED else ('actions', 'sprite', 'tries')
  rc, msg, res, per, drawn = raw_guided(eng, plan, seed, n_cand, n_steps, first_env=first_env, keep=keep, sampled=which)
  assert rc == 0, msg
  host = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
  return host(res), host(per), {k: v for k, v in host(drawn).items() if k in which}


_MODELLED = {}


def modelled(name, kind, cfg, pool, live):
  """(plan, drawn, want): tests/_rollout_guided_model.rollout of (workload, plan) at the sizes and the seed of this module, run
  once per process."""
  key = (name, kind)
  if key not in _MODELLED:
    plan = make_plan(name, cfg, kind)
    drawn, want = model.rollout(cfg, pool, live, SEED, 0, plan, M, K)
    for a in list(drawn.values()) + list(want.values()):
      a.setflags(write=False)
    _MODELLED[key] = (plan, drawn, want)
  return _MODELLED[key]


def assert_coverage(name, kind, cfg, plan, drawn, want):
  """The conditions under which a parity case proves something, on the model's values alone."""
  embodied = cfg.action_space == _abi.ACTION_EMBODIED
  how, sprite, n_acted = drawn['how'], drawn['sprite'], drawn['n_acted']
  width = plan['width']
  assert (want['step_type'][1:] == _abi.STEP_LAST).any() and (want['step_type'][1:] == _abi.STEP_FIRST).any(), name
  chosen = how != model.NO_SPRITE
  assert (sprite[chosen] >= 0).all() and (sprite[chosen] < n_acted[chosen]).all(), name
  if kind == 'uniform':
    assert (how[chosen] == model.FALLBACK_NO_CDF).all() and chosen.any(), name
  else:
    weighted = (how == model.WEIGHTED) | (how == model.WEIGHTED_ROUNDED_UP)
    assert weighted.any(), name
    # a sprite of weight 0 (or at an index >= W) is never chosen, although the uniform choice would have taken one
    uniform_would, zero_taken = 0, 0
    for k, e, m in zip(*np.nonzero(weighted)):
      w = plan['weights'][k, e]
      s = int(sprite[k, e, m])
      assert s < width and w[s] > 0.0, (name, k, e, m, s)
      u = min(int(drawn['u_c'][k, e, m] * n_acted[k, e, m]), n_acted[k, e, m] - 1)
      uniform_would += int(u >= width or not w[u] > 0.0)
    assert uniform_would > 0, (name, 'the uniform choice never lands on a sprite without weight')
    # the all-zero row and the row with a NaN take the fallback, wherever there was a sprite to choose
    for row in (ZERO_ROW, NAN_ROW):
      there = chosen[row]
      if row == NAN_ROW and not embodied:                 # (a NaN behind the first W' running sums does not reach the total)
        there = there & (n_acted[row] > width // 2)
      assert (how[row][there] == model.FALLBACK_TOTAL).all(), (name, row)
    assert (how == model.FALLBACK_TOTAL).any(), (name, 'no fallback')
  if embodied:
    assert (drawn['tries'] == -9).all()
    return
  tries = drawn['tries']
  assert (tries > 1).any(), (name, 'no rejected draw')
  assert (tries <= FAR_BELOW_CAP).all() and ((tries >= 1) == (sprite >= 0)).all() and ((tries == 0) == (sprite == -1)).all(), name
  if name == 'cluster_s5_f32a' or name == 'ragged_s16':
    assert (n_acted > width).any(), (name, 'no W < n')
  if name == 'ragged_s64':
    assert ((n_acted > 0) & (n_acted < width)).any(), (name, 'no n < W')
    assert (sprite == -1).any(), (name, 'no environment without sprites')
    assert sprite.max() >= 16, (name, int(sprite.max()))
  # the motion: clipped at 0 and at 1, and exactly the mean where std is 0
  v, motion = drawn['v'], drawn['actions'][..., 2:].astype(np.float64)
  assert ((v < 0.0) & (motion == 0.0)).any() and ((v > 1.0) & (motion == 1.0)).any(), name
  assert (motion >= 0.0).all() and (motion <= 1.0).all()
  still = plan['std'][:, :, None, :] == 0.0
  still = np.broadcast_to(still, v.shape)
  assert still.any() and (v[still] == np.broadcast_to(plan['mean'][:, :, None, :], v.shape)[still]).all(), name
  assert (np.abs(drawn['z']) > 0.5).any()


# ---------------------------------------------------------------------------------------------------------------------
def parity_case(make_engine, name, kind):
  """1. actions, sprite and tries bit for bit against the model; reward, discount, step type, success, error and the end
  positions against the oracle stepped with the model's actions; with keep_steps the per-step states too."""
  cfg, pool, sample, eng, live, rng = started(make_engine, name, n_envs=N)
  before = eng.state()
  plan, drawn, want = modelled(name, kind, cfg, pool, live)
  assert_coverage(name, kind, cfg, plan, drawn, want)
  got, _, got_drawn = guided(eng, plan)
  what = '%s %s' % (name, kind)
  assert got_drawn['actions'].dtype == drawn['actions'].dtype, what
  np.testing.assert_array_equal(_raw(got_drawn['actions']), _raw(drawn['actions']), err_msg='actions ' + what)
  np.testing.assert_array_equal(got_drawn['sprite'], drawn['sprite'], err_msg='sprite ' + what)
  if 'tries' in got_drawn:
    np.testing.assert_array_equal(got_drawn['tries'], drawn['tries'], err_msg='tries ' + what)
  assert_equal(got, want, what)
  _same_state(eng.state(), before)
  got, got_steps, got_drawn = guided(eng, plan, keep=True)
  np.testing.assert_array_equal(_raw(got_drawn['actions']), _raw(drawn['actions']), err_msg='actions, keep_steps ' + what)
  np.testing.assert_array_equal(got_drawn['sprite'], drawn['sprite'], err_msg='sprite, keep_steps ' + what)
  assert_equal(got, want, what + ' keep_steps')
  assert_steps_equal(got_steps, {k: want[k + '_steps'] for k in ('x', 'y', 'n_sprites')}, what)
  _same_state(eng.state(), before)
  eng.close()


def replay_case(make_engine, name):
  """2. Needs no model: the drawn actions fed to plain swb_rollout give every output bit-equal; with keep_steps, x, y and
  n_sprites of every step equal swb_rollout_trajectory of those actions."""
  cfg, pool, sample, eng, live, rng = started(make_engine, name, n_envs=N)
  plan = make_plan(name, cfg)
  got, _, drawn = guided(eng, plan, seed=SEED + 1)
  assert_equal(rollout(eng, drawn['actions']), got, 'replay %s' % name)
  kept, kept_steps, kept_drawn = guided(eng, plan, seed=SEED + 1, keep=True)
  np.testing.assert_array_equal(_raw(kept_drawn['actions']), _raw(drawn['actions']))
  assert_equal(kept, got, 'keep_steps against the plain form')
  replayed, replayed_steps = trajectory(eng, drawn['actions'])
  assert_equal(replayed, kept, 'trajectory replay %s' % name)
  assert_steps_equal(kept_steps, replayed_steps, 'trajectory replay %s' % name)
  assert (kept['step_type'][1:] == _abi.STEP_FIRST).any(), name
  eng.close()


def stream_case(make_engine, name='goal_s5'):
  """3. A candidate's stream depends neither on K nor on M, differs between seeds and is offset by first_env, its high word
  included (against the model)."""
  cfg, pool, sample, eng, live, rng = started(make_engine, name, n_envs=N)
  plan = make_plan(name, cfg)
  full, _, drawn = guided(eng, plan)
  short, _, drawn_short = guided(eng, plan, n_steps=2)
  for k in drawn:
    np.testing.assert_array_equal(_raw(drawn_short[k]), _raw(drawn[k][:2]), err_msg='%s, K = 2 of 6' % k)
  np.testing.assert_array_equal(_bits(short['reward']), _bits(full['reward'][:2]))
  few, _, drawn_few = guided(eng, plan, n_cand=2)
  for k in drawn:
    np.testing.assert_array_equal(_raw(drawn_few[k]), _raw(drawn[k][:, :, :2]), err_msg='%s, M = 2 of 3' % k)
  np.testing.assert_array_equal(_bits(few['reward']), _bits(full['reward'][:, :, :2]))
  _, _, other = guided(eng, plan, seed=SEED + 1)
  # (environment 3: the motion of the others is clipped or has std 0, and equal values prove nothing either way)
  assert (_raw(other['actions'][:, 3]) != _raw(drawn['actions'][:, 3])).mean() > 0.9, 'another seed draws the same actions'
  assert (_raw(drawn['actions'][:, 3, 0]) != _raw(drawn['actions'][:, 3, 1])).mean() > 0.9, 'two candidates draw the same actions'
  # first_env moves every environment to another stream: against the model, which restates the counter words
  for first_env in (1, (1 << 40) + 9):                   # (the low and the high word of the entry)
    _, _, at = guided(eng, plan, first_env=first_env, n_steps=2)
    want_drawn, _ = model.rollout(cfg, pool, live, SEED, first_env, plan, M, 2)
    for k in at:
      np.testing.assert_array_equal(_raw(at[k]), _raw(want_drawn[k]), err_msg='%s, first_env = %d' % (k, first_env))
    assert (_raw(at['actions'][:, 3]) != _raw(drawn['actions'][:2, 3])).mean() > 0.9
  eng.close()


def handle_case(make_engine, name='goal_s5'):
  """4. The handle is as it was: state() bit-equal, a caller's marks in the sticky error buffer, and the next K real steps
  equal the oracle's (frames +-0) and candidate 0, whose drawn actions they take."""
  from oracle import oracle
  cfg, pool, sample, eng, live, rng = started(make_engine, name, n_envs=N)
  plan = make_plan(name, cfg)
  ora = oracle.Engine(cfg, pool)
  for a in live:
    ora.step(a, render=False)
  marks = (np.arange(cfg.n_envs) % 3 == 0).astype(np.uint8) * 0x40        # a caller's unread flags (no bit the engine sets)
  eng.error.copy_(torch.as_tensor(marks))
  before = eng.state()
  for keep in (False, True):
    got, _, drawn = guided(eng, plan, keep=keep)
    _same_state(eng.state(), before)
    np.testing.assert_array_equal(eng.outputs_host()['error'], marks)
  eng.error.zero_()
  acts = drawn['actions']
  for k in range(K):
    a = acts[k, :, 0]
    want = ora.step(a)
    eng.step(a)
    out = eng.outputs_host()
    _parity.compare(k, ora, eng, want, out, what='after a guided rollout')
    np.testing.assert_array_equal(out['step_type'], got['step_type'][k, :, 0])
    np.testing.assert_array_equal(_bits(out['reward']), _bits(got['reward'][k, :, 0]))
  st = eng.state()
  np.testing.assert_array_equal(_bits(st['x']), _bits(got['x'][:, 0]))
  np.testing.assert_array_equal(_bits(st['y']), _bits(got['y'][:, 0]))
  eng.close()


def frames_case(make_engine, name='goal_s5'):
  """5. After a guided rollout swb_rollout_frames with picked candidates equals, byte for byte, the frames after replaying the
  actions through swb_rollout; with keep_steps the same for swb_rollout_step_frames(step = 1) against swb_rollout_trajectory."""
  cfg, pool, sample, eng, live, rng = start(make_engine, name, n_envs=N)
  plan = make_plan(name, cfg)
  pick = (np.arange(cfg.n_envs) * 2 + 1) % M
  _, _, drawn = guided(eng, plan)
  ends, ends_all = frames(eng, M, pick), frames(eng, M)
  rollout(eng, drawn['actions'])
  assert_frames_equal(ends, frames(eng, M, pick), 'picked end frames')
  assert_frames_equal(ends_all, frames(eng, M), 'end frames of all candidates')
  assert any((ends_all[n, 0] != ends_all[n, m]).any() for n in range(cfg.n_envs) for m in range(1, M))
  guided(eng, plan, keep=True)
  second, last = step_frames(eng, M, 1, pick), step_frames(eng, M, K - 1, pick)
  assert_frames_equal(last, ends, 'step K - 1 is the end frame')
  trajectory(eng, drawn['actions'])
  assert_frames_equal(second, step_frames(eng, M, 1, pick), 'picked frames of step 1')
  assert (second != last).any()
  # a guided rollout without keep_steps keeps none: swb_rollout_step_frames refuses as after a plain swb_rollout
  guided(eng, plan)
  rc = eng.lib.swb_rollout_step_frames(eng._h, M, 0, None, _ptr(torch.zeros((cfg.n_envs, M) + tuple(eng.obs_shape), dtype=torch.uint8, device=eng.device)),
                                       None, eng._stream())
  assert rc == ERR_STATE and 'kept no steps' in eng.lib.swb_last_error().decode()
  eng.close()


def refusals_case(make_engine):
  """6. Every SWB_ERR_INVALID condition and the SWB_ERR_STATE after a setter, each with a message naming the function."""
  cfg, pool, sample, eng, live, rng = started(make_engine, 'goal_s5', n_envs=N)
  plan = make_plan('goal_s5', cfg)

  def refused(e, pl, code, what, *args, **kw):
    rc, msg, res, per, drawn = raw_guided(e, pl, *args, **kw)
    assert rc == code and what in msg and 'swb_rollout_guided' in msg, (args, kw, rc, msg)
    assert (res['step_type'].cpu().numpy() == 9).all() and (drawn['sprite'].cpu().numpy() == -7).all(), 'a refused call wrote'

  refused(eng, plan, ERR_INVALID, 'plan is NULL', 1, M, K, null_plan=True)
  for width in (0, -1, cfg.max_sprites + 1):
    refused(eng, dict(plan, width=width, cdf=None), ERR_INVALID, 'width = %d is outside' % width, 1, M, K)
  refused(eng, dict(plan, mean=None), ERR_INVALID, 'motion_mean and motion_std are required', 1, M, K)
  refused(eng, dict(plan, std=None), ERR_INVALID, 'motion_mean and motion_std are required', 1, M, K)
  refused(eng, plan, ERR_INVALID, 'sampled->actions is NULL', 1, M, K, sampled=None)
  refused(eng, plan, ERR_INVALID, 'sampled->actions is NULL', 1, M, K, sampled=('sprite', 'tries'))
  refused(eng, plan, ERR_INVALID, 'need keep_steps', 1, M, K, keep=False, steps=True)
  refused(eng, plan, ERR_INVALID, 'M and K must be positive', 1, 0, K)
  refused(eng, plan, ERR_INVALID, 'M and K must be positive', 1, M, 0)
  refused(eng, plan, ERR_INVALID, 'exceed the grid limit', 1, (1 << 24) // cfg.n_envs + 1, K)
  refused(eng, plan, ERR_INVALID, 'exceeds the limit of 65536 steps', 1, M, (1 << 16) + 1)
  rc = eng.lib.swb_rollout_frames(eng._h, M, None, _ptr(eng.obs), None, eng._stream())      # (a refused rollout is none)
  assert rc == ERR_STATE and 'no rollout has run' in eng.lib.swb_last_error().decode()
  # accepted: every optional pointer NULL, width 1
  rc, msg, _, _, _ = raw_guided(eng, dict(plan, cdf=None, width=1), 1, M, K, out=False, sampled=('actions',))
  assert rc == 0, msg
  rc, msg, _, _, _ = raw_guided(eng, plan, 1, M, K, keep=True, steps=False, sampled=('actions',))
  assert rc == 0, msg
  for bad in (dict(outputs=('actions', 'sprites')), dict(M=0), dict(motion_mean=torch.zeros((K, N, 3), dtype=torch.float64))):
    kw = dict(seed=1, M=M, K=K)
    kw.update(bad)
    try:
      eng.rollout_guided(**kw)
    except ValueError:
      pass
    else:
      raise AssertionError('Engine.rollout_guided(%r) did not raise' % (bad,))
  env = int(np.flatnonzero(eng.state()['reset_next'] == 0)[0])
  eng.set_sprite_attr(env, 0, _abi.ATTR_ANGLE, 45.0)
  refused(eng, plan, ERR_STATE, 'sprite setters', 1, M, K)
  eng.close()
  # Embodied: exactly 8 weights, no motion parameters, no tries
  cfg, pool, sample, eng, live, rng = started(make_engine, 'embodied_s12', n_envs=N)
  plan = make_plan('embodied_s12', cfg)
  two = np.zeros((K, N, 2))
  for width in (7, 9, 12):
    refused(eng, dict(plan, width=width, cdf=None), ERR_INVALID, 'exactly 8 action weights', 1, M, K, sampled=('actions', 'sprite'))
  refused(eng, dict(plan, mean=two), ERR_INVALID, 'must be NULL for an Embodied', 1, M, K, sampled=('actions', 'sprite'))
  refused(eng, dict(plan, std=two), ERR_INVALID, 'must be NULL for an Embodied', 1, M, K, sampled=('actions', 'sprite'))
  refused(eng, plan, ERR_INVALID, 'tries must be NULL for an Embodied', 1, M, K)
  eng.close()


# ---------------------------------------------------------------------------------------------------------------------
def surface_case(n_envs=4):
  """7. BatchedEnvironment.rollout_guided.  The engine class is environment._engine.Engine: the caller has patched the
  emulated one in, or runs on the GPU."""
  from spriteworld_amd import environment
  from tests._random_agent_cases import _surface_env
  env = _surface_env(n_envs)       # a noiseless SelectMove, three sprites, float64 actions
  env.reset()
  env.step(env.sample_actions())
  n_sprites = env.engine.S
  dev = env.engine.device
  idx = torch.arange(n_envs, device=dev)
  weights = torch.zeros((n_envs, K, n_sprites), dtype=torch.float32, device=dev)
  weights[:, :, 1] = 2.0                                  # every click on sprite 1 ...
  weights[:, :, 0] = -5.0                                 # (... a negative weight counts as 0)
  weights[0, 0] = 0.0                                     # ... except where the row is all zero: uniform
  mean = torch.full((n_envs, K, 2), 0.25, dtype=torch.float64, device=dev)
  env.seed_actions(4)
  r, actions, sprite = env.rollout_guided(M, K, sprite_weights=weights, motion_mean=mean, motion_std=0.0)
  assert isinstance(r, environment.Rollout)
  for f in ('step_type', 'reward', 'discount', 'success'):
    assert tuple(getattr(r, f).shape) == (n_envs, M, K), f
  assert tuple(r.x.shape) == tuple(r.y.shape) == (n_envs, M, n_sprites) and tuple(r.n_sprites.shape) == tuple(r.error.shape) == (n_envs, M)
  assert tuple(actions.shape) == (n_envs, M, K, 4) and actions.dtype == torch.float64 and actions.device == dev
  assert tuple(sprite.shape) == (n_envs, M, K) and sprite.dtype == torch.int32
  sp = sprite.cpu().numpy()
  rest = np.ones(sp.shape, bool)
  rest[0, :, 0] = False
  assert (sp[rest] == 1).all() and (sp >= 0).all() and (sp < n_sprites).all()
  assert (actions[..., 2:] == 0.25).all(), 'std 0 gives exactly the mean'
  # the layout rollout() accepts: the same Rollout, bit for bit
  again = env.rollout(actions)
  for f in r._fields:
    np.testing.assert_array_equal(_raw(getattr(again, f).cpu().numpy()), _raw(getattr(r, f).cpu().numpy()), err_msg=f)
  # seed_actions(s) reproduces it; the next call draws another key; no weights, scalar motion: the defaults
  _, other, _ = env.rollout_guided(M, K)
  assert ((other[..., 2:] >= 0) & (other[..., 2:] <= 1)).all() and other[..., 2:].std() > 0.1
  env.seed_actions(4)
  r2, actions2, sprite2 = env.rollout_guided(M, K, sprite_weights=weights, motion_mean=mean, motion_std=0.0)
  assert torch.equal(actions2, actions) and torch.equal(sprite2, sprite) and not torch.equal(other, actions)
  np.testing.assert_array_equal(_bits(r2.reward.cpu().numpy()), _bits(r.reward.cpu().numpy()))
  # execute the best plan's first step: the live batch returns what the rollout said (the action space is noiseless)
  best = r2.episode_return().argmax(1)
  picked = env.rollout_frames(candidates=best)
  assert tuple(picked.shape) == (n_envs, 16, 16, 3) and picked.dtype == torch.uint8
  assert len(env.rollout_snapshot(best)) == n_envs
  try:
    env.rollout_positions()
  except environment.EnvironmentError_ as e:
    assert 'kept no steps' in str(e)
  else:
    raise AssertionError('rollout_positions after a rollout_guided that kept no steps did not raise')
  ts = env.step(actions[idx, best, 0])
  host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
  np.testing.assert_array_equal(host(ts.step_type), host(r.step_type[idx, best, 0]))
  np.testing.assert_array_equal(_bits(host(ts.reward).astype(np.float64)), _bits(host(r.reward[idx, best, 0])))
  # keep_steps: positions and frames per step
  r, actions, sprite = env.rollout_guided(M, K, sprite_weights=weights, keep_steps=True)
  pos = env.rollout_positions()
  assert tuple(pos.x.shape) == (n_envs, M, K, n_sprites) and torch.equal(pos.x[:, :, K - 1], r.x)
  assert tuple(env.rollout_frames(step=1).shape) == (n_envs, M, 16, 16, 3)
  for bad in (dict(sprite_weights=weights[:, :2]), dict(motion_mean=torch.zeros((n_envs, K, 3))), dict(sprite_weights=weights[0])):
    try:
      env.rollout_guided(M, K, **bad)
    except ValueError as e:
      assert 'rollout_guided' in str(e)
    else:
      raise AssertionError('rollout_guided(%r) did not raise' % (sorted(bad),))
  env.close()


def offsets_case(n_envs=4):
  """7. global_env_offset is the kernel's first_env: two shards with one seed draw the two halves of the whole batch's streams."""
  from tests._random_agent_cases import _surface_env
  whole, lo, hi = _surface_env(n_envs), _surface_env(n_envs // 2), _surface_env(n_envs // 2, global_env_offset=n_envs // 2)
  out = []
  for env in (whole, lo, hi):
    env.reset()
    env.seed_actions(12)
    out.append(env.rollout_guided(2, 2)[1].cpu().numpy())
    env.close()
  assert np.array_equal(out[0], np.concatenate([out[1], out[2]])) and not np.array_equal(out[1], out[2])


def groups_case(n_envs=4):
  """7. EnvironmentGroups (GPU: it owns HIP streams): the per-group form, on the group's stream."""
  from spriteworld_amd import environment
  from tests._random_agent_cases import _surface_env
  groups = _surface_env(n_envs, cls=environment.EnvironmentGroups, num_groups=2)
  draws = []
  for g in range(2):
    groups.reset(g)
    groups.groups[g].seed_actions(12)
    with torch.cuda.stream(groups.streams[g]):
      weights = torch.ones((n_envs // 2, 2, groups.groups[g].engine.S), device=groups.groups[g].engine.device)
      weights[:, :, 0] = 0.0
    r, actions, sprite = groups.rollout_guided(g, M, 2, sprite_weights=weights, motion_std=0.1)
    assert isinstance(r, environment.Rollout) and tuple(actions.shape) == (n_envs // 2, M, 2, 4) and tuple(sprite.shape) == (n_envs // 2, M, 2)
    draws.append((actions, sprite))
  groups.synchronize()                                  # (a group's tensors are valid on the group's stream)
  draws = [(a.cpu().numpy(), s.cpu().numpy()) for a, s in draws]
  groups.close()
  assert not np.array_equal(draws[0][0], draws[1][0]) and all((s >= 1).all() for _, s in draws)
