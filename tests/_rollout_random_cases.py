"""Scenarios of swb_rollout_sampled (a rollout that draws its candidates' actions in the kernel, uniform or as clicks on
sprites), written against an engine factory so that the emulated suite (tests/test_emulated_rollout_random.py) and the GPU
suite (tests/test_gpu_rollout_random.py) run the same checks.  Sizes are those of tests/_rollout_cases.py: N = 16, M = 3,
K = 6 after T0 = 3 live steps with episodes of at most 4 steps, so that every candidate ends, resets and plays on inside the
rollout.

The expected values are tests/_rollout_random_model.py: the Philox stream of every virtual environment restated, an
oracle.Engine per candidate stepped with the actions drawn so far -- actions, sprites and tries bit for bit, every output of the
rollout against that oracle.  One model run per (workload, mode) serves every test of a process (`modelled`).  Output buffers
are filled with garbage first (-7 / 9 / 0x5A), so that a word never written shows.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np
import torch

from spriteworld_amd import _abi
from tests import _parity
from tests import _rollout_random_model as model
from tests._rollout_cases import K, M, N_ENVS, T0, assert_equal, built, rollout, started, _same_state
from tests._rollout_frames_cases import ERR_INVALID, ERR_STATE, assert_frames_equal, frames, start
from tests._rollout_trajectory_cases import assert_steps_equal, step_frames, trajectory

_bits = _parity.bits
UNIFORM, ON_SPRITE = _abi.SAMPLE_UNIFORM, _abi.SAMPLE_ON_SPRITE
MODES = {'uniform': UNIFORM, 'sprite': ON_SPRITE}
PARITY = ('goal_s5', 'cluster_s5_f32a', 'f64_drag', 'embodied_s12', 'ragged_s16', 'ragged_s64')
CONTAINED = ('goal_s5', 'ragged_s16', 'ragged_s64')      # float64-action SelectMove workloads
SEED = 0x51ED270B9F3C4A11
# a tries count "far below the cap" (tests/_random_agent_cases.FAR_BELOW_CAP: 0.6464^64 < 1e-12 per draw)
FAR_BELOW_CAP = 64


def _ptr(t):
  return None if t is None else C.c_void_p(t.data_ptr())


def _raw(a):
  a = np.ascontiguousarray(a)
  return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def action_layout(eng):
  if eng.cfg.action_space == _abi.ACTION_EMBODIED:
    return 2, torch.int32
  return 4, (torch.float32 if eng.cfg.action_is_f32 else torch.float64)


def raw_sampled(eng, mode, seed, n_cand, n_steps, first_env=0, keep=False, out=True, steps=None, sampled=('actions', 'sprite', 'tries')):
  """(status, message, outputs, per-step outputs, drawn) of swb_rollout_sampled called on the engine's handle as given.  The
  buffers are tensors on the engine's device filled with garbage first (error: zeros, it is ORed into).  `steps` defaults to
  `keep`; `sampled`: which pointers of swb_rollout_sampled_outputs are given, or None for a NULL struct."""
  n, s = eng.N, eng.S
  kk, mm = max(min(n_steps, 64), 1), max(min(n_cand, 64), 1)      # (a refused size gets small buffers: nothing is written)
  width, a_dtype = action_layout(eng)
  full = lambda shape, value, dtype: torch.full(shape, value, dtype=dtype, device=eng.device)
  res = {'reward': full((kk, n, mm), -7.0, torch.float64), 'discount': full((kk, n, mm), -7.0, torch.float32),
         'step_type': full((kk, n, mm), 9, torch.uint8), 'success': full((kk, n, mm), 9, torch.uint8),
         'error': full((n, mm), 0, torch.uint8), 'x': full((n, mm, s), -7.0, torch.float64), 'y': full((n, mm, s), -7.0, torch.float64),
         'n_sprites': full((n, mm), -7, torch.int32)}
  per = {'x': full((kk, n, mm, s), -7.0, torch.float64), 'y': full((kk, n, mm, s), -7.0, torch.float64),
         'n_sprites': full((kk, n, mm), -7, torch.int32)}
  drawn = {'actions': full((kk, n, mm, width), -7, a_dtype), 'sprite': full((kk, n, mm), -7, torch.int32),
           'tries': full((kk, n, mm), -7, torch.int32)}
  o, so, sa = _abi.SwbRolloutOutputs(), _abi.SwbRolloutStepOutputs(), _abi.SwbRolloutSampledOutputs()
  for k, t in res.items():
    setattr(o, k, t.data_ptr())
  for k, t in per.items():
    setattr(so, k, t.data_ptr())
  for k in (sampled or ()):
    setattr(sa, k, drawn[k].data_ptr())
  steps = keep if steps is None else steps
  rc = eng.lib.swb_rollout_sampled(eng._h, int(mode), C.c_uint64(seed), C.c_uint64(first_env), int(n_cand), int(n_steps), int(keep),
                                   C.byref(o) if out else None, C.byref(so) if steps else None,
                                   C.byref(sa) if sampled is not None else None, eng._stream())
  eng._sync()
  return rc, (eng.lib.swb_last_error().decode() if rc else ''), res, per, drawn


def sampled(eng, mode, seed=SEED, n_cand=M, n_steps=K, first_env=0, keep=False):
  """swb_rollout_sampled through the handle -> (outputs, per-step outputs, drawn) as dicts of numpy arrays in the C layout."""
  which = ('actions', 'sprite', 'tries') if mode == ON_SPRITE else ('actions',)
  rc, msg, res, per, drawn = raw_sampled(eng, mode, seed, n_cand, n_steps, first_env=first_env, keep=keep, sampled=which)
  assert rc == 0, msg
  host = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
  return host(res), host(per), {k: v for k, v in host(drawn).items() if k in which}


_MODELLED = {}


def modelled(name, mode, cfg, pool, live):
  """tests/_rollout_random_model.rollout of (workload, mode) at the sizes and the seed of this module, run once per process."""
  key = (name, mode)
  if key not in _MODELLED:
    drawn, want = model.rollout(cfg, pool, live, SEED, 0, mode, M, K)
    for a in list(drawn.values()) + list(want.values()):
      if isinstance(a, np.ndarray):
        a.setflags(write=False)
    _MODELLED[key] = (drawn, want)
  return _MODELLED[key]


def assert_coverage(name, mode, drawn, want):
  """The conditions under which a parity case proves something, on the model's values alone."""
  assert (want['step_type'][1:] == _abi.STEP_LAST).any() and (want['step_type'][1:] == _abi.STEP_FIRST).any(), name
  if mode == ON_SPRITE:
    tries, sprite = drawn['tries'], drawn['sprite']
    assert (tries > 1).any(), (name, 'no rejected draw')
    assert (tries <= FAR_BELOW_CAP).all() and ((tries >= 1) == (sprite >= 0)).all() and ((tries == 0) == (sprite == -1)).all(), name
    if name == 'ragged_s16':
      assert (sprite == -1).any(), (name, 'no environment without sprites')
    if name == 'ragged_s64':
      assert sprite.max() > _abi.SWB_TUNED_SPRITES, (name, int(sprite.max()))


# ---------------------------------------------------------------------------------------------------------------------
def parity_case(make_engine, name, mode):
  """1. actions, sprite and tries bit for bit against the model; reward, discount, step type, success, error and the end
  positions against the oracle stepped with the model's actions; with keep_steps the per-step states too."""
  cfg, pool, sample, eng, live, rng = started(make_engine, name)
  before = eng.state()
  drawn, want = modelled(name, mode, cfg, pool, live)
  assert_coverage(name, mode, drawn, want)
  got, _, got_drawn = sampled(eng, mode)
  what = '%s mode %d' % (name, mode)
  assert got_drawn['actions'].dtype == drawn['actions'].dtype, what
  np.testing.assert_array_equal(_raw(got_drawn['actions']), _raw(drawn['actions']), err_msg='actions ' + what)
  if mode == ON_SPRITE:
    np.testing.assert_array_equal(got_drawn['sprite'], drawn['sprite'], err_msg='sprite ' + what)
    np.testing.assert_array_equal(got_drawn['tries'], drawn['tries'], err_msg='tries ' + what)
  assert_equal(got, want, what)
  _same_state(eng.state(), before)
  got, got_steps, got_drawn = sampled(eng, mode, keep=True)
  np.testing.assert_array_equal(_raw(got_drawn['actions']), _raw(drawn['actions']), err_msg='actions, keep_steps ' + what)
  assert_equal(got, want, what + ' keep_steps')
  assert_steps_equal(got_steps, {k: want[k + '_steps'] for k in ('x', 'y', 'n_sprites')}, what)
  _same_state(eng.state(), before)
  eng.close()


def replay_case(make_engine, name, mode):
  """2. Needs no model: the drawn actions fed to plain swb_rollout give every output bit-equal; with keep_steps, x, y and
  n_sprites of every step equal swb_rollout_trajectory of those actions."""
  cfg, pool, sample, eng, live, rng = started(make_engine, name)
  got, _, drawn = sampled(eng, mode, seed=SEED + 1)
  assert_equal(rollout(eng, drawn['actions']), got, 'replay %s mode %d' % (name, mode))
  kept, kept_steps, kept_drawn = sampled(eng, mode, seed=SEED + 1, keep=True)
  np.testing.assert_array_equal(_raw(kept_drawn['actions']), _raw(drawn['actions']))
  assert_equal(kept, got, 'keep_steps against the plain form')
  replayed, replayed_steps = trajectory(eng, drawn['actions'])
  assert_equal(replayed, kept, 'trajectory replay %s mode %d' % (name, mode))
  assert_steps_equal(kept_steps, replayed_steps, 'trajectory replay %s mode %d' % (name, mode))
  assert (kept['step_type'][1:] == _abi.STEP_FIRST).any(), name
  eng.close()


def containment_case(name):
  """3. Independent of the engine's hit test: for a float64-action SelectMove workload every (k, n, m) with tries >= 1 has
  oracle.contains_point true for the chosen sprite at click - position, positions from the model run (which parity_case pins
  the engine to)."""
  from oracle import oracle
  cfg, pool, sample = built(name)
  assert cfg.action_is_f32 == 0 and cfg.action_space == _abi.ACTION_SELECT_MOVE, name
  rng = np.random.default_rng(100)                                   # (tests/_rollout_cases.started's live steps)
  live = [sample(rng) for _ in range(T0)]
  drawn, want = modelled(name, ON_SPRITE, cfg, pool, live)
  checked = 0
  for k, e, m in zip(*np.nonzero(drawn['tries'] >= 1)):
    s = int(drawn['sprite'][k, e, m])
    shape, scale, angle = drawn['shape_of'][(k, e, m)]
    click = drawn['actions'][k, e, m, :2]
    assert oracle.contains_point(shape, scale, angle, click[0] - drawn['pos_x'][k, e, m, s], click[1] - drawn['pos_y'][k, e, m, s]), (k, e, m, s)
    checked += 1
  assert checked > N_ENVS * M * K // 2, checked


def stream_case(make_engine, name='goal_s5'):
  """4. A candidate's stream depends neither on K nor on M, differs between seeds, is offset by first_env, and is not the
  stream swb_sample_actions draws under the same seed."""
  cfg, pool, sample, eng, live, rng = started(make_engine, name)
  for mode in (UNIFORM, ON_SPRITE):
    full, _, drawn = sampled(eng, mode)
    short, _, drawn_short = sampled(eng, mode, n_steps=2)
    for k in drawn:
      np.testing.assert_array_equal(_raw(drawn_short[k]), _raw(drawn[k][:2]), err_msg='%s, K = 2 of 6, mode %d' % (k, mode))
    np.testing.assert_array_equal(_bits(short['reward']), _bits(full['reward'][:2]))
    few, _, drawn_few = sampled(eng, mode, n_cand=2)
    for k in drawn:
      np.testing.assert_array_equal(_raw(drawn_few[k]), _raw(drawn[k][:, :, :2]), err_msg='%s, M = 2 of 3, mode %d' % (k, mode))
    np.testing.assert_array_equal(_bits(few['reward']), _bits(full['reward'][:, :, :2]))
    _, _, other = sampled(eng, mode, seed=SEED + 1)
    assert (_raw(other['actions']) != _raw(drawn['actions'])).mean() > 0.9, 'another seed draws the same actions'
    # candidates differ from each other
    assert (_raw(drawn['actions'][:, :, 0]) != _raw(drawn['actions'][:, :, 1])).mean() > 0.9
    # the fourth counter word: no value of step 0 is swb_sample_actions' under the same seed
    live_draw = eng.sample_actions(mode, SEED, outputs=('actions',))['actions'].cpu().numpy()
    assert not (_raw(drawn['actions'][0]) == _raw(live_draw)[:, None, :]).any(), 'a candidate replays the stream of swb_sample_actions'
  _, _, at0 = sampled(eng, UNIFORM)
  _, _, at5 = sampled(eng, UNIFORM, first_env=5)
  np.testing.assert_array_equal(_raw(at5['actions'][:, 0]), _raw(at0['actions'][:, 5]), err_msg='first_env = 5')
  np.testing.assert_array_equal(_raw(at5['actions'][:, :N_ENVS - 5]), _raw(at0['actions'][:, 5:]))
  _, _, far = sampled(eng, UNIFORM, first_env=(1 << 40) + 9)     # (the high word of the entry)
  want = np.array([[model.draw_step(model.CandidateStream(SEED, (1 << 40) + 9 + e, m), UNIFORM, cfg, None)[0] for m in range(M)]
                   for e in range(N_ENVS)])
  np.testing.assert_array_equal(_raw(far['actions'][0]), _raw(want), err_msg='first_env = 2^40 + 9')
  eng.close()


def handle_case(make_engine, name='goal_s5'):
  """5. The handle is as it was: state() bit-equal, a caller's marks in the sticky error buffer, and the next K real steps
  equal the oracle's (frames +-0) and candidate 0, whose drawn actions they take."""
  from oracle import oracle
  cfg, pool, sample, eng, live, rng = started(make_engine, name)
  ora = oracle.Engine(cfg, pool)
  for a in live:
    ora.step(a, render=False)
  marks = (np.arange(cfg.n_envs) % 3 == 0).astype(np.uint8) * 0x40        # a caller's unread flags (no bit the engine sets)
  eng.error.copy_(torch.as_tensor(marks))
  before = eng.state()
  for mode, keep in ((UNIFORM, False), (ON_SPRITE, True)):
    got, _, drawn = sampled(eng, mode, keep=keep)
    _same_state(eng.state(), before)
    np.testing.assert_array_equal(eng.outputs_host()['error'], marks)
  eng.error.zero_()
  acts = drawn['actions']
  for k in range(K):
    a = acts[k, :, 0]
    want = ora.step(a)
    eng.step(a)
    out = eng.outputs_host()
    _parity.compare(k, ora, eng, want, out, what='after a sampled rollout')
    np.testing.assert_array_equal(out['step_type'], got['step_type'][k, :, 0])
    np.testing.assert_array_equal(_bits(out['reward']), _bits(got['reward'][k, :, 0]))
  st = eng.state()
  np.testing.assert_array_equal(_bits(st['x']), _bits(got['x'][:, 0]))
  np.testing.assert_array_equal(_bits(st['y']), _bits(got['y'][:, 0]))
  eng.close()


def frames_case(make_engine, name='goal_s5'):
  """6. After a sampled rollout swb_rollout_frames with picked candidates equals, byte for byte, the frames after replaying the
  actions through swb_rollout; with keep_steps the same for swb_rollout_step_frames(step = 1) against swb_rollout_trajectory."""
  cfg, pool, sample, eng, live, rng = start(make_engine, name)
  pick = (np.arange(cfg.n_envs) * 2 + 1) % M
  _, _, drawn = sampled(eng, ON_SPRITE)
  ends, ends_all = frames(eng, M, pick), frames(eng, M)
  rollout(eng, drawn['actions'])
  assert_frames_equal(ends, frames(eng, M, pick), 'picked end frames')
  assert_frames_equal(ends_all, frames(eng, M), 'end frames of all candidates')
  assert any((ends_all[n, 0] != ends_all[n, m]).any() for n in range(cfg.n_envs) for m in range(1, M))
  sampled(eng, ON_SPRITE, keep=True)
  second, last = step_frames(eng, M, 1, pick), step_frames(eng, M, K - 1, pick)
  assert_frames_equal(last, ends, 'step K - 1 is the end frame')
  assert_frames_equal(frames(eng, M, pick), ends, 'swb_rollout_frames after keep_steps')
  trajectory(eng, drawn['actions'])
  assert_frames_equal(second, step_frames(eng, M, 1, pick), 'picked frames of step 1')
  assert (second != last).any()
  # a sampled rollout without keep_steps keeps none: swb_rollout_step_frames refuses as after a plain swb_rollout
  sampled(eng, UNIFORM)
  rc = eng.lib.swb_rollout_step_frames(eng._h, M, 0, None, _ptr(torch.zeros((cfg.n_envs, M) + tuple(eng.obs_shape), dtype=torch.uint8, device=eng.device)),
                                       None, eng._stream())
  assert rc == ERR_STATE and 'kept no steps' in eng.lib.swb_last_error().decode()
  eng.close()


def refusals_case(make_engine, name='goal_s5'):
  """7. Every SWB_ERR_INVALID condition and the SWB_ERR_STATE after a setter, each with a message naming the function."""
  cfg, pool, sample, eng, live, rng = started(make_engine, name)

  def refused(code, what, *args, **kw):
    rc, msg, res, per, drawn = raw_sampled(eng, *args, **kw)
    assert rc == code and what in msg and 'swb_rollout_sampled' in msg, (args, kw, rc, msg)
    assert (res['step_type'].cpu().numpy() == 9).all() and (drawn['tries'].cpu().numpy() == -7).all(), 'a refused call wrote'

  refused(ERR_INVALID, 'sampled->actions is NULL', ON_SPRITE, 1, M, K, sampled=None)
  refused(ERR_INVALID, 'sampled->actions is NULL', ON_SPRITE, 1, M, K, sampled=('sprite', 'tries'))
  for mode in (2, -1, 77):
    refused(ERR_INVALID, 'unknown mode', mode, 1, M, K)
  refused(ERR_INVALID, 'SWB_SAMPLE_ON_SPRITE only', UNIFORM, 1, M, K, sampled=('actions', 'sprite'))
  refused(ERR_INVALID, 'SWB_SAMPLE_ON_SPRITE only', UNIFORM, 1, M, K, sampled=('actions', 'tries'))
  refused(ERR_INVALID, 'need keep_steps', UNIFORM, 1, M, K, keep=False, steps=True, sampled=('actions',))
  refused(ERR_INVALID, 'M and K must be positive', ON_SPRITE, 1, 0, K)
  refused(ERR_INVALID, 'M and K must be positive', ON_SPRITE, 1, M, 0)
  refused(ERR_INVALID, 'exceed the grid limit', ON_SPRITE, 1, (1 << 24) // cfg.n_envs + 1, K)
  refused(ERR_INVALID, 'exceeds the limit of 65536 steps', ON_SPRITE, 1, M, (1 << 16) + 1)
  rc = eng.lib.swb_rollout_frames(eng._h, M, None, _ptr(eng.obs), None, eng._stream())      # (a refused rollout is none)
  assert rc == ERR_STATE and 'no rollout has run' in eng.lib.swb_last_error().decode()
  # accepted: every optional pointer NULL
  rc, msg, _, _, _ = raw_sampled(eng, ON_SPRITE, 1, M, K, out=False, sampled=('actions',))
  assert rc == 0, msg
  rc, msg, _, _, _ = raw_sampled(eng, UNIFORM, 1, M, K, keep=True, steps=False, sampled=('actions',))
  assert rc == 0, msg
  for bad in (dict(outputs=('actions', 'sprites')), dict(M=0)):
    kw = dict(mode=UNIFORM, seed=1, M=M, K=K)
    kw.update(bad)
    try:
      eng.rollout_sampled(**kw)
    except ValueError:
      pass
    else:
      raise AssertionError('Engine.rollout_sampled(%r) did not raise' % (bad,))
  env = int(np.flatnonzero(eng.state()['reset_next'] == 0)[0])
  eng.set_sprite_attr(env, 0, _abi.ATTR_ANGLE, 45.0)
  refused(ERR_STATE, 'sprite setters', ON_SPRITE, 1, M, K)
  refused(ERR_STATE, 'not supported', UNIFORM, 1, M, K, sampled=('actions',))
  eng.close()


def cap_case(make_engine, name='goal_s5'):
  """8. (The emulator only, as the cap test of swb_sample_actions: 1024 tries of a wave take the device no time, but the case
  needs a pool no generator draws.)  Sprite 0 of every episode has scale 0.0: its path is a point that contains nothing, so a
  draw that chooses it gives tries = -1 and clicks the sprite's own position; other sprites are unaffected, and the rollout
  still equals its replay."""
  cfg, pool, sample = built(name)
  pool.scale[:, 0] = 0.0
  eng = make_engine(cfg, pool)
  rng = np.random.default_rng(100)
  for _ in range(T0):
    eng.step(sample(rng), render=False)
  live_state = eng.state()
  got, steps, drawn = sampled(eng, ON_SPRITE, keep=True)
  capped = drawn['sprite'] == 0
  assert capped.any() and (~capped).any()
  assert (drawn['tries'][capped] == -1).all() and (drawn['tries'][~capped] >= 1).all() and (drawn['tries'][~capped] <= FAR_BELOW_CAP).all()
  for k, e, m in zip(*np.nonzero(capped)):
    if got['step_type'][k, e, m] == _abi.STEP_FIRST:      # the fresh episode, which a FIRST step does not move
      px, py = steps['x'][k, e, m, 0], steps['y'][k, e, m, 0]
    elif k == 0:
      px, py = live_state['x'][e, 0], live_state['y'][e, 0]
    else:
      px, py = steps['x'][k - 1, e, m, 0], steps['y'][k - 1, e, m, 0]
    np.testing.assert_array_equal(_raw(drawn['actions'][k, e, m, :2]), _raw(np.array([px, py])), err_msg=str((k, e, m)))
  assert_equal(rollout(eng, drawn['actions']), got, 'replay with capped draws')
  eng.close()


# ---------------------------------------------------------------------------------------------------------------------
def surface_case(n_envs=8):
  """9. BatchedEnvironment.rollout_random.  The engine class is environment._engine.Engine: the caller has patched the
  emulated one in, or runs on the GPU."""
  from spriteworld_amd import environment
  from tests._random_agent_cases import _surface_env
  env = _surface_env(n_envs)       # a noiseless SelectMove, three sprites, float64 actions
  env.reset()
  env.step(env.sample_actions())
  n_sprites = env.engine.S
  idx = torch.arange(n_envs, device=env.engine.device)
  for click in ('uniform', 'sprite'):
    env.seed_actions(4)
    r, actions = env.rollout_random(M, K, click=click)
    assert isinstance(r, environment.Rollout)
    for f in ('step_type', 'reward', 'discount', 'success'):
      assert tuple(getattr(r, f).shape) == (n_envs, M, K), f
    assert tuple(r.x.shape) == tuple(r.y.shape) == (n_envs, M, n_sprites) and tuple(r.n_sprites.shape) == tuple(r.error.shape) == (n_envs, M)
    assert (r.step_type.dtype, r.reward.dtype, r.discount.dtype, r.success.dtype) == (torch.uint8, torch.float64, torch.float32, torch.uint8)
    assert tuple(actions.shape) == (n_envs, M, K, 4) and actions.dtype == torch.float64 and actions.device == env.engine.device
    # (a click inside a sprite that has moved to the frame's edge may lie outside [0, 1), as the reference's does)
    assert ((actions[..., 2:] >= 0) & (actions[..., 2:] < 1)).all() and (click == 'sprite' or ((actions >= 0) & (actions < 1)).all())
    # the layout rollout() accepts: the same Rollout, bit for bit
    again = env.rollout(actions)
    for f in r._fields:
      np.testing.assert_array_equal(_raw(getattr(again, f).cpu().numpy()), _raw(getattr(r, f).cpu().numpy()), err_msg='%s %s' % (click, f))
    # seed_actions(s) reproduces it; the next call draws another key
    _, other = env.rollout_random(M, K, click=click)
    env.seed_actions(4)
    r2, actions2 = env.rollout_random(M, K, click=click)
    assert torch.equal(actions2, actions) and not torch.equal(other, actions)
    np.testing.assert_array_equal(_bits(r2.reward.cpu().numpy()), _bits(r.reward.cpu().numpy()))
  # execute the best plan's first step: the live batch returns what the rollout said (the action space is noiseless)
  best = r.episode_return().argmax(1)
  picked = env.rollout_frames(candidates=best)
  assert tuple(picked.shape) == (n_envs, 16, 16, 3) and picked.dtype == torch.uint8
  try:
    env.rollout_positions()
  except environment.EnvironmentError_ as e:
    assert 'kept no steps' in str(e)
  else:
    raise AssertionError('rollout_positions after a rollout_random that kept no steps did not raise')
  ts = env.step(actions[idx, best, 0])
  host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
  np.testing.assert_array_equal(host(ts.step_type), host(r.step_type[idx, best, 0]))
  np.testing.assert_array_equal(_bits(host(ts.reward).astype(np.float64)), _bits(host(r.reward[idx, best, 0])))
  assert (host(ts.step_type) != _abi.STEP_FIRST).all()
  # keep_steps: positions and frames per step
  r, actions = env.rollout_random(M, K, click='sprite', keep_steps=True)
  pos = env.rollout_positions()
  assert tuple(pos.x.shape) == (n_envs, M, K, n_sprites) and torch.equal(pos.x[:, :, K - 1], r.x)
  assert tuple(env.rollout_frames(step=1).shape) == (n_envs, M, 16, 16, 3)
  assert tuple(env.rollout_frames(candidates=best, step='all').shape) == (n_envs, K, 16, 16, 3)
  try:
    env.rollout_random(M, K, click='any')
  except ValueError as e:
    assert "click is 'uniform' or 'sprite'" in str(e)
  else:
    raise AssertionError("rollout_random(click='any') did not raise")
  env.close()


def offsets_case(n_envs=8):
  """9. global_env_offset is the kernel's first_env: two shards with one seed draw the two halves of the whole batch's streams."""
  from tests._random_agent_cases import _surface_env
  whole, lo, hi = _surface_env(n_envs), _surface_env(n_envs // 2), _surface_env(n_envs // 2, global_env_offset=n_envs // 2)
  out = []
  for env in (whole, lo, hi):
    env.reset()
    env.seed_actions(12)
    out.append(env.rollout_random(2, 2)[1].cpu().numpy())
    env.close()
  assert np.array_equal(out[0], np.concatenate([out[1], out[2]])) and not np.array_equal(out[1], out[2])


def groups_case(n_envs=8):
  """9. EnvironmentGroups (GPU: it owns HIP streams): the per-group form, on the group's stream; the groups draw different
  streams under one seed."""
  from spriteworld_amd import environment
  from tests._random_agent_cases import _surface_env
  groups = _surface_env(n_envs, cls=environment.EnvironmentGroups, num_groups=2)
  draws = []
  for g in range(2):
    groups.reset(g)
    groups.groups[g].seed_actions(12)
    r, actions = groups.rollout_random(g, M, 2, click='sprite')
    assert isinstance(r, environment.Rollout) and tuple(actions.shape) == (n_envs // 2, M, 2, 4)
    draws.append(actions)
  groups.synchronize()                                  # (a group's tensors are valid on the group's stream)
  draws = [a.cpu().numpy() for a in draws]
  groups.close()
  assert not np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[0][..., 2:], draws[1][..., 2:])
