"""Scenarios of swb_rollout_frames (the frames the candidate action sequences of a rollout end in), written against an engine
factory so that the emulated suite (tests/test_emulated_rollout_frames.py) and the GPU suite (tests/test_gpu_rollout_frames.py)
run the same checks.  Sizes are those of tests/_rollout_cases.py unless a case says otherwise.

The expected frame for [n, m] is a fresh oracle.Engine on the same cfg and pool, replayed through the live steps taken so far
and then through actions[:, :, m], the LAST step rendered; the bar is +-0 (tests/_parity.py).  The output buffer is filled
with 0x5A first, so that a byte never written shows.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np
import torch

from spriteworld_amd import _abi
from spriteworld_amd import workloads
from tests import _parity
from tests._rollout_cases import K, M, MAX_LEN, N_ENVS, T0, built, candidates, reference, rollout, started

ERR_INVALID, ERR_STATE = -1, -4
_bits = _parity.bits


def _violations(eng):
  """Reads outside a run list's own part and the arena since the last call, which only the emulated build counts."""
  if not hasattr(eng.lib, 'emu_violations'):
    return 0
  eng.lib.emu_violations.restype = C.c_long
  return eng.lib.emu_violations(1)


def _ptr(t):
  return None if t is None else C.c_void_p(t.data_ptr())


def raw_frames(eng, n_cand, cand=None, obs='new', error='new'):
  """(status, message, obs, error) of swb_rollout_frames called on the engine's handle as given: `cand` None or int values per
  environment; `obs` / `error`: 'new' (a buffer of the right shape, filled with 0x5A / zeros), a tensor, or None (NULL)."""
  lead = (eng.N,) if cand is not None else (eng.N, n_cand)
  if isinstance(obs, str):
    obs = torch.full(lead + tuple(eng.obs_shape), 0x5A, dtype=torch.uint8, device=eng.device)
  if isinstance(error, str):
    error = torch.zeros(lead, dtype=torch.uint8, device=eng.device)
  c = None if cand is None else torch.as_tensor(np.asarray(cand, dtype=np.int32), device=eng.device)
  rc = eng.lib.swb_rollout_frames(eng._h, int(n_cand), _ptr(c), _ptr(obs), _ptr(error), eng._stream())
  eng._sync()
  return rc, (eng.lib.swb_last_error().decode() if rc else ''), obs, error


def frames(eng, n_cand, cand=None):
  """The frames (numpy, [N, M, H, W, 3] or [N, H, W, 3]) of the last rollout; no error flag, no violation of the run lists."""
  rc, msg, obs, error = raw_frames(eng, n_cand, cand)
  assert rc == 0, msg
  assert not error.cpu().numpy().any(), 'error flags'
  assert _violations(eng) == 0
  return obs.cpu().numpy()


def reference_frames(cfg, pool, live, actions, reset_after_live=False):
  """The oracle's (frames [N, M, H, W, 3] after step K, step types [K, N, M]) for every candidate."""
  from oracle import oracle
  n_steps, n, n_cand, _ = actions.shape
  obs, step_type = None, np.zeros((n_steps, n, n_cand), np.uint8)
  for m in range(n_cand):
    ora = oracle.Engine(cfg, pool)
    for a in live:
      ora.step(a, render=False)
    if reset_after_live:
      ora.reset_all()
    for k in range(n_steps):
      out = ora.step(actions[k, :, m], render=(k == n_steps - 1))
      step_type[k, :, m] = out['step_type']
    assert not out['error'].any()
    if obs is None:
      obs = np.zeros((n, n_cand) + out['obs'].shape[1:], np.uint8)
    obs[:, m] = out['obs']
  return obs, step_type


def assert_frames_equal(got, want, what=''):
  assert got.shape == want.shape, (got.shape, want.shape, what)
  diff = got.astype(np.int16) != want.astype(np.int16)
  assert not diff.any(), ('frame diff', what, int(diff.sum()), np.argwhere(diff)[:5].tolist())


def start(make_engine, name, aa=2, rendered=0, seed=0, n_envs=N_ENVS):
  """(cfg, pool, sample, engine, the live actions it has taken, rng): the engine T0 live steps into workload `name`, the last
  `rendered` of them rendering.  anti_aliasing 2 is tests/_rollout_cases.started's; any other is built here the same way."""
  if aa == 2 and not rendered:
    out = started(make_engine, name, seed=seed, n_envs=n_envs)
    _violations(out[3])
    return out
  if aa == 2:
    cfg, pool, sample = built(name, n_envs=n_envs, seed=seed)
  else:
    cfg, pool, sample = workloads.build(name, n_envs, episodes_per_env=2, seed=seed, anti_aliasing=aa)
    cfg.max_episode_length = MAX_LEN
  eng = make_engine(cfg, pool)
  _violations(eng)
  rng = np.random.default_rng(seed + 100)
  live = [sample(rng) for _ in range(T0)]
  for t, a in enumerate(live):
    eng.step(a, render=(t >= T0 - rendered))
  return cfg, pool, sample, eng, live, rng


# ---------------------------------------------------------------------------------------------------------------------
# 1. every render route.  name -> (workload, anti_aliasing, SWB_* switches, what variant() must say)
ROUTES = {
    'tuned_goal_s5': ('goal_s5', 2, {}, {'large_frames': 0, 'many_sprites': 0, 'paint_in_cover': 0, 'vs': 6, 'nw': 4}),
    'tuned_cluster_s5': ('cluster_s5', 2, {}, {'large_frames': 0, 'many_sprites': 0, 'paint_in_cover': 0, 'nw': 4}),
    'wider_canvas_embodied_s12': ('embodied_s12', 2, {}, {'large_frames': 0, 'many_sprites': 0, 'paint_in_cover': 0}),
    'f64_drag': ('f64_drag', 2, {}, {'large_frames': 0, 'many_sprites': 0}),
    'position_keyed': ('pos:goal_x_lt_half', 2, {}, {'large_frames': 0, 'many_sprites': 0}),
    'painting_cover': ('goal_s5', 1, {}, {'large_frames': 0, 'paint_in_cover': 1, 'vs': 0, 'nw': 2}),
    'fill': ('geom_96x32', 1, {}, {'large_frames': 0, 'paint_in_cover': 0, 'vs': 0, 'n_column_groups': 2}),
    'many_sprites_ragged_s64': ('ragged_s64', 2, {}, {'large_frames': 1, 'many_sprites': 1}),
    'forced_large_frames': ('goal_s5', 2, {'SWB_LARGE_FRAMES': '1'}, {'large_frames': 1, 'many_sprites': 0}),
}


def route_case(make_engine, monkeypatch, route):
  """T0 = 3 live steps, then K = 6 with episodes of at most 4 steps: every candidate ends an episode and restarts from the pool
  inside the rollout; frames [n, m] of all candidates against the oracle, on the render route the handle takes."""
  name, aa, switches, expect = ROUTES[route]
  for k, v in switches.items():
    monkeypatch.setenv(k, v)
  cfg, pool, sample, eng, live, rng = start(make_engine, name, aa=aa)
  v = eng.variant()
  for k, value in expect.items():
    assert v[k] == value, (route, k, v)
  if route == 'wider_canvas_embodied_s12':
    assert v['nw'] > ROUTES['tuned_goal_s5'][3]['nw'] and cfg.max_sprites == 12, v
  acts = candidates(cfg, sample, rng, eng.state(), M, K)
  want, step_type = reference_frames(cfg, pool, live, acts)
  # coverage, from the oracle: the auto-reset happens inside the rollout, and the frames of some candidates of an environment differ
  assert (step_type[1:] == _abi.STEP_LAST).any() and (step_type[1:] == _abi.STEP_FIRST).any(), route
  assert any((want[n, 0] != want[n, m]).any() for n in range(cfg.n_envs) for m in range(1, M)), route
  if aa == 2 and not switches:      # (the rollout itself, where tests/_rollout_cases.reference applies as it stands)
    np.testing.assert_array_equal(reference(cfg, pool, live, acts)['step_type'], step_type)
  rollout(eng, acts)
  assert_frames_equal(frames(eng, M), want, route)
  eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. where the rollout ends
def ends_case(make_engine, n_steps, name='goal_s5', seed=0):
  """Episodes of at most 4 steps, three live steps.  K = 2: step K is LAST for a candidate, its frame shows the terminal
  sprites (render_only ignores reset_next).  K = 3: step K is FIRST, the frame shows the new episode.  Seed 0 gives both on
  goal_s5 (asserted on the oracle's step types)."""
  kind = {2: _abi.STEP_LAST, 3: _abi.STEP_FIRST}[n_steps]
  cfg, pool, sample, eng, live, rng = start(make_engine, name, seed=seed)
  acts = candidates(cfg, sample, rng, eng.state(), M, n_steps)
  want, step_type = reference_frames(cfg, pool, live, acts)
  assert (step_type[-1] == kind).any(), step_type[-1]
  rollout(eng, acts)
  got = frames(eng, M)
  assert_frames_equal(got, want, 'K = %d' % n_steps)
  if kind == _abi.STEP_FIRST:       # the fresh episode's frame does not depend on the candidate
    n = int(np.flatnonzero((step_type[-1] == kind).all(axis=1))[0])
    assert all((got[n, m] == got[n, 0]).all() for m in range(M))
  eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the handle is as it was
HANDLE = {'before_the_auto_trim': (1, False), 'after_the_auto_trim': (3, False), 'trim_straight_after': (1, True)}


def _same_state(a, b):
  for k in ('x', 'y'):
    np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)
  for k in ('n_sprites', 'pool_entry', 'step_count', 'reset_next', 'episode'):
    np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def handle_case(make_engine, which, name='goal_s5'):
  """state() bit-equal, a caller's marks in the sticky error buffer and the last step's frame in eng.obs survive, the launch
  count of step_time_ms() does not move; the next K real steps (rendering) equal the oracle, and real step K's frame equals
  frames[:, 0]: candidate 0 carries the live actions.  `rendered` live steps render before the call, so that it falls before
  (1) or after (3 = Engine.TRIM_AFTER) the engine's auto-trim; 'trim_straight_after' trims from the candidate scenes."""
  from oracle import oracle
  rendered, trim_after = HANDLE[which]
  cfg, pool, sample, eng, live, rng = start(make_engine, name, rendered=rendered)
  assert eng.TRIM_AFTER == 3 and eng._rendered == rendered
  ora = oracle.Engine(cfg, pool)
  for a in live:
    ora.step(a, render=False)
  acts = candidates(cfg, sample, rng, eng.state(), M, K)
  marks = (np.arange(cfg.n_envs) % 3 == 0).astype(np.uint8) * 0x40        # a caller's unread flags (no bit the engine sets)
  eng.error.copy_(torch.as_tensor(marks))
  eng.timing(True)
  before, obs_before, launches = eng.state(), eng.outputs_host()['obs'], eng.step_time_ms()[1]
  eng.rollout(acts)
  res = eng.rollout_frames()
  got = res['obs'].cpu().numpy()
  assert tuple(res['obs'].shape) == (cfg.n_envs, M) + tuple(eng.obs_shape) and not res['error'].cpu().numpy().any()
  if trim_after:
    assert eng.trim() > 0
  assert eng._rendered == rendered, 'rollout_frames counts as a rendering step of the auto-trim'
  assert eng.step_time_ms()[1] == launches, 'a counted step of swb_timing_enable'
  _same_state(eng.state(), before)
  host = eng.outputs_host()
  np.testing.assert_array_equal(host['error'], marks)
  np.testing.assert_array_equal(host['obs'], obs_before)
  eng.error.zero_()
  for k in range(K):
    a = acts[k, :, 0]
    want = ora.step(a)
    eng.step(a)
    out = eng.outputs_host()
    _parity.compare(k, ora, eng, want, out, what=which)
  assert eng.step_time_ms()[1] == launches + K
  assert_frames_equal(got[:, 0], out['obs'], 'candidate 0 against real step K')
  assert_frames_equal(got, reference_frames(cfg, pool, live, acts)[0], which)
  assert _violations(eng) == 0
  eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. picked candidates
def picked_case(make_engine, name='goal_s5'):
  """candidates = cand[N] equals the matching slices of the all-candidates result; -3 and M + 2 are clamped to 0 and M - 1;
  error has shape [N]."""
  cfg, pool, sample, eng, live, rng = start(make_engine, name)
  acts = candidates(cfg, sample, rng, eng.state(), M, K)
  rollout(eng, acts)
  every = frames(eng, M)
  assert_frames_equal(every, reference_frames(cfg, pool, live, acts)[0], 'all candidates')
  n = np.arange(cfg.n_envs)
  mixed = (n * 2 + 1) % M
  assert set(mixed) == set(range(M))
  assert_frames_equal(frames(eng, M, mixed), every[n, mixed], 'mixed')
  wild = np.where(n % 2 == 0, -3, M + 2)
  assert_frames_equal(frames(eng, M, wild), every[n, np.where(n % 2 == 0, 0, M - 1)], 'clamped')
  assert any((every[i, 0] != every[i, M - 1]).any() for i in n)
  rc, msg, obs, error = raw_frames(eng, M, mixed, error=torch.full((cfg.n_envs,), 0x40, dtype=torch.uint8, device=eng.device))
  assert rc == 0 and (error.cpu().numpy() == 0x40).all(), (rc, msg)          # ORed into: marks survive
  assert_frames_equal(frames(eng, M), every, 'all candidates again, after the picks')
  eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. edges
EDGES = ('one_candidate_one_step', 'sixty_four_candidates', 'five_environments', 'twice', 'scratch_grows', 'after_reset_all')


def edge_case(make_engine, which, name='goal_s5'):
  n_envs = 5 if which == 'five_environments' else N_ENVS      # (odd, fewer environments than a wave has lanes)
  cfg, pool, sample, eng, live, rng = start(make_engine, name, n_envs=n_envs)
  st = eng.state()
  if which == 'one_candidate_one_step':
    acts = candidates(cfg, sample, rng, st, 1, 1)
    rollout(eng, acts)
    assert_frames_equal(frames(eng, 1), reference_frames(cfg, pool, live, acts)[0], which)
  elif which == 'sixty_four_candidates':
    acts = candidates(cfg, sample, rng, st, 64, 1)
    rollout(eng, acts)
    assert_frames_equal(frames(eng, 64), reference_frames(cfg, pool, live, acts)[0], which)
  elif which == 'five_environments':
    acts = candidates(cfg, sample, rng, st, M, K)
    rollout(eng, acts)
    every = frames(eng, M)
    assert_frames_equal(every, reference_frames(cfg, pool, live, acts)[0], which)
    pick = np.arange(n_envs) % M
    assert_frames_equal(frames(eng, M, pick), every[np.arange(n_envs), pick], which + ' picked')
  elif which == 'twice':
    acts = candidates(cfg, sample, rng, st, M, K)
    rollout(eng, acts)
    first, second = frames(eng, M), frames(eng, M)
    assert_frames_equal(first, reference_frames(cfg, pool, live, acts)[0], which)
    assert_frames_equal(second, first, which + ': second call')
  elif which == 'scratch_grows':                # M = 2, then M = 5 (the scratch grows), then the frames of the second
    small, large = candidates(cfg, sample, rng, st, 2, K), candidates(cfg, sample, rng, st, 5, K)
    rollout(eng, small)
    assert_frames_equal(frames(eng, 2), reference_frames(cfg, pool, live, small)[0], which + ' M=2')
    rollout(eng, large)
    assert_frames_equal(frames(eng, 5), reference_frames(cfg, pool, live, large)[0], which + ' M=5')
  elif which == 'after_reset_all':              # K = 1 straight after reset_all: every frame is a FIRST frame
    eng.reset_all()
    acts = candidates(cfg, sample, rng, st, M, 1)
    want, step_type = reference_frames(cfg, pool, live, acts, reset_after_live=True)
    assert (step_type == _abi.STEP_FIRST).all()
    rollout(eng, acts)
    got = frames(eng, M)
    assert_frames_equal(got, want, which)
    assert all((got[:, m] == got[:, 0]).all() for m in range(M))
  else:
    raise ValueError(which)
  eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
def refusals_case(make_engine, name='goal_s5'):
  """Before any rollout: SWB_ERR_STATE; M mismatch and NULL obs: SWB_ERR_INVALID; after swb_set_pool: SWB_ERR_STATE until the
  next rollout; after a sprite setter: SWB_ERR_STATE; each with its message."""
  cfg, pool, sample, eng, live, rng = start(make_engine, name)
  rc, msg, _, _ = raw_frames(eng, M)
  assert rc == ERR_STATE and 'no rollout has run' in msg, (rc, msg)
  try:
    eng.rollout_frames()
    raise AssertionError('Engine.rollout_frames before any rollout did not raise')
  except AssertionError:
    raise
  except Exception as e:  # pylint: disable=broad-except
    assert 'no rollout has run' in str(e) and not isinstance(e, (ValueError, TypeError)), (type(e), e)
  acts = candidates(cfg, sample, rng, eng.state(), M, K)
  rollout(eng, acts)
  for n_cand in (M + 1, M - 1):
    rc, msg, _, _ = raw_frames(eng, n_cand)
    assert rc == ERR_INVALID and 'the last rollout of this handle had %d candidates' % M in msg, (rc, msg)
  rc, msg, _, _ = raw_frames(eng, M, obs=None)
  assert rc == ERR_INVALID and 'obs is NULL' in msg, (rc, msg)
  rc, msg, _, _ = raw_frames(eng, M, error=None)      # (accepted without an error buffer)
  assert rc == 0, msg
  eng.set_pool(pool)
  rc, msg, _, _ = raw_frames(eng, M)
  assert rc == ERR_STATE and 'pool has changed' in msg and 'swb_set_pool' in msg, (rc, msg)
  for a in live:
    eng.step(a, render=False)
  rollout(eng, acts)
  assert_frames_equal(frames(eng, M), reference_frames(cfg, pool, live, acts)[0], 'after a new pool and a new rollout')
  env = int(np.flatnonzero(eng.state()['reset_next'] == 0)[0])
  eng.set_sprite_attr(env, 0, _abi.ATTR_ANGLE, 45.0)
  rc, msg, _, _ = raw_frames(eng, M)
  assert rc == ERR_STATE and 'sprite setters' in msg and 'not supported' in msg, (rc, msg)
  eng.close()


def refusals_after_device_sampling_case(case='hsv_mixed', n_envs=N_ENVS):
  """swb_sample_pool (refill_pool) and swb_resample_pool (refresh_pool) invalidate the scratch: SWB_ERR_STATE until the next
  rollout.  A device-sampled workload of tests/_sampler_cases.py; the engine class is environment._engine.Engine: the caller has
  patched the emulated one in, or runs on the GPU."""
  from tests import _sampler_cases
  env, _, _, _ = _sampler_cases.make_env(case, num_envs=n_envs, episodes_per_env=2)
  eng = env.engine
  env.reset()
  acts = np.random.default_rng(3).uniform(0.0, 1.0, size=(n_envs, M, 2, 4))
  for redraw, call in ((env.refill_pool, 'swb_sample_pool'), (env.refresh_pool, 'swb_resample_pool')):
    env.rollout(acts)
    first = env.rollout_frames()
    assert tuple(first.shape) == (n_envs, M) + tuple(eng.obs_shape)
    redraw()
    rc, msg, _, _ = raw_frames(eng, M)
    assert rc == ERR_STATE and 'pool has changed' in msg and call in msg, (call, rc, msg)
    try:
      env.rollout_frames()
      raise AssertionError('rollout_frames after %s did not raise' % call)
    except AssertionError:
      raise
    except Exception as e:  # pylint: disable=broad-except
      assert 'pool has changed' in str(e), e
    env.reset()
  env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the Python surface
def surface_case(n_envs=N_ENVS):
  """BatchedEnvironment.rollout followed by rollout_frames() and rollout_frames(candidates=argmax) on the environment of
  tests/_rollout_cases.surface_case: shapes, dtype, device, equality with Engine.rollout_frames, and an exception before any
  rollout.  The engine class is environment._engine.Engine: the caller has patched the emulated one in, or runs on the GPU."""
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
  try:
    env.rollout_frames()
    raise AssertionError('rollout_frames before any rollout did not raise')
  except AssertionError:
    raise
  except Exception as e:  # pylint: disable=broad-except
    assert 'no rollout has run' in str(e), e
  cfg, pool = eng.cfg, eng.get_pool()
  a = np.random.default_rng(8).uniform(0.0, 1.0, size=(n_envs, M, K, 4))      # the planner's layout
  st = env.state()
  a[:, 1, 0, 0], a[:, 1, 0, 1] = st['x'][:, 0], st['y'][:, 0]
  r = env.rollout(torch.as_tensor(a))
  every = env.rollout_frames()
  assert tuple(every.shape) == (n_envs, M, 16, 16, 3) and every.dtype == torch.uint8 and every.device == eng.device
  best = r.episode_return().argmax(1).int()
  one = env.rollout_frames(candidates=best)
  assert tuple(one.shape) == (n_envs, 16, 16, 3) and one.dtype == torch.uint8 and one.device == eng.device
  assert torch.equal(one, every[torch.arange(n_envs, device=eng.device), best.long()])
  direct = eng.rollout_frames()
  assert sorted(direct) == ['error', 'obs'] and torch.equal(direct['obs'], every)
  assert tuple(direct['error'].shape) == (n_envs, M) and direct['error'].dtype == torch.uint8 and not direct['error'].any()
  picked = eng.rollout_frames(best.cpu().numpy().astype(np.int64))      # (an array of another integer type)
  assert torch.equal(picked['obs'], one) and tuple(picked['error'].shape) == (n_envs,)
  for bad in (np.zeros(n_envs + 1, np.int32), np.zeros((n_envs, 1), np.int32), np.zeros(n_envs)):
    try:
      eng.rollout_frames(bad)
      raise AssertionError('accepted candidates %s %s' % (bad.dtype, bad.shape))
    except ValueError as e:
      assert 'rollout_frames candidates must be' in str(e)
  # against the oracle: reset() was one live step (FIRST, its action unused); the rollout is of the noiseless dynamics
  kn = np.ascontiguousarray(a.transpose(2, 0, 1, 3))
  want, step_type = reference_frames(cfg, pool, [np.zeros((n_envs, 4))], kn)
  assert_frames_equal(every.cpu().numpy(), want, 'BatchedEnvironment.rollout_frames')
  assert (step_type == _abi.STEP_LAST).any()
  env.close()
