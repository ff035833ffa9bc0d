"""Scenarios of swb_sample_actions (random-agent actions drawn on the device, clicks on sprites included), written against an
engine factory so that the emulated suite (tests/test_emulated_random_agent.py) and the GPU suite
(tests/test_gpu_random_agent.py) run the same checks.

The reference value is tests/_random_agent_model.py (the Philox stream and the draw order restated, geometry and containment
from the oracle) fed with an oracle.Engine stepped alongside the engine under test: actions, positions, sprites and tries are
compared bit for bit.  TEST INFRASTRUCTURE ONLY."""
import contextlib
import ctypes as C
import math
import os

import numpy as np

from spriteworld_amd import _abi
from spriteworld_amd import shapes
from spriteworld_amd import workloads
from tests import _parity
from tests import _random_agent_model as model
from tests import _util

N_ENVS, MAX_LEN = 16, 3
UNIFORM, ON_SPRITE = _abi.SAMPLE_UNIFORM, _abi.SAMPLE_ON_SPRITE
ALL = ('actions', 'position', 'sprite', 'tries')
# a tries count "far below the cap": the worst shipped acceptance rate is 0.3536 (star_4 over its bounding box), so a draw
# needs more than 64 tries with probability 0.6464^64 < 1e-12 -- per draw, on any of these inputs
FAR_BELOW_CAP = 64
# the workloads of model_case; '+many_sprites_forced': the handle is created under SWB_MANY_SPRITES=1 (swb_ms_state_kernel's path)
MODEL = ('goal_s5', 'embodied_s12', 'meta_s24_f64', 'meta_s24_f64+many_sprites_forced', 'goal_s5+many_sprites_forced', 'cluster_s5_f32a',
         'shapes_64', 'ragged_s16', 'ragged_s64', 'ragged_s64_embodied', 'f64_drag')


@contextlib.contextmanager
def _environ(**kw):
  old = {k: os.environ.get(k) for k in kw}
  os.environ.update(kw)
  try:
    yield
  finally:
    for k, v in old.items():
      if v is None:
        del os.environ[k]
      else:
        os.environ[k] = v


def built(name, n_envs=N_ENVS, seed=0, max_len=MAX_LEN, tweak=None):
  """(cfg, pool, sample) with episodes of at most `max_len` steps.  'shapes_64': five sprites drawn from star_4, the circle
  (30 vertices) and a 64-gon uploaded in the octagon's place (the last lane of the path and of the ballot), at many angles."""
  if name == 'shapes_64':
    cfg, pool, sample = workloads.build('goal_s5', n_envs, episodes_per_env=2, seed=seed, anti_aliasing=2)
    rng = np.random.default_rng(seed + 7)
    ids = np.array([shapes.shape_index(s) for s in ('star_4', 'circle', 'octagon')], np.int32)
    pool.shape[:] = ids[rng.integers(0, 3, size=pool.shape.shape)]
    pool.shape[:, 0] = ids[2]
    pool.angle[:] = rng.integers(0, 360, size=pool.angle.shape).astype(np.float64)
    for idx in np.ndindex(pool.angle.shape):       # (math.cos(math.radians()) as lowering computes them)
      th = math.radians(pool.angle[idx])
      pool.cos_a[idx], pool.sin_a[idx] = math.cos(th), math.sin(th)
    pool.scale[:] = rng.choice([0.08, 0.13, 0.2], size=pool.scale.shape)
  else:
    cfg, pool, sample = workloads.build(name, n_envs, episodes_per_env=2, seed=seed, anti_aliasing=2)
  cfg.max_episode_length = max_len
  if tweak:
    tweak(cfg, pool)
  return cfg, pool, sample


@contextlib.contextmanager
def started(make_engine, name, steps=MAX_LEN, seed=0, n_envs=N_ENVS, tweak=None):
  """(cfg, oracle engine, engine, sample, rng): both `steps` live steps into workload `name` (no frames)."""
  from oracle import oracle
  name, _, forced = name.partition('+')
  shape_ctx = _util.swapped_shape('octagon', shapes.polygon(64)) if name == 'shapes_64' else contextlib.nullcontext()
  with shape_ctx:
    cfg, pool, sample = built(name, n_envs=n_envs, seed=seed, tweak=tweak)
    with (_environ(SWB_MANY_SPRITES='1') if forced else contextlib.nullcontext()):
      eng = make_engine(cfg, pool)
    if forced:
      assert eng.variant()['many_sprites'] == 1
    ora = oracle.Engine(cfg, pool)
    rng = np.random.default_rng(seed + 100)
    live(ora, eng, sample, rng, steps)
    try:
      yield cfg, ora, eng, sample, rng
    finally:
      eng.close()


def live(ora, eng, sample, rng, steps):
  for _ in range(steps):
    a = sample(rng)
    ora.step(a, render=False)
    eng.step(a, render=False)


def draw(eng, mode, seed, first_env=0, outputs=None):
  """Engine.sample_actions of the engine under test -> dict of numpy arrays."""
  outputs = outputs or (ALL if mode == ON_SPRITE else ('actions',))
  return {k: v.cpu().numpy() for k, v in eng.sample_actions(mode, seed, first_env=first_env, outputs=outputs).items()}


def _raw(a):
  a = np.ascontiguousarray(a)
  return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def assert_same(got, want, what=''):
  assert sorted(got) == sorted(want), (sorted(got), sorted(want))
  for k in want:
    assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, want[k].dtype, got[k].shape, want[k].shape)
    np.testing.assert_array_equal(_raw(got[k]), _raw(want[k]), err_msg='%s %s' % (k, what))


def differs(a, b):
  return any((_raw(a[k]) != _raw(b[k])).any() for k in a)


def assert_same_state(eng, ora):
  a, b = eng.state(), ora.state()
  for k in ('x', 'y'):
    np.testing.assert_array_equal(_parity.bits(a[k]), _parity.bits(b[k]), err_msg=k)
  for k in ('n_sprites', 'pool_entry', 'step_count', 'reset_next', 'episode'):
    np.testing.assert_array_equal(a[k], b[k], err_msg=k)
  return b


# ---------------------------------------------------------------------------------------------------------------------
def model_case(make_engine, name):
  """2. Both modes against the model, bit for bit, at two moments: MAX_LEN live steps in (episodes running) and one step
  later (every episode that ran its full length sits on reset_next and keeps its terminal sprites)."""
  with started(make_engine, name) as (cfg, ora, eng, sample, rng):
    seen_reset, seen_running, most, chosen = False, False, 0, []
    for moment in range(2):
      st = assert_same_state(eng, ora)
      seen_reset |= bool(st['reset_next'].any())
      seen_running |= bool((st['reset_next'] == 0).any())
      most = max(most, int(st['n_sprites'].max()))
      for mode in (UNIFORM, ON_SPRITE):
        seed, first = 0x9E3779B97F4A7C15 ^ (moment * 77 + mode), 5 * moment
        want = model.sample_batch(seed, first, mode, cfg, ora, st)
        if mode == ON_SPRITE:      # the condition on tries is the reference's: asserted on the model alone first
          has = st['n_sprites'] > 0
          assert (want['tries'][has] >= 1).all() and (want['tries'][has] <= FAR_BELOW_CAP).all(), want['tries']
          assert (want['tries'][~has] == 0).all() and (want['sprite'][~has] == -1).all()
          assert ((want['sprite'][has] >= 0) & (want['sprite'][has] < st['n_sprites'][has])).all()
          chosen += want['sprite'].tolist()
        assert_same(draw(eng, mode, seed, first), want, '%s mode %d moment %d' % (name, mode, moment))
      assert_same_state(eng, ora)                       # (sampling moved nothing)
      live(ora, eng, sample, rng, 1)
    assert seen_reset and seen_running, name
    base = name.partition('+')[0]
    if base == 'meta_s24_f64':
      assert max(chosen) > 16 and eng.variant()['many_sprites'] == 1, chosen
      assert cfg.pos_is_f32 == 0
    if base.startswith('ragged'):
      assert -1 in chosen and len(set(chosen)) > 4, chosen          # an environment without sprites, and ragged counts
    if base == 'cluster_s5_f32a':
      assert cfg.action_is_f32 == 1


def shapes_64_coverage_case(make_engine):
  """... and the shapes_64 scene really draws on the 64-gon (sprite 0 of every episode), the circle and star_4."""
  with started(make_engine, 'shapes_64') as (cfg, ora, eng, sample, rng):
    st = ora.state()
    seen = set()
    for k in range(6):
      want = model.sample_batch(1000 + k, 0, ON_SPRITE, cfg, ora, st)
      assert_same(draw(eng, ON_SPRITE, 1000 + k), want, 'shapes_64 draw %d' % k)
      for e, s in enumerate(want['sprite']):
        sp = ora.get_sprite(e, int(s))
        seen.add((sp['shape'], len(sp['path'])))
    names = {shapes.SHAPE_NAMES[s]: nv for s, nv in seen}
    assert names == {'star_4': 8, 'circle': 30, 'octagon': 64}, names


def setters_case(make_engine, zero_scale=False):
  """3. set_sprite_attr (angle, scale, shape) on a few sprites: the sampled positions follow the overridden paths -- the model
  fed by oracle.Engine.get_sprite.  7. zero_scale (the emulator only): the sprites of one environment, scaled to nothing, are
  never hit: tries = -1 and the sprite's own position; the other environments are unaffected."""
  with started(make_engine, 'goal_s5', steps=2) as (cfg, ora, eng, sample, rng):
    st = ora.state()
    assert not st['reset_next'].any()
    star = float(shapes.shape_index('star_5'))
    calls = [(1, 0, _abi.ATTR_ANGLE, 33.0), (1, 0, _abi.ATTR_SCALE, 0.3), (2, 3, _abi.ATTR_SHAPE, star), (2, 3, _abi.ATTR_ANGLE, 133.5),
             (4, 1, _abi.ATTR_SCALE, 0.05), (4, 2, _abi.ATTR_SHAPE, star), (7, 4, _abi.ATTR_ANGLE, 270.0)]
    for env, k, attr, value in calls:
      ora.set_sprite_attr(env, k, attr, value)
      eng.set_sprite_attr(env, k, attr, value)
    if zero_scale:      # sprite.py:171-175 scales the path by (s - _scale): assigning a sprite its own scale collapses it to a point
      for k in range(5):
        own = ora.get_sprite(9, k)['scale']
        ora.set_sprite_attr(9, k, _abi.ATTR_SCALE, own, delta=0.0)
        eng.set_sprite_attr(9, k, _abi.ATTR_SCALE, own, delta=0.0)
        assert not ora.get_sprite(9, k)['path'].any()
    touched = sorted({c[0] for c in calls} | ({9} if zero_scale else set()))
    hits = set()
    for k in range(8):
      want = model.sample_batch(50 + k, 3, ON_SPRITE, cfg, ora, st)
      got = draw(eng, ON_SPRITE, 50 + k, 3)
      assert_same(got, want, 'setters draw %d' % k)
      hits |= {(e, int(want['sprite'][e])) for e in touched}
      if zero_scale:
        assert got['tries'][9] == -1
        assert np.array_equal(got['position'][9], [st['x'][9, got['sprite'][9]], st['y'][9, got['sprite'][9]]])
        others = np.arange(cfg.n_envs) != 9
        assert (got['tries'][others] >= 1).all() and (got['tries'][others] <= FAR_BELOW_CAP).all()
    # the draws visited overridden sprites, and their paths are not the pool's any more
    assert {(1, 0), (2, 3)} & hits, hits
    incremental = [s for s in model.oracle_sprites(ora, 1, 5, st['x'], st['y']) if not s['fresh']]
    assert incremental, 'no sprite carries an incrementally transformed path'
    # one live step later the episodes go on with their overrides; an environment that resets drops them
    live(ora, eng, sample, rng, 1)
    st = assert_same_state(eng, ora)
    assert_same(draw(eng, ON_SPRITE, 99), model.sample_batch(99, 0, ON_SPRITE, cfg, ora, st), 'setters, a step later')


def read_only_case(make_engine, name='goal_s5', steps=6):
  """4. Sampling calls between the steps of a tests/_parity.compare run: state, outputs, frames (+-0) and error flags stay
  bit-exact through every step; the same seed returns the same bits, another seed or first_env other bits, and first_env = k
  on environment n is the model's entry n + k."""
  from oracle import oracle
  cfg, pool, sample = built(name, n_envs=8, max_len=4)
  ora, eng = oracle.Engine(cfg, pool), make_engine(cfg, pool)
  rng = np.random.default_rng(3)
  marks = (np.arange(cfg.n_envs) % 3 == 0).astype(np.uint8) * 0x40          # a caller's unread flags (no bit the engine sets)
  import torch
  for t in range(steps):
    a = sample(rng)
    want = ora.step(a)
    eng.step(a)
    out = eng.outputs_host()
    st = _parity.compare(t, ora, eng, want, out)
    eng.error.copy_(torch.as_tensor(marks))
    first = draw(eng, ON_SPRITE, 11 + t, 2)
    uniform = draw(eng, UNIFORM, 11 + t, 2)
    assert_same(draw(eng, ON_SPRITE, 11 + t, 2), first, 'same seed, t=%d' % t)
    assert_same(draw(eng, UNIFORM, 11 + t, 2), uniform, 'same seed, t=%d' % t)
    assert differs(draw(eng, ON_SPRITE, 12 + t, 2), first) and differs(draw(eng, UNIFORM, 12 + t, 2), uniform)
    assert differs(draw(eng, ON_SPRITE, 11 + t, 3), first) and differs(draw(eng, UNIFORM, 11 + t, 3), uniform)
    assert_same(first, model.sample_batch(11 + t, 2, ON_SPRITE, cfg, ora, st), 'first_env = 2, t=%d' % t)
    far = draw(eng, UNIFORM, 11 + t, (1 << 40) + 9)                         # (the high word of the entry)
    assert_same(far, model.sample_batch(11 + t, (1 << 40) + 9, UNIFORM, cfg, ora, st), 'first_env = 2^40 + 9')
    # nothing of the handle moved: state, the last step's outputs (frame included), the error buffer
    assert_same_state(eng, ora)
    after = eng.outputs_host()
    for k in out:
      if k != 'error':
        np.testing.assert_array_equal(_raw(after[k]), _raw(out[k]), err_msg='%s after sampling, t=%d' % (k, t))
    np.testing.assert_array_equal(after['error'], marks)
    eng.error.zero_()
  eng.close()


def containment_case(make_engine, name='f64_cluster'):
  """5. Independent of the model, on a float64 SelectMove handle with float64 positions: oracle.contains_point holds for every
  (sprite, position); stepping with the sampled actions matches the oracle's step and moves a sprite in every environment that
  is not resetting and whose motion is non-zero (the workload's velocities are zeroed: only a hit moves anything)."""
  from oracle import oracle

  def still(cfg, pool):
    pool.x_vel[:] = 0.0
    pool.y_vel[:] = 0.0

  with started(make_engine, name, steps=2, tweak=still) as (cfg, ora, eng, sample, rng):
    assert cfg.action_is_f32 == 0 and cfg.action_space != _abi.ACTION_EMBODIED
    moved_any = 0
    for t in range(4):
      st = ora.state()
      got = draw(eng, ON_SPRITE, 700 + t)
      for e in range(cfg.n_envs):
        s = int(got['sprite'][e])
        assert 0 <= s < st['n_sprites'][e] and got['tries'][e] >= 1
        sp = ora.get_sprite(e, s)
        px, py = got['position'][e]
        assert oracle.contains_point(sp['shape'], sp['scale'], sp['angle'], px - st['x'][e, s], py - st['y'][e, s]), (t, e, s)
      np.testing.assert_array_equal(_raw(got['actions'][:, :2]), _raw(got['position']))
      a = got['actions']
      want = ora.step(a, render=False)
      eng.step(a, render=False)
      out = eng.outputs_host()
      np.testing.assert_array_equal(out['step_type'], want['step_type'])
      _parity.assert_rewards_equal(out['reward'], want['reward'], 't=%d' % t)
      after = assert_same_state(eng, ora)
      if cfg.action_space == _abi.ACTION_DRAG_AND_DROP:
        motion = (a[:, 2:] - a[:, :2]) * cfg.action_scale
      else:
        motion = (a[:, 2:] - 0.5) * cfg.action_scale
      expect = (st['reset_next'] == 0) & (np.abs(motion).sum(axis=1) > 0)
      moved = ((_parity.bits(after['x']) != _parity.bits(st['x'])) | (_parity.bits(after['y']) != _parity.bits(st['y']))).any(axis=1)
      assert moved[expect].all(), (t, np.flatnonzero(expect & ~moved))
      moved_any += int(expect.sum())
    assert moved_any > cfg.n_envs


def raw_call(eng, mode, seed=1, first_env=0, **outs):
  """(status, message) of swb_sample_actions called on the engine's handle with the given output tensors (others NULL)."""
  o = _abi.SwbSampledActions()
  for k, t in outs.items():
    setattr(o, k, t.data_ptr())
  rc = eng.lib.swb_sample_actions(eng._h, int(mode), C.c_uint64(seed), C.c_uint64(first_env), C.byref(o), eng._stream())
  return rc, eng.lib.swb_last_error().decode() if rc else ''


def refusals_case(make_engine, name='goal_s5'):
  """6. Unknown mode, every output NULL, and position / sprite / tries with SWB_SAMPLE_UNIFORM: SWB_ERR_INVALID with a message;
  any single output alone is accepted."""
  import torch
  with started(make_engine, name, steps=1) as (cfg, ora, eng, sample, rng):
    new = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=eng.device)
    bufs = {'actions': new((cfg.n_envs, 4), torch.float64), 'position': new((cfg.n_envs, 2), torch.float64),
            'sprite': new((cfg.n_envs,), torch.int32), 'tries': new((cfg.n_envs,), torch.int32)}
    for mode in (2, -1, 77):
      rc, msg = raw_call(eng, mode, **bufs)
      assert rc == -1 and 'unknown mode' in msg, (mode, rc, msg)
    for mode in (UNIFORM, ON_SPRITE):
      rc, msg = raw_call(eng, mode)
      assert rc == -1 and 'every output is NULL' in msg, (rc, msg)
    rc = eng.lib.swb_sample_actions(eng._h, UNIFORM, C.c_uint64(1), C.c_uint64(0), None, eng._stream())
    assert rc == -1
    for k in ('position', 'sprite', 'tries'):
      rc, msg = raw_call(eng, UNIFORM, actions=bufs['actions'], **{k: bufs[k]})
      assert rc == -1 and 'SWB_SAMPLE_ON_SPRITE only' in msg, (k, rc, msg)
      rc, msg = raw_call(eng, ON_SPRITE, **{k: bufs[k]})            # alone, in its own mode
      assert rc == 0, (k, msg)
    whole = draw(eng, ON_SPRITE, 1)
    eng._sync()
    for k in ('position', 'sprite', 'tries'):
      np.testing.assert_array_equal(_raw(bufs[k].cpu().numpy()), _raw(whole[k]), err_msg=k)
    try:
      eng.sample_actions(UNIFORM, 1, outputs=('actions', 'sprites'))
    except ValueError:
      pass
    else:
      raise AssertionError('an unknown output name was accepted')
    assert not differs({'e': eng.outputs_host()['error']}, {'e': np.zeros(cfg.n_envs, np.uint8)})


def _surface_env(n_envs, action_space=None, **kw):
  from spriteworld_amd import action_spaces, environment, renderers, sprite_generators, tasks
  from spriteworld_amd import factor_distributions as distribs
  factors = distribs.Product([
      distribs.Continuous('x', 0.1, 0.9), distribs.Continuous('y', 0.1, 0.9),
      distribs.Discrete('shape', ['square', 'triangle', 'star_4']), distribs.Discrete('scale', [0.15]),
      distribs.Continuous('c0', 0., 1.), distribs.Continuous('c1', 0.3, 1.), distribs.Continuous('c2', 0.9, 1.)])
  rend = {'image': renderers.PILRenderer(image_size=(16, 16), anti_aliasing=1, color_to_rgb=renderers.color_maps.hsv_to_rgb)}
  make = kw.pop('cls', environment.BatchedEnvironment)
  return make(task=tasks.FindGoalPosition(filter_distrib=None, goal_position=(3., 3.), terminate_distance=0.01),
              action_space=action_space or action_spaces.SelectMove(scale=0.25), renderers=rend,
              init_sprites=sprite_generators.generate_sprites(factors, num_sprites=3), max_episode_length=10, num_envs=n_envs,
              episodes_per_env=2, seed=5, **kw)


def surface_case(n_envs=8):
  """6. The Python surface.  The engine class is environment._engine.Engine: the caller has patched the emulated one in, or
  runs on the GPU."""
  import torch
  from spriteworld_amd import action_spaces, environment
  env = _surface_env(n_envs)
  env.reset()
  # no arguments: host numpy, float64, the values of action_space.sample under the same np.random.seed -- as before
  np.random.seed(21)
  host = env.sample_actions()
  np.random.seed(21)
  again = env.sample_actions(where='host', click='uniform')
  np.random.seed(21)
  direct = env.action_space.sample(n_envs)
  np.random.seed(21)
  as_before = np.random.uniform(0., 1., size=(n_envs, 4))                  # what action_spaces.SelectMove.sample(n) has always drawn
  assert isinstance(host, np.ndarray) and host.dtype == np.float64 and host.shape == (n_envs, 4)
  assert np.array_equal(host, again) and np.array_equal(host, direct) and np.array_equal(host, as_before)
  for bad in (dict(click='sprite'), dict(where='host', click='sprite'), dict(where='gpu'), dict(where='device', click='any')):
    try:
      env.sample_actions(**bad)
    except ValueError:
      pass
    else:
      raise AssertionError('sample_actions(%r) did not raise' % bad)
  # the device forms: a tensor step() takes as it is
  dev = env.engine.device
  for click in ('uniform', 'sprite'):
    a = env.sample_actions(where='device', click=click)
    assert isinstance(a, torch.Tensor) and a.device == dev and a.dtype == torch.float64 and tuple(a.shape) == (n_envs, 4)
    assert ((a >= 0) & (a < 1)).all()
    ts = env.step(a)
    assert env.engine._last_actions is a                                    # (no copy, no conversion)
    assert tuple(ts.step_type.shape) == (n_envs,)
  # sample_contained_positions(): shapes, dtypes, and positions inside the chosen sprites
  from oracle import oracle
  cp = env.sample_contained_positions()
  assert isinstance(cp, environment.ContainedPositions) and cp._fields == ('position', 'sprite', 'tries')
  assert (cp.position.dtype, cp.sprite.dtype, cp.tries.dtype) == (torch.float64, torch.int32, torch.int32)
  assert tuple(cp.position.shape) == (n_envs, 2) and tuple(cp.sprite.shape) == tuple(cp.tries.shape) == (n_envs,)
  st = env.state()
  pos, spr = cp.position.cpu().numpy(), cp.sprite.cpu().numpy()
  assert (cp.tries.cpu().numpy() >= 1).all()
  for e in range(n_envs):
    sp = env.engine.get_sprite(e, int(spr[e]))
    assert oracle.contains_point(sp['shape'], sp['scale'], sp['angle'], pos[e, 0] - st['x'][e, spr[e]], pos[e, 1] - st['y'][e, spr[e]])
  # seed_actions: the same seed replays the same calls, call k differs from call k + 1, another seed differs
  def three(seed):
    env.seed_actions(seed)
    return [env.sample_actions(where='device', click='sprite').cpu().numpy(), env.sample_actions(where='device').cpu().numpy(),
            env.sample_contained_positions().position.cpu().numpy()]
  a, b, c = three(4), three(4), three(5)
  # ... and its keys are not the reset sampler's under the same seed (the kernels share the Philox counter layout)
  from spriteworld_amd import device_sampler
  reset_keys = device_sampler.DeviceSampler.__new__(device_sampler.DeviceSampler)
  reset_keys.seed, reset_keys._draws = 4, 0
  env.seed_actions(4)
  assert not {env._next_action_seed() for _ in range(8)} & {reset_keys.next_seed() for _ in range(8)}
  assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not any(np.array_equal(x, y) for x, y in zip(a, c))
  assert not np.array_equal(a[0][:, 2:], a[1][:, 2:])
  # unseeded: the base seed comes from numpy's global stream, once, at the first device call
  fresh = []
  for _ in range(2):
    other = _surface_env(n_envs)
    other.reset()
    np.random.seed(9)
    fresh.append(other.sample_actions(where='device').cpu().numpy())
    state = np.random.get_state()[1].copy()
    other.sample_actions(where='device')
    assert np.array_equal(np.random.get_state()[1], state)                  # (no further draw from numpy)
    other.close()
  assert np.array_equal(fresh[0], fresh[1])
  env.close()
  # an Embodied environment: integer actions
  emb = _surface_env(4, action_space=action_spaces.Embodied(step_size=0.1))
  emb.reset()
  a = emb.sample_actions(where='device', click='sprite')
  assert a.dtype == torch.int32 and tuple(a.shape) == (4, 2) and ((a[:, 0] >= 0) & (a[:, 0] < 2) & (a[:, 1] >= 0) & (a[:, 1] < 4)).all()
  emb.step(a)
  emb.close()


def offsets_case(n_envs=8):
  """6. global_env_offset is the kernel's first_env: two shards with one seed draw the two halves of the whole batch's
  streams, never each other's."""
  whole, lo, hi = _surface_env(n_envs), _surface_env(n_envs // 2), _surface_env(n_envs // 2, global_env_offset=n_envs // 2)
  out = []
  for env in (whole, lo, hi):
    env.reset()
    env.seed_actions(12)
    out.append(env.sample_actions(where='device').cpu().numpy())
    env.close()
  assert np.array_equal(out[0], np.concatenate([out[1], out[2]])) and not np.array_equal(out[1], out[2])


def groups_case(n_envs=8):
  """6. EnvironmentGroups (GPU: it owns HIP streams): the groups draw different streams under one seed."""
  from spriteworld_amd import environment
  groups = _surface_env(n_envs, cls=environment.EnvironmentGroups, num_groups=2)
  draws = []
  for g in range(2):
    groups.reset(g)
    groups.groups[g].seed_actions(12)
    draws.append(groups.sample_actions(g, where='device', click='sprite'))
  groups.synchronize()                                  # (a group's tensors are valid on the group's stream)
  draws = [a.cpu().numpy() for a in draws]
  groups.close()
  assert draws[0].shape == draws[1].shape == (n_envs // 2, 4) and not np.array_equal(draws[0], draws[1])
  assert not np.array_equal(draws[0][:, 2:], draws[1][:, 2:])
