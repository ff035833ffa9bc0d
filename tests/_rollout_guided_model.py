"""Pure-Python restatement of swb_rollout_guided's draws (rollout_guided_drawer, spriteworld_amd/csrc/swb_sampler.hip.inc).

Test infrastructure.  It is tests/_rollout_random_model.py with the draw order of swb_rollout_guided (include/swb.h): the
stream per virtual environment is that module's `CandidateStream`, the bounding-box arithmetic and the containment test are
tests/_random_agent_model.py's (geometry and containment from the oracle), the walk is one oracle.Engine per candidate stepped
with the actions drawn so far.  What is added: the choice of the sprite from the running sums of a plan's row, and the motion --
Python floats are IEEE doubles and every operation below rounds once, as __dadd_rn / __dmul_rn / __dsub_rn do.
"""
import math

import numpy as np

from spriteworld_amd import _abi
from tests import _random_agent_model
from tests._rollout_random_model import CandidateStream, _uniforms

SQRT3 = 1.7320508075688772
# how a sprite (Embodied: an action index) was chosen
NO_SPRITE, FALLBACK_NO_CDF, FALLBACK_TOTAL, WEIGHTED, WEIGHTED_ROUNDED_UP = 0, 1, 2, 3, 4


def irwin_hall_z(rng):
  """z of one motion component: four uniforms of the stream, (((u1 + u2) + (u3 + u4)) - 2) * sqrt(3)."""
  u1, u2, u3, u4 = rng.uniform(), rng.uniform(), rng.uniform(), rng.uniform()
  return (((u1 + u2) + (u3 + u4)) - 2.0) * SQRT3


def choose(u_c, n, cdf_row, width):
  """Rule 3 of swb_rollout_guided: (index, how) among `n` choices from the running sums `cdf_row` (None: no cdf) of `width`."""
  uniform = min(int(u_c * n), n - 1)
  if cdf_row is None:
    return uniform, FALLBACK_NO_CDF
  wp = min(n, width)
  total = float(cdf_row[wp - 1])
  if not (math.isfinite(total) and total > 0.0):
    return uniform, FALLBACK_TOTAL
  t = u_c * total
  for j in range(wp):
    if float(cdf_row[j]) > t:
      return j, WEIGHTED
  for j in range(wp):
    if float(cdf_row[j]) >= total:
      return j, WEIGHTED_ROUNDED_UP
  raise AssertionError('no running sum reaches the total')


def clip01(v):
  return (v if v < 1.0 else 1.0) if v > 0.0 else 0.0


def draw_step(rng, cfg, sprites, cdf_row, width, mean, std):
  """One step's draw of one virtual environment from its running stream: dict(actions, sprite, tries, how, u_c, z, v).
  sprites: tests/_random_agent_model.oracle_sprites (None for Embodied); cdf_row: f64[width] or None; mean, std: two floats each
  (None for Embodied).  tries is None for Embodied; z, v: the two motion draws before scaling / clipping."""
  u_c = rng.uniform()
  if cfg.action_space == _abi.ACTION_EMBODIED:
    idx, how = choose(u_c, 8, cdf_row, 8)
    return {'actions': np.array([idx // 4, idx % 4], np.int32), 'sprite': idx, 'tries': None, 'how': how, 'u_c': u_c, 'z': (0.0, 0.0),
            'v': (0.0, 0.0)}
  n = len(sprites)
  if n == 0:
    sprite, tries, how, head = -1, 0, NO_SPRITE, (rng.uniform(), rng.uniform())
  else:
    sprite, how = choose(u_c, n, cdf_row, width)
    s = sprites[sprite]
    head, tries = _random_agent_model.contained_from_uniforms(s['pos'], s['path'], s['contains'], _uniforms(rng))
  z = (irwin_hall_z(rng), irwin_hall_z(rng))
  v = tuple(float(mean[c]) + float(std[c]) * z[c] for c in range(2))
  actions = np.array([head[0], head[1], clip01(v[0]), clip01(v[1])], np.float64)
  if cfg.action_is_f32:
    actions = actions.astype(np.float32)
  return {'actions': actions, 'sprite': sprite, 'tries': tries, 'how': how, 'u_c': u_c, 'z': z, 'v': v}


def rollout(cfg, pool, live, seed, first_env, plan, n_cand, n_steps):
  """The model's rollout: (drawn, want).  plan: dict(cdf f64[K, N, W] or None, width, mean, std f64[K, N, 2] or None) in the C
  layout.  drawn: actions [K, N, M, A] in the handle's action dtype, sprite, tries, how i32[K, N, M] (tries -9 for Embodied),
  n_acted i32[K, N, M] (the sprites the draw was taken on), u_c f64[K, N, M], z, v f64[K, N, M, 2].  want: the oracle's outputs
  stepped with those actions, as tests/_rollout_random_model.rollout returns them."""
  from oracle import oracle
  n, s = cfg.n_envs, cfg.max_sprites
  embodied = cfg.action_space == _abi.ACTION_EMBODIED
  a_width = 2 if embodied else 4
  a_dtype = np.int32 if embodied else (np.float32 if cfg.action_is_f32 else np.float64)
  shape = (n_steps, n, n_cand)
  drawn = {'actions': np.zeros(shape + (a_width,), a_dtype), 'sprite': np.full(shape, -9, np.int32), 'tries': np.full(shape, -9, np.int32),
           'how': np.full(shape, -9, np.int32), 'n_acted': np.full(shape, -9, np.int32), 'u_c': np.zeros(shape), 'z': np.zeros(shape + (2,)),
           'v': np.zeros(shape + (2,))}
  want = {'reward': np.zeros(shape), 'discount': np.zeros(shape, np.float32), 'step_type': np.zeros(shape, np.uint8),
          'success': np.zeros(shape, np.uint8), 'error': np.zeros((n, n_cand), np.uint8), 'x': np.zeros((n, n_cand, s)),
          'y': np.zeros((n, n_cand, s)), 'n_sprites': np.zeros((n, n_cand), np.int32), 'x_steps': np.zeros(shape + (s,)),
          'y_steps': np.zeros(shape + (s,)), 'n_sprites_steps': np.zeros(shape, np.int32)}
  for m in range(n_cand):
    ora = oracle.Engine(cfg, pool)
    for a in live:
      ora.step(a, render=False)
    streams = [CandidateStream(seed, first_env + e, m) for e in range(n)]

    def draw(e, k, st):
      sprites = None if embodied else _random_agent_model.oracle_sprites(ora, e, int(st['n_sprites'][e]), st['x'], st['y'])
      d = draw_step(streams[e], cfg, sprites, None if plan['cdf'] is None else plan['cdf'][k, e], plan['width'],
                    None if embodied else plan['mean'][k, e], None if embodied else plan['std'][k, e])
      drawn['actions'][k, e, m], drawn['sprite'][k, e, m], drawn['how'][k, e, m] = d['actions'], d['sprite'], d['how']
      drawn['u_c'][k, e, m], drawn['z'][k, e, m], drawn['v'][k, e, m] = d['u_c'], d['z'], d['v']
      drawn['n_acted'][k, e, m] = 8 if embodied else len(sprites)
      if d['tries'] is not None:
        drawn['tries'][k, e, m] = d['tries']

    st = ora.state()
    for k in range(n_steps):
      resets = st['reset_next'] != 0
      for e in np.flatnonzero(~resets):         # a running episode: the step acts on the sprites as they are
        draw(int(e), k, st)
      out = ora.step(drawn['actions'][k, :, m], render=False)
      st = ora.state()
      for e in np.flatnonzero(resets):          # a FIRST step: the fresh episode's sprites, which the step did not move
        assert out['step_type'][e] == _abi.STEP_FIRST
        draw(int(e), k, st)
      for f in ('reward', 'discount', 'step_type', 'success'):
        want[f][k, :, m] = out[f]
      want['error'][:, m] |= out['error']
      want['x_steps'][k, :, m], want['y_steps'][k, :, m], want['n_sprites_steps'][k, :, m] = st['x'], st['y'], st['n_sprites']
    want['x'][:, m], want['y'][:, m], want['n_sprites'][:, m] = st['x'], st['y'], st['n_sprites']
  return drawn, want
