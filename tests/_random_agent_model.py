"""Pure-Python restatement of the device action sampler (swb_sample_actions_kernel, spriteworld_amd/csrc/swb_sampler.hip.inc).

Test infrastructure: draws the Philox stream of tests/_sampler_model.Stream in the documented order, does the float64
arithmetic of numpy's uniform(low, high) and of sprite.py:117-126 on Python floats (IEEE doubles, one rounding per
operation), takes the geometry from the oracle (oracle.vertices for a pool sprite, oracle.Engine.get_sprite for a sprite the
setters touched) and decides containment with oracle.contains_point -- so a bit-for-bit comparison with the engine checks the
stream, the draw order, the bounding box, the arithmetic and the hit test at once.  `contained_from_uniforms` is the part the
reference itself can check (tests/test_emulated_random_agent.py feeds it MT19937 doubles).
"""
import numpy as np

from spriteworld_amd import _abi
from tests import _sampler_model

MAX_TRIES = _abi.SWB_CONTAINED_MAX_TRIES


def contains_path(path, tx, ty):
  """matplotlib point_in_path (radius 0, even-odd rule) on an explicit centred path, in float64: the test of
  oracle.contains_point for a path no (shape, scale, angle) describes -- one the setters rotated or scaled incrementally."""
  n, inside = len(path), False
  for i in range(n):
    x0, y0 = float(path[i][0]), float(path[i][1])
    x1, y1 = float(path[(i + 1) % n][0]), float(path[(i + 1) % n][1])
    f0, f1 = y0 >= ty, y1 >= ty
    if f0 != f1 and (((y1 - ty) * (x0 - x1) >= (x1 - tx) * (y0 - y1)) == f1):
      inside = not inside
  return inside


def contained_from_uniforms(pos, path, contains, uniforms, max_tries=MAX_TRIES):
  """sprite.py:117-126 with the doubles np.random.uniform would consume handed in: (sample (x, y), tries), tries = -1 and the
  sprite's position when `max_tries` draws all miss.  pos: the position as float64 values; path: [nv, 2] centred vertices;
  contains(tx, ty): sprite.py:113-115 on the centred path; uniforms: an iterator of doubles in [0, 1)."""
  px, py = float(pos[0]), float(pos[1])
  xs, ys = [float(v) for v in path[:, 0]], [float(v) for v in path[:, 1]]
  lo_x, lo_y, hi_x, hi_y = min(xs), min(ys), max(xs), max(ys)          # np.min / np.max over the vertices: exact
  w_x, w_y = hi_x - lo_x, hi_y - lo_y
  for t in range(1, max_tries + 1):
    ux, uy = next(uniforms), next(uniforms)
    sx, sy = px + (lo_x + w_x * ux), py + (lo_y + w_y * uy)            # position + uniform(low, high)
    if contains(sx - px, sy - py):                                      # contains_point(sample): sample - position
      return (sx, sy), t
  return (px, py), -1


def _stream_uniforms(stream):
  while True:
    yield stream.uniform()


def sample_env(seed, entry, mode, cfg, sprites):
  """One environment's draw: dict(actions, position, sprite, tries).  sprites: a list of dict(pos, path, contains) of the
  environment's sprites as they are now, back to front.  position / sprite / tries are None in the uniform mode."""
  rng = _sampler_model.Stream(seed, entry)
  embodied = cfg.action_space == _abi.ACTION_EMBODIED
  position = sprite = tries = None
  if mode == _abi.SAMPLE_ON_SPRITE:
    n = len(sprites)
    if n == 0:
      sprite, tries, position = -1, 0, (rng.uniform(), rng.uniform())
    else:
      sprite = rng.u32() % n
      s = sprites[sprite]
      position, tries = contained_from_uniforms(s['pos'], s['path'], s['contains'], _stream_uniforms(rng))
    head = position
  elif not embodied:
    head = (rng.uniform(), rng.uniform())
  if embodied:
    actions = np.array([rng.u32() % 2, rng.u32() % 4], np.int32)
  else:
    actions = np.array([head[0], head[1], rng.uniform(), rng.uniform()], np.float64)
    if cfg.action_is_f32:
      actions = actions.astype(np.float32)
  return {'actions': actions, 'position': position, 'sprite': sprite, 'tries': tries}


def oracle_sprites(ora, env, n, x, y):
  """The sprites of environment `env` as the oracle engine `ora` sees them now, for sample_env.  A sprite whose path is the
  fresh one of its (shape, scale, angle) is tested with oracle.contains_point; one the setters left another path is tested on
  that path."""
  from oracle import oracle
  out = []
  for k in range(n):
    sp = ora.get_sprite(env, k)
    pool_path = oracle.vertices(sp['shape'], sp['scale'], sp['angle'], 0.0, 0.0)
    fresh = pool_path.shape == sp['path'].shape and np.array_equal(pool_path, sp['path'])
    if fresh:
      contains = (lambda tx, ty, sp=sp: oracle.contains_point(sp['shape'], sp['scale'], sp['angle'], tx, ty))
    else:
      contains = (lambda tx, ty, sp=sp: contains_path(sp['path'], tx, ty))
    out.append({'pos': (float(x[env, k]), float(y[env, k])), 'path': sp['path'], 'contains': contains, 'fresh': fresh})
  return out


def sample_batch(seed, first_env, mode, cfg, ora, state=None):
  """The whole batch: dict of arrays in the C layout of swb_sampled_actions (position / sprite / tries in the sprite mode).
  `ora`: the oracle engine in the state the engine under test is in; `state`: its state() if the caller has it already."""
  st = state or ora.state()
  n_envs = cfg.n_envs
  rows = [sample_env(seed, first_env + e, mode, cfg,
                     oracle_sprites(ora, e, int(st['n_sprites'][e]), st['x'], st['y']) if mode == _abi.SAMPLE_ON_SPRITE else None)
          for e in range(n_envs)]
  out = {'actions': np.stack([r['actions'] for r in rows])}
  if mode == _abi.SAMPLE_ON_SPRITE:
    out['position'] = np.array([r['position'] for r in rows], np.float64).reshape(n_envs, 2)
    out['sprite'] = np.array([r['sprite'] for r in rows], np.int32)
    out['tries'] = np.array([r['tries'] for r in rows], np.int32)
  return out
