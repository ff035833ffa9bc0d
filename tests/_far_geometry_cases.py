"""Sprites far off the canvas, huge, at the edge of the coordinate limit and at non-finite positions (TEST INFRASTRUCTURE ONLY),
written against an engine FACTORY: tests/test_emulated_far_geometry.py runs the cases on the emulated library with a few
environments, tests/test_gpu_far_geometry.py on the HIP engine.

The contract (include/swb.h, SWB_ENV_ERR_SPAN_OVERFLOW): a render path takes canvas coordinates -- (int)(canvas size * vertex),
pil_renderer.py:81-83 -- within +-32000 (tuned paths: the cover kernel's int16 edge records) or +-2^24 (large frames, many
sprites); inside that, frames are +-0 against the oracle wherever the sprite lies; a vertex beyond it, or not finite, flags the
environment, and nothing else about the step differs from the reference.

Scenes are workloads of spriteworld_amd.workloads with keep_in_frame = 0 and pool.x / y / scale overwritten here (rounded through
float32 where the workload's positions are float32).  `canvas_doubles` is numpy's account of sprite.py:131-133 and
pil_renderer.py:81-83 (double arithmetic, then C truncation); every claim a case makes about its scene, and every flag it expects,
comes from it and from the oracle's frames and flags -- never from the engine under test.

  family A  inside the contract: all off-canvas (A1), full cover (A2), a far vertex while crossing the canvas (A3), extreme
            vertices on the truncation edges -1, 0, W - 1, W (A4), and random far / huge sprites
  family B  the edge of the limit: a vertex at exactly +-limit (clean, +-0) beside one at +-(limit + 1) (flagged)
  family C  far beyond the limit and non-finite positions, through swb_set_positions and through drags
"""
import numpy as np

from spriteworld_amd import _abi, shapes, workloads
from tests import _kernel_cases, _parity

FLAG = _abi.ENV_ERR_SPAN_OVERFLOW
TUNED_LIMIT, LF_LIMIT = 32000, 1 << 24

# name -> (workload, anti_aliasing, SWB_* switches, what variant() must say, the start of variant()['kernel'])
PATHS = {
    'resample_96': ('f64_drag', 3, {}, {'large_frames': 0, 'many_sprites': 0, 'paint_in_cover': 0}, 'swb_resample_kernel'),
    'wide_320': ('goal_s5', 5, {}, {'large_frames': 0, 'many_sprites': 0, 'nw': 10}, 'swb_resample_kernel'),
    'wide_640': ('geom_128x64', 5, {}, {'large_frames': 0, 'many_sprites': 0, 'nw': 20}, 'swb_resample_kernel'),
    'paint': ('f64_drag', 1, {}, {'large_frames': 0, 'paint_in_cover': 1}, 'none'),
    'fill': ('geom_128x64', 1, {}, {'large_frames': 0, 'paint_in_cover': 0, 'vs': 0}, 'swb_fill_kernel'),
    'large_natural': ('geom_96x96', 8, {}, {'large_frames': 1, 'many_sprites': 0}, 'swb_lf_raster_kernel'),
    'large_forced': ('f64_drag', 3, {'SWB_LARGE_FRAMES': '1'}, {'large_frames': 1, 'many_sprites': 0}, 'swb_lf_raster_kernel'),
    'many_f64': ('meta_s24_f64', 2, {}, {'large_frames': 1, 'many_sprites': 1}, 'swb_lf_raster_kernel'),
    'many_f32': ('ragged_s64', 3, {}, {'large_frames': 1, 'many_sprites': 1}, 'swb_lf_raster_kernel'),
}
TUNED_PATHS = ('resample_96', 'wide_320', 'wide_640', 'paint', 'fill')
LF_PATHS = ('large_natural', 'large_forced', 'many_f64', 'many_f32')
LF_EDGE_PATHS = ('large_forced', 'many_f64')     # (float64 positions: a float32 position near 2^24 pixels cannot choose its pixel)
# (path, workload): DragAndDrop and SelectMove, float64 and float32 actions, float64 and float32 positions
DRAG_SCENES = (('resample_96', 'f64_drag'), ('resample_96', 'f64_drag_f32a'), ('wide_320', 'goal_s5'), ('wide_320', 'goal_s5_f32a'),
               ('large_forced', 'f64_drag'), ('many_f32', 'ragged_s64_f32a'))
GROUPS = ('A1', 'A2', 'A3', 'A4')
GROUP_ENVS = {'A1': 2, 'A2': 2, 'A3': 4, 'A4': 4}
DIRS8 = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


# ---------------------------------------------------------------------------------------------------------------------
# numpy's account of the vertices
def canvas_size(cfg):
  """(Wc, Hc): PIL's (width, height) of the canvas (oracle/sw_oracle.c render_env)."""
  return cfg.anti_aliasing * cfg.image_h, cfg.anti_aliasing * cfg.image_w


def num(cfg, v):
  """`v` as a position of the workload: through float32 where its positions are float32."""
  return np.float64(np.float32(v)) if cfg.pos_is_f32 else np.float64(v)


def centred_path(pool, e, s, scale=None):
  """f64[n, 2]: sprite.py:96-101, the shape's vertices scaled, then rotated (one matrix, products before the sum, no FMA)."""
  verts, offs = shapes.packed_table()
  sh = int(pool.shape[e, s])
  v = np.asarray(verts, dtype=np.float64).reshape(-1, 2)[offs[sh]:offs[sh + 1]]
  sc = np.float64(pool.scale[e, s] if scale is None else scale)
  ca, sa = np.float64(pool.cos_a[e, s]), np.float64(pool.sin_a[e, s])
  m00, m01, m10, m11 = ca * sc, (-sa) * sc, sa * sc, ca * sc
  return np.stack([(m00 * v[:, 0] + m01 * v[:, 1]) + 0.0, (m10 * v[:, 0] + m11 * v[:, 1]) + 0.0], 1)


def canvas_doubles(cfg, pool, e, s, px, py, scale=None):
  """(fx, fy) f64[n]: canvas size * (centred path + position), before the truncation to int."""
  Wc, Hc = canvas_size(cfg)
  c = centred_path(pool, e, s, scale)
  with np.errstate(invalid='ignore', over='ignore'):
    vx = (1.0 * c[:, 0] + 0.0 * c[:, 1]) + np.float64(px)
    vy = (0.0 * c[:, 0] + 1.0 * c[:, 1]) + np.float64(py)
    return np.float64(Wc) * vx, np.float64(Hc) * vy


def canvas_ints(cfg, pool, e, s, px, py, scale=None):
  """(X, Y): the doubles truncated towards zero (kept as float64: they may lie outside any int; NaN stays NaN)."""
  fx, fy = canvas_doubles(cfg, pool, e, s, px, py, scale)
  return np.trunc(fx), np.trunc(fy)


def sprite_fits(cfg, pool, e, s, px, py, limit):
  X, Y = canvas_ints(cfg, pool, e, s, px, py)
  with np.errstate(invalid='ignore'):
    return bool(np.all(np.abs(X) <= limit) and np.all(np.abs(Y) <= limit))      # (NaN compares false)


def expected_flags(cfg, pool, st, limit):
  """u8[N]: FLAG where a live sprite of the oracle's state `st` has a vertex beyond +-limit or not finite."""
  out = np.zeros(cfg.n_envs, np.uint8)
  for i in range(cfg.n_envs):
    e = int(st['pool_entry'][i])
    if not all(sprite_fits(cfg, pool, e, s, st['x'][i, s], st['y'][i, s], limit) for s in range(int(st['n_sprites'][i]))):
      out[i] = FLAG
  return out


def polygon_mask(cfg, X, Y):
  """bool[Hc, Wc]: the pixels the oracle's polygon fill gives the vertices (X, Y) on an empty canvas."""
  from oracle import oracle
  Wc, Hc = canvas_size(cfg)
  img = oracle.fill_polygon(Wc, Hc, np.stack([X, Y], 1).astype(np.int32))
  return img[..., 0] != 0


def bisect_position(cfg, f, target, lo, hi):
  """A position p in [lo, hi] (of the workload's dtype) with f(p) as close to `target` as the dtype allows; f increasing."""
  lo, hi = np.float64(lo), np.float64(hi)
  for _ in range(200):
    mid = num(cfg, 0.5 * (lo + hi))
    if not lo < mid < hi:
      break
    if f(mid) < target:
      lo = mid
    else:
      hi = mid
  return min((num(cfg, lo), num(cfg, hi)), key=lambda p: abs(f(p) - target))


def place_extreme(cfg, pool, e, s, axis, side, value):
  """The position along `axis` (0: x, 1: y) at which the sprite's extreme vertex on `side` (-1: smallest, +1: largest
  coordinate) has the canvas DOUBLE closest to `value`; the other coordinate stays."""
  other = pool.y[e, s] if axis == 0 else pool.x[e, s]

  def f(p):
    d = canvas_doubles(cfg, pool, e, s, p, other) if axis == 0 else canvas_doubles(cfg, pool, e, s, other, p)
    return d[axis].min() if side < 0 else d[axis].max()
  size = canvas_size(cfg)[axis]
  span = (abs(value) + 4.0 * size) / size + 4.0 * float(pool.scale[e, s])
  return bisect_position(cfg, f, value, -span, span)


# ---------------------------------------------------------------------------------------------------------------------
# scenes
class Scene(object):
  """A workload with keep_in_frame = 0, far / huge random sprites, and crafted environments in front."""

  def __init__(self, path, n_envs, seed=0, limit=None, keep_in_frame=0, name=None, random_far=True):
    wl, aa, self.switches, self.expect, self.kernel = PATHS[path]
    self.path = path
    self.cfg, self.pool, self.sample = workloads.build(name or wl, n_envs, episodes_per_env=2, seed=seed, anti_aliasing=aa)
    self.cfg.keep_in_frame = keep_in_frame
    self.N = n_envs
    self.limit = limit or (LF_LIMIT if self.expect['large_frames'] else TUNED_LIMIT)
    self.rng = np.random.default_rng(seed + 17)
    self.claims = {}                 # environment -> (group, what it claims)
    self.next_env = 0
    if random_far:
      self.randomise()

  # the recipe: scales log-uniform up to 15000 / max(Wc, Hc), 40 % of the positions in [-0.5, 1.5], the others uniform within
  # +-15000 / max(Wc, Hc) -- all of it scaled by limit / 32000.  In scenes of more than 16 sprites each sprite follows it with
  # probability 4 / S and is a small sprite in or around the frame otherwise (two dozen huge sprites leave no frame to look at).
  # The first episode of every third environment is drawn again until the ORACLE's frame of it shows background and sprites.
  def draw(self, rows):
    cfg, pool, rng = self.cfg, self.pool, self.rng
    reach = 15000.0 * (self.limit / 32000.0) / max(canvas_size(cfg))
    shape = pool.x[rows].shape
    near = rng.uniform(size=shape) < 0.4
    tame = rng.uniform(size=shape) >= 4.0 / max(pool.max_sprites, 4)
    pool.x[rows] = np.where(near | tame, rng.uniform(-0.5, 1.5, size=shape), rng.uniform(-reach, reach, size=shape))
    pool.y[rows] = np.where(near | tame, rng.uniform(-0.5, 1.5, size=shape), rng.uniform(-reach, reach, size=shape))
    pool.scale[rows] = np.where(tame, np.exp(rng.uniform(np.log(0.03), np.log(0.4), size=shape)),
                                np.exp(rng.uniform(np.log(0.05), np.log(reach), size=shape)))
    if cfg.pos_is_f32:
      for arr in (pool.x, pool.y, pool.scale):
        arr[rows] = arr[rows].astype(np.float32).astype(np.float64)

  def randomise(self, mixed_every=3):
    from oracle import oracle
    cfg, pool = self.cfg, self.pool
    self.draw(slice(None))
    bg = np.array([cfg.bg_rgb[0], cfg.bg_rgb[1], cfg.bg_rgb[2]], np.uint8)
    for env in range(0, self.N, mixed_every):
      e = self.entries(env)[0]
      n = int(pool.n_sprites[e])
      for _ in range(400 if n else 0):
        f = oracle.render_sprites(cfg, pool.x[e, :n], pool.y[e, :n], pool.shape[e, :n], pool.scale[e, :n], pool.cos_a[e, :n],
                                  pool.sin_a[e, :n], pool.rgb[e, :n, :3])
        if (f != bg).any() and (f == bg).all(axis=-1).any():
          break
        self.draw(slice(e, e + 1))

  def entries(self, env):
    """The pool entries environment `env` plays, in turn."""
    return [int(self.pool.pool_base[env]) + k for k in range(int(self.pool.pool_len[env]))]

  def take(self, min_sprites=1, ok=None):
    """The next environment not crafted yet whose first episode has `min_sprites` sprites (and passes `ok(entry)`)."""
    for env in range(self.N):
      e = self.entries(env)[0]
      if env not in self.claims and self.pool.n_sprites[e] >= min_sprites and (ok is None or ok(e)):
        return env, e
    raise AssertionError('no environment left for a crafted scene (%s, %d environments)' % (self.path, self.N))

  def put(self, env, e, s, x=None, y=None, scale=None):
    """Writes sprite `s` of entry `e` (the first episode of `env`) in the workload's position dtype."""
    pool, cfg = self.pool, self.cfg
    if scale is not None:
      pool.scale[e, s] = num(cfg, scale)
    if x is not None:
      pool.x[e, s] = num(cfg, x)
    if y is not None:
      pool.y[e, s] = num(cfg, y)

  def in_contract(self):
    """Every sprite of every episode lies within the path's limit where its episode starts."""
    pool = self.pool
    return all(sprite_fits(self.cfg, pool, e, s, pool.x[e, s], pool.y[e, s], self.limit)
               for e in range(pool.n_entries) for s in range(int(pool.n_sprites[e])))

  # ---- A1: every sprite wholly outside the canvas, the eight directions among them
  def craft_a1(self):
    cfg, pool = self.cfg, self.pool
    k = 0
    for _ in range(GROUP_ENVS['A1']):
      env, e = self.take(4)
      for s in range(int(pool.n_sprites[e])):
        dx, dy = DIRS8[k % 8]
        k += 1
        self.put(env, e, s, x=0.5 + dx * (3.0 + 0.37 * (k % 11)), y=0.5 + dy * (3.0 + 0.21 * (k % 7)), scale=0.3)
      self.claims[env] = ('A1', e)

  # ---- A2: one sprite covers the whole canvas: top-most, then bottom-most under small sprites
  def craft_a2(self):
    cfg, pool = self.cfg, self.pool
    big = min(40.0, 12000.0 / max(canvas_size(cfg)))
    for where in ('top', 'bottom'):
      env, e = self.take(2)
      n = int(pool.n_sprites[e])
      cover = n - 1 if where == 'top' else 0
      for s in range(n):
        if s == cover:
          self.put(env, e, s, x=0.5, y=0.5, scale=big)
        else:
          self.put(env, e, s, x=self.rng.uniform(0.2, 0.8), y=self.rng.uniform(0.2, 0.8), scale=0.12)
      self.claims[env] = ('A2', (e, cover, where))

  # ---- A3: a sprite with a vertex 25000 .. 32000 pixels (scaled with the limit) to the left / right / below / above, whose
  # opposite corner lies in the middle of the canvas: its edges cross the frame after tens of thousands of rows or columns
  def craft_a3(self):
    pool = self.pool
    far = 26500.0 * (self.limit / 32000.0)
    for axis, side in ((0, -1), (0, 1), (1, -1), (1, 1)):
      found = None
      for env in range(self.N):
        e = self.entries(env)[0]
        if env in self.claims:
          continue
        for s in range(int(pool.n_sprites[e]) - 1, -1, -1):
          found = found or self.fit_a3(env, e, s, axis, side, far)
        if found:
          break
      assert found, ('A3: no sprite fits', self.path, axis, side)
      env, e, s, pos, scale = found
      self.put(env, e, s, x=pos[0], y=pos[1], scale=scale)
      for above in range(s + 1, int(pool.n_sprites[e])):     # nothing hides it
        self.put(env, e, above, x=4.0, y=0.5, scale=0.3)
      self.claims[env] = ('A3', (e, s, axis, side))

  def fit_a3(self, env, e, s, axis, side, far):
    """(env, e, s, position, scale) with which sprite `s` makes the A3 scene of that direction, or None."""
    cfg, pool, L = self.cfg, self.pool, self.limit
    size = np.array(canvas_size(cfg), np.float64)
    if shapes.SHAPE_NAMES[int(pool.shape[e, s])] == 'square' and pool.angle[e, s] % 90 == 0:
      return None                                            # (axis-aligned edges have no slope to speak of)
    unit = centred_path(pool, e, s, scale=1.0) * size
    extent = unit[:, axis].max() - unit[:, axis].min()
    scale = num(cfg, (far + 0.5 * size[axis]) / extent)
    c = centred_path(pool, e, s, scale=scale) * size
    near = int(np.argmin(c[:, axis]) if side > 0 else np.argmax(c[:, axis]))    # the corner that stays on the canvas
    pos = [num(cfg, (size[a] * 0.5 - c[near, a]) / size[a]) for a in (0, 1)]
    X, Y = canvas_ints(cfg, pool, e, s, pos[0], pos[1], scale=scale)
    if max(np.abs(X).max(), np.abs(Y).max()) > L or (side * (X, Y)[axis]).max() < 25000.0 * (L / 32000.0):
      return None
    mask = polygon_mask(cfg, X, Y)
    return (env, e, s, pos, scale) if mask.any() and not mask.all() else None

  # ---- A4: extreme vertices that truncate to -1, 0 (from a double in (-1, 0) and from one in [0, 1)), size - 1 and size
  A4_CASES = ((-1, -1.5, -1.0), (-1, -0.5, 0.0), (-1, 0.5, 0.0), (1, -0.5, 'size-1'), (1, 0.5, 'size'))

  def craft_a4(self):
    cfg, pool = self.cfg, self.pool
    jobs = [(axis, c) for axis in (0, 1) for c in self.A4_CASES]
    made = []
    while jobs:
      env, e = self.take(1)
      for s in range(int(pool.n_sprites[e])):
        if not jobs:
          break
        axis, (side, offset, want) = jobs.pop(0)
        size = canvas_size(cfg)[axis]
        base = 0.0 if side < 0 else float(size)
        self.put(env, e, s, x=0.5, y=0.5, scale=0.21)
        p = place_extreme(cfg, pool, e, s, axis, side, base + offset)
        self.put(env, e, s, **{'xy'[axis]: p})
        made.append((e, s, axis, side, base + offset, (size - 1 if want == 'size-1' else size if want == 'size' else want)))
      self.claims[env] = ('A4', e)
    self.a4 = made

  def craft(self, groups):
    for g in groups:
      getattr(self, 'craft_' + g.lower())()
    return self

  # ---- what the crafted scenes claim, on the helper and the oracle's first frames
  def check_claims(self, frames):
    cfg, pool = self.cfg, self.pool
    Wc, Hc = canvas_size(cfg)
    bg = np.array([cfg.bg_rgb[0], cfg.bg_rgb[1], cfg.bg_rgb[2]], np.uint8)
    dirs = set()
    for env, (group, what) in self.claims.items():
      f = frames[env]
      if group == 'A1':
        e = what
        for s in range(int(pool.n_sprites[e])):
          X, Y = canvas_ints(cfg, pool, e, s, pool.x[e, s], pool.y[e, s])
          dx = -1 if X.max() < 0 else (1 if X.min() >= Wc else 0)
          dy = -1 if Y.max() < 0 else (1 if Y.min() >= Hc else 0)
          assert (dx, dy) != (0, 0), ('A1: a sprite reaches the canvas', self.path, env, s)
          dirs.add((dx, dy))
        assert (f == bg).all(), ('A1: the oracle frame is not the background', self.path, env)
      elif group == 'A2':
        e, cover, where = what
        X, Y = canvas_ints(cfg, pool, e, cover, pool.x[e, cover], pool.y[e, cover])
        assert polygon_mask(cfg, X, Y).all(), ('A2: the sprite does not cover the canvas', self.path, env)
        if where == 'top':
          assert (f != bg).any(axis=-1).all(), ('A2: a background pixel under the top-most cover', self.path, env)
        else:
          assert len(np.unique(f.reshape(-1, 3), axis=0)) >= 2, ('A2: nothing shows above the cover', self.path, env)
      elif group == 'A3':
        e, s, axis, side = what
        X, Y = canvas_ints(cfg, pool, e, s, pool.x[e, s], pool.y[e, s])
        k = self.limit / 32000.0
        assert 25000.0 * k <= ((X, Y)[axis] * side).max() <= self.limit, ('A3: far vertex', self.path, env)
        mask = polygon_mask(cfg, X, Y)
        assert mask.any() and not mask.all(), ('A3: the sprite does not cross the canvas', self.path, env)
        assert (f != bg).any(), ('A3: frame', self.path, env)
    if any(g == 'A1' for g, _ in self.claims.values()):
      assert dirs == set(DIRS8), ('A1: directions', sorted(dirs))
    for e, s, axis, side, value, want in getattr(self, 'a4', ()):
      d = canvas_doubles(cfg, pool, e, s, pool.x[e, s], pool.y[e, s])[axis]
      ext = d.min() if side < 0 else d.max()
      assert np.trunc(ext) == want and abs(ext - value) < 0.45, ('A4', self.path, e, s, axis, side, ext, value, want)

  def random_envs(self):
    return [i for i in range(self.N) if i not in self.claims]

  def check_random_floor(self, frames):
    """At least a tenth of the random environments show both background and sprite pixels."""
    cfg = self.cfg
    bg = np.array([cfg.bg_rgb[0], cfg.bg_rgb[1], cfg.bg_rgb[2]], np.uint8)
    envs = self.random_envs()
    both = sum(1 for i in envs if (frames[i] != bg).any() and (frames[i] == bg).all(axis=-1).any())
    assert 10 * both >= len(envs) and both >= 1, ('random far scenes: too few show sprites and background', self.path, both, len(envs))


class Pair(object):
  """The engine beside the oracle (told the limit of the path the engine takes), the engine's flags so far."""

  def __init__(self, make_engine, monkeypatch, scene):
    from oracle import oracle
    for k, v in scene.switches.items():
      monkeypatch.setenv(k, v)
    self.scene, self.cfg, self.pool = scene, scene.cfg, scene.pool
    self.ora, self.eng = oracle.Engine(scene.cfg, scene.pool), make_engine(scene.cfg, scene.pool)
    v = self.eng.variant()
    for k, value in scene.expect.items():
      assert v[k] == value, (scene.path, k, v)
    assert v['kernel'].startswith(scene.kernel), (scene.path, v['kernel'])
    self.limit = LF_LIMIT if v['large_frames'] else TUNED_LIMIT
    self.ora.set_coord_limit(self.limit)
    _kernel_cases._violations(self.eng)
    self.sticky = np.zeros(scene.N, np.uint8)
    self.t = 0
    self.flagged_steps = 0

  def step(self, a, clean=False):
    """One step of both, to the bar of _parity.compare; the frame of an environment flagged AT THIS STEP is not compared.
    `clean`: no environment may be flagged at this step.  Returns the oracle's outputs."""
    want = self.ora.step(a)
    self.eng.step(a)
    st = self.ora.state()
    mine = expected_flags(self.cfg, self.pool, st, self.limit)
    np.testing.assert_array_equal(want['error'] & FLAG, mine, err_msg='%s t=%d: the oracle\'s flags against numpy\'s' % (self.scene.path, self.t))
    if clean:
      assert not want['error'].any(), (self.scene.path, self.t, np.flatnonzero(want['error']))
    self.sticky |= want['error']
    self.flagged_steps += int((want['error'] & FLAG != 0).sum())
    _parity.compare(self.t, self.ora, self.eng, want, self.eng.outputs_host(), what=self.scene.path,
                    errors=self.sticky.copy() if self.sticky.any() else None, nan_positions=True,
                    frame_envs=(want['error'] & FLAG) == 0)
    assert _kernel_cases._violations(self.eng) == 0, (self.scene.path, self.t)
    self.t += 1
    return want

  def clear(self):
    """The caller clears the sticky flags."""
    self.eng.error.zero_()
    self.sticky[:] = 0

  def set_positions(self, x, y):
    if self.cfg.pos_is_f32:
      with np.errstate(over='ignore', invalid='ignore'):
        x, y = x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    self.ora.set_positions(x, y)
    self.eng.set_positions(x, y)

  def close(self):
    self.eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# family A
def family_a(make_engine, monkeypatch, path, n_envs, groups=GROUPS, steps=3, seed=0, limit=None, random_floor=True):
  """Inside the contract: frames +-0, everything else to the bar of _parity.compare, no flag at any step.  `limit`: the
  coordinate limit the random recipe and A3 are scaled to (default: the path's own)."""
  scene = Scene(path, n_envs, seed=seed, limit=limit).craft(groups)
  assert scene.in_contract(), path
  p = Pair(make_engine, monkeypatch, scene)
  assert scene.limit <= p.limit
  rng = np.random.default_rng(seed + 100)
  for t in range(steps):
    want = p.step(scene.sample(rng))
    if t == 0:
      scene.check_claims(want['obs'])
      if random_floor:
        scene.check_random_floor(want['obs'])
  assert not p.sticky.any()
  p.close()


# ---------------------------------------------------------------------------------------------------------------------
# family B
def family_b(make_engine, monkeypatch, path, n_envs, seed=1):
  """For +x, -x, +y, -y two neighbouring environments: the farthest vertex at exactly +-limit (clean, +-0) and at
  +-(limit + 1) (flagged).  The flag stays until the caller clears it; after swb_set_positions brings the sprites back the next
  step is clean and +-0."""
  scene = Scene(path, n_envs, seed=seed, random_far=False)
  cfg, pool = scene.cfg, scene.pool
  pool.x_vel[:] = 0.0          # (the edge is a matter of one pixel: nothing drifts while the case looks at it)
  pool.y_vel[:] = 0.0
  L = scene.limit
  at, beyond = [], []
  for axis, side in ((0, 1), (0, -1), (1, 1), (1, -1)):
    for over in (0, 1):
      env, e = scene.take(1)
      s = int(pool.n_sprites[e]) - 1
      scene.put(env, e, s, x=0.5, y=0.5, scale=0.17)
      p0 = place_extreme(cfg, pool, e, s, axis, side, side * (L + over + 0.5))
      scene.put(env, e, s, **{'xy'[axis]: p0})
      X, Y = canvas_ints(cfg, pool, e, s, pool.x[e, s], pool.y[e, s])
      assert ((X, Y)[axis] * side).max() == L + over and max(np.abs(X).max(), np.abs(Y).max()) == L + over, (path, axis, side, over)
      scene.claims[env] = ('B', over)
      (beyond if over else at).append(env)
  p = Pair(make_engine, monkeypatch, scene)
  assert p.limit == L
  want = p.step(miss_actions(scene))                        # FIRST: the episodes start on the edge
  np.testing.assert_array_equal(np.flatnonzero(want['error'] & FLAG), sorted(beyond))
  # the sprites come back before the episode's second step (a sprite outside the frame would end it there: sprite.py:135-138)
  # sticky: the engine's buffer keeps the flag through a step in which nothing is flagged
  st = p.ora.state()
  x, y = st['x'].copy(), st['y'].copy()
  for env in at + beyond:
    n = int(st['n_sprites'][env])
    x[env, :n], y[env, :n] = 0.4, 0.6
  p.set_positions(x, y)
  p.step(miss_actions(scene), clean=True)
  np.testing.assert_array_equal(np.flatnonzero(p.eng.outputs_host()['error'] & FLAG), sorted(beyond))
  p.clear()
  p.step(miss_actions(scene), clean=True)                   # cleared, and the sprites are back: a clean step, every frame +-0
  assert not p.eng.outputs_host()['error'].any()
  p.close()


def miss_actions(scene, value=0.97):
  """A click no crafted sprite is under and a zero motion (SelectMove: a[2:] = 0.5; DragAndDrop: a[2:] = a[:2]); Embodied: no
  grab."""
  cfg, N = scene.cfg, scene.N
  if cfg.action_space == _abi.ACTION_EMBODIED:
    return np.zeros((N, 2), np.int32)
  a = np.full((N, 4), value)
  if cfg.action_space != _abi.ACTION_DRAG_AND_DROP:
    a[:, 2:] = 0.5
  return a.astype(np.float32) if cfg.action_is_f32 else a


# ---------------------------------------------------------------------------------------------------------------------
# family C
FAR_COORDS = (1e5, 3e7, -3e7, 1e12, -1e12, 1e300, -1e300)
NON_FINITE = (np.nan, np.inf, -np.inf)


def family_c_positions(make_engine, monkeypatch, path, n_envs, seed=2):
  """swb_set_positions puts one sprite of every second environment at a canvas coordinate far beyond the limit, or at a
  non-finite position: exactly the environments the oracle and numpy flag are flagged, every other environment is +-0, positions
  are the oracle's (NaN where it has NaN), rewards and step types are the oracle's."""
  scene = Scene(path, n_envs, seed=seed, random_far=False)      # (sprites in the frame: the episodes of the others go on)
  cfg = scene.cfg
  Wc, Hc = canvas_size(cfg)
  p = Pair(make_engine, monkeypatch, scene)
  rng = np.random.default_rng(seed + 100)
  p.step(scene.sample(rng))
  values = list(NON_FINITE) + [c / Wc for c in FAR_COORDS]
  total = k = 0
  for rnd in range(2):
    st = p.ora.state()
    x, y = st['x'].copy(), st['y'].copy()
    for env in range(rnd, n_envs, 2):
      n = int(st['n_sprites'][env])
      if n == 0 or st['reset_next'][env]:
        continue
      s = k % n
      (x if k % 2 == 0 else y)[env, s] = values[k % len(values)]
      k += 1
    p.set_positions(x, y)
    before = p.flagged_steps
    want = p.step(scene.sample(rng))
    total += p.flagged_steps - before
  assert total >= min(n_envs // 2, 3), (path, total)
  p.step(scene.sample(rng))                                  # the flagged episodes ended (a sprite out of frame): fresh ones
  p.close()


def drag_actions(scene, st, motions):
  """Actions that click the centre of the top-most sprite of environment i and ask for motion `motions[i]` in x (None: a miss)."""
  cfg = scene.cfg
  a = miss_actions(scene).astype(np.float64)
  with np.errstate(over='ignore', invalid='ignore'):
    for i, m in enumerate(motions):
      n = int(st['n_sprites'][i])
      if m is None or n == 0:
        continue
      a[i, 0], a[i, 1] = st['x'][i, n - 1], st['y'][i, n - 1]
      if cfg.action_space == _abi.ACTION_DRAG_AND_DROP:
        a[i, 2], a[i, 3] = a[i, 0] + m / cfg.action_scale, a[i, 1]
      else:
        a[i, 2], a[i, 3] = 0.5 + m / cfg.action_scale, 0.5
    return a.astype(np.float32) if cfg.action_is_f32 else a


DRAG_MOTIONS = (1e30, -1e30, np.nan, np.inf, -np.inf)


def family_c_drags(make_engine, monkeypatch, path, n_envs, name, keep_in_frame=0, seed=3):
  """A drag whose motion is +-1e30, NaN or +-inf on every second environment (`name`: the workload, '_f32a' for float32
  actions).  keep_in_frame = 0: all of them leave the contract and are flagged.  keep_in_frame = 1: the clip (np.clip(pos, 0, 1))
  brings +-1e30 and +-inf back to 0 or 1 -- finite, +-0, no flag -- and only NaN survives it."""
  scene = Scene(path, n_envs, seed=seed, keep_in_frame=keep_in_frame, name=name, random_far=False)
  # sprites in the frame, so that the click on a centre hits: the workload's own positions
  from oracle import oracle
  p = Pair(make_engine, monkeypatch, scene)
  rng = np.random.default_rng(seed + 100)
  p.step(scene.sample(rng))
  st = p.ora.state()
  motions = [DRAG_MOTIONS[(i // 2) % len(DRAG_MOTIONS)] if i % 2 == 0 else None for i in range(n_envs)]
  # the click lands on the centre of the top-most sprite, which is the first one asked (action_spaces.py:77-81): a hit where
  # the centre lies inside the sprite's polygon
  pool = scene.pool
  moved = []
  for i in range(n_envs):
    n, e = int(st['n_sprites'][i]), int(st['pool_entry'][i])
    if motions[i] is not None and n and not st['reset_next'][i] and oracle.contains_point(
        int(pool.shape[e, n - 1]), pool.scale[e, n - 1], pool.angle[e, n - 1], 0.0, 0.0):
      moved.append(i)
  want = p.step(drag_actions(scene, st, motions))
  after = p.ora.state()
  assert len(moved) >= min(3, n_envs // 2), ('the drags missed', path, name, moved)
  flagged = np.flatnonzero(want['error'] & FLAG)
  if keep_in_frame:
    nan_envs = [i for i in moved if np.isnan(motions[i])]
    np.testing.assert_array_equal(flagged, nan_envs)
    assert all(np.isfinite(after['x'][i, :int(after['n_sprites'][i])]).all() for i in moved if not np.isnan(motions[i]))
  else:
    np.testing.assert_array_equal(flagged, moved)
  p.step(scene.sample(rng))
  p.close()


# ---------------------------------------------------------------------------------------------------------------------
# one rollout
def rollout_case(make_engine, monkeypatch, path='resample_96', n_envs=8, seed=4):
  """rollout with M = 2: candidate 0 misses, candidate 1 drags the top-most sprite past the limit.  rollout_frames()['error'] is
  flagged at [n, 1] only, frame [n, 0] is the oracle's, and the live state and the caller's flags are untouched."""
  from oracle import oracle
  scene = Scene(path, n_envs, seed=seed, random_far=False)
  cfg, pool = scene.cfg, scene.pool
  p = Pair(make_engine, monkeypatch, scene)
  rng = np.random.default_rng(seed + 100)
  live = [scene.sample(rng) for _ in range(2)]
  for a in live:
    p.step(a)
  st = p.ora.state()
  cand = np.stack([miss_actions(scene), drag_actions(scene, st, [1e30] * n_envs)], 1)[None]       # [K = 1, N, M = 2, 4]
  wants = []
  for m in range(2):
    ora = oracle.Engine(cfg, pool)
    ora.set_coord_limit(p.limit)
    for a in live:
      ora.step(a, render=False)
    wants.append(ora.step(cand[0, :, m]))
  assert not (wants[0]['error'] & FLAG).any() and (wants[1]['error'] & FLAG).sum() >= n_envs // 2
  live_before = p.eng.state()
  res = p.eng.rollout(cand, positions=True)
  fr = p.eng.rollout_frames()
  err = fr['error'].cpu().numpy()
  np.testing.assert_array_equal(err[:, 0], wants[0]['error'] & FLAG)
  np.testing.assert_array_equal(err[:, 1], wants[1]['error'] & FLAG)
  np.testing.assert_array_equal(fr['obs'].cpu().numpy()[:, 0], wants[0]['obs'])
  assert not res['error'].cpu().numpy().any()               # (the state phases of the rollout raise no raster flag)
  for m in range(2):
    _parity.assert_rewards_equal(res['reward'].cpu().numpy()[0, :, m], wants[m]['reward'], 'rollout candidate %d' % m)
  live_after = p.eng.state()
  for k in live_before:
    np.testing.assert_array_equal(live_after[k], live_before[k], err_msg=k)
  assert not p.eng.outputs_host()['error'].any()
  p.step(scene.sample(rng), clean=True)                      # the live episode goes on as if nothing had been asked
  p.close()
