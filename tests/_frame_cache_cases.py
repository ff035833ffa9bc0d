"""Scenes for the frame cache (tests/test_emulated_frame_cache.py, tests/test_gpu_frame_cache.py).

Where a cover wave kept its run lists, the resample waves of its environment write the caller's frame from the engine's own copy
of the previous frame instead of from the lists: the first launch that keeps FILLS the copy (header word 1), every further one
COPIES from it (word 2), a launch that builds the lists RESAMPLES only (word 0).  Every case steps the engine beside oracle.Engine
through the bar of tests/_parity.py at EVERY step -- frames +-0 -- with SWB_LIST_STATS set, and holds swb_frame_stats and
swb_list_stats to the counts a model of the three-state word gives for the oracle's own step types and the script's clicks: no
case passes with a path dead, or taken where it must not be.

The scene: five sprites (squares and circles of scale 0.13) in the left half, a goal far outside the frame, SelectMove(scale=0.1),
64x64 at anti_aliasing 5 on black unless the case says otherwise.  A MISS clicks at x > 0.8; a HIT clicks on the centre of the
top sprite and moves it by (+0.04, -0.02).  The engines never trim their lists by themselves (Engine.TRIM_AFTER).
"""
import numpy as np
import torch

from spriteworld_amd import _abi
from spriteworld_amd import action_spaces
from spriteworld_amd import lowering
from spriteworld_amd import renderers
from spriteworld_amd import synthetic
from spriteworld_amd import tasks
from tests import _parity
from tests import _resample_tables

N_SPRITES = 5
# per environment: build, fill, move, fill, move (a fill that no copy follows), fill, copy, copy, move, fill
SCRIPT = (0, 0, 1, 0, 1, 0, 0, 0, 1, 0)
BETWEEN = ('render', 'evaluate', 'step_without_frame', 'set_positions', 'sprite_setter', 'trim', 'rollout_frames', 'upload_tables')
GEOMETRIES = ('two_column_groups', 'bands_default', 'one_band', 'band_tasks_8', 'background')


def build(n_envs, aa=5, size=(64, 64), bg=(0, 0, 0), max_episode_length=50, episodes_per_env=4, seed=0):
  rng = np.random.default_rng(seed)
  P = n_envs * episodes_per_env
  n = N_SPRITES
  rend = {'image': renderers.PILRenderer(image_size=size, anti_aliasing=aa, bg_color=bg, color_to_rgb=renderers.hsv_to_rgb)}
  task = tasks.FindGoalPosition(filter_distrib=None, goal_position=(3., 3.), terminate_distance=0.01)
  aspace = action_spaces.SelectMove(scale=0.1)
  pool = synthetic.make_pool(rng, P, n, [(0.0, 1.0)] * n, [[1]] * n, shape_names=('square', 'circle'), scales=(0.13,), angles=(0,),
                             shuffle=False)
  for e in range(P):
    for s in range(n):
      pool.x[e, s] = float(np.float32(rng.uniform(0.15, 0.45)))
      pool.y[e, s] = float(np.float32(rng.uniform(0.15, 0.85)))
  pool.x_vel[:] = 0.0
  pool.y_vel[:] = 0.0
  cfg = lowering.lower_config(task, aspace, rend, True, max_episode_length, n_envs, n, True)
  pool.assign_round_robin(n_envs, episodes_per_env)
  return cfg, pool


def actions(state, hit, motion=(0.9, 0.3)):
  N = state['x'].shape[0]
  a = np.empty((N, 4))
  top = N_SPRITES - 1
  a[:, 0] = np.where(hit, state['x'][:, top], 0.9)
  a[:, 1] = np.where(hit, state['y'][:, top], 0.5)
  a[:, 2], a[:, 3] = motion
  return a


class Pair(object):
  """The engine and the oracle side by side, and the model of the header word: `word[e]` is what SWB_RHDR_FRAME of environment e
  holds.  A rendering launch in which e keeps its lists moves it to min(word + 1, 2) on a handle with a cache, any other to 0;
  its tasks -- one per column group and band -- then count as copied (2), filled (1) or resampled (0).
  `tables` (the horizontal pair (bounds, coeffs), the vertical pair): resampling tables uploaded over the engine's own before the
  first step -- the frames every step is held to are then tests/_resample_tables.py's two passes, with these tables, over the
  canvases a second oracle paints; `canvases`: keep that second oracle in step for an `upload` later on."""

  def __init__(self, make_engine, monkeypatch, cfg, pool, what, env=(), cache=True, tables=None, canvases=False):
    from oracle import oracle
    monkeypatch.setenv('SWB_LIST_STATS', '1')
    for k, v in env:
      monkeypatch.setenv(k, v)
    self.cfg, self.what, self.t = cfg, what, 0
    self.ora, self.eng = oracle.Engine(cfg, pool), make_engine(cfg, pool)
    self.eng.TRIM_AFTER = 0
    self.N = cfg.n_envs
    v = self.eng.variant()
    self.cache = cache
    assert v['frame_cache_bytes'] == (self.N * cfg.image_w * cfg.image_h * 3 if cache else 0), v
    self.tasks = v['n_bands'] * v['n_column_groups']      # of the resample kernel, per environment and launch
    self.paints = bool(v['paint_in_cover'])
    self.word = np.zeros(self.N, np.int64)
    self.kept = self.built = 0
    self.copied = self.filled = self.resampled = 0
    self.scribble = False
    self.frames = []
    self.tables = None
    self.big = _resample_tables.canvases(cfg, pool) if (tables is not None or canvases) else None
    if tables is not None:
      self.upload(*tables)

  def upload(self, tab_h, tab_v):
    """swb_upload_resample of both axes on the live handle: from here on the frames are these tables'.  (The bands follow the
    tables: the tasks per environment are read again after the next launch.)"""
    assert self.big is not None
    _resample_tables.upload(self.eng, tab_h, tab_v)
    self.tables = (tab_h, tab_v)

  def expected(self, want, canv):
    """`want` with the frames the uploaded tables give (the oracle's own where none were uploaded)."""
    if self.big is not None:
      for k in ('step_type', 'success'):
        np.testing.assert_array_equal(canv[k], want[k], err_msg='%s canvases %s t=%d' % (self.what, k, self.t))
    if self.tables is not None and want['obs'] is not None:
      want['obs'] = _resample_tables.expected_frames(canv['obs'], *self.tables)
    return want

  def launch(self, keeps):
    """A rendering launch of the live state in which the waves of `keeps` kept their lists."""
    keeps = np.broadcast_to(np.asarray(keeps, dtype=bool), (self.N,))
    if not self.paints:                                 # (a cover build that paints the frame itself has no lists to count)
      self.kept += int(keeps.sum())
      self.built += int((~keeps).sum())
    self.word = np.where(keeps & self.cache, np.minimum(self.word + 1, 2), 0)
    if self.tables is not None:
      v = self.eng.variant()
      self.tasks = v['n_bands'] * v['n_column_groups']
    resample_kernel = self.cfg.anti_aliasing != 1       # (the fill kernel and the painting builds count nothing)
    if resample_kernel:
      self.copied += self.tasks * int((self.word == 2).sum())
      self.filled += self.tasks * int((self.word == 1).sum())
      self.resampled += self.tasks * int((self.word == 0).sum())
    self.check_counts()

  def check_counts(self):
    got = self.eng.list_stats(), self.eng.frame_stats()
    want = (self.kept, self.built), (self.copied, self.filled, self.resampled)
    assert got == want, (self.what, self.t, got, want)

  def step(self, hit, keeps=None, render=True):
    hit = np.broadcast_to(np.asarray(hit, dtype=bool), (self.N,))
    a = actions(self.ora.state(), hit)
    want = self.ora.step(a, render=render)
    if self.big is not None:
      want = self.expected(want, self.big.step(a, render=render and self.tables is not None))
    if self.scribble:
      self.eng.obs.fill_(0xA5)
    self.eng.step(a, render=render)
    got = self.eng.outputs_host()
    _parity.compare(self.t, self.ora, self.eng, want, got, frames=render, what=self.what)
    if render:
      self.frames.append(got['obs'].copy())
      if keeps is None:
        keeps = (want['step_type'] != _abi.STEP_FIRST) & ~hit
      self.launch(keeps)
    self.t += 1
    return want

  def render(self, keeps):
    if self.scribble:
      self.eng.obs.fill_(0xA5)
    want = self.ora.render()
    if self.tables is not None:
      want = _resample_tables.expected_frames(self.big.render(), *self.tables)
    np.testing.assert_array_equal(self.eng.render().cpu().numpy(), want, err_msg='%s render t=%d' % (self.what, self.t))
    self.launch(keeps)

  def close(self):
    self.eng.close()


def scripted_hits(n_envs, t):
  """Environment e is at position (t + 3 e) of SCRIPT at step t: different environments at different points in one launch."""
  return np.array([SCRIPT[(t + 3 * e) % len(SCRIPT)] for e in range(n_envs)], dtype=bool)


def never_hit(make_engine, monkeypatch, n_envs, what='never_hit', env=(), steps=8, tables=None, **scene):
  """Every click a miss: step 1 (the reset) resamples, step 2 fills, steps 3 and later copy.  tables(cfg): see Pair."""
  cfg, pool = build(n_envs, **scene)
  p = Pair(make_engine, monkeypatch, cfg, pool, what, env, tables=tables and tables(cfg))
  for _ in range(steps):
    p.step(False)
  T = p.tasks * n_envs
  assert (p.copied, p.filled, p.resampled) == ((steps - 2) * T, T, T)
  assert (p.kept, p.built) == ((steps - 1) * n_envs, n_envs)
  p.close()
  return p.frames


def hit_every_step(make_engine, monkeypatch, n_envs):
  """A sprite moves at every step: nothing is kept, nothing filled, nothing copied."""
  cfg, pool = build(n_envs)
  p = Pair(make_engine, monkeypatch, cfg, pool, 'hit_every_step')
  for _ in range(8):
    p.step(True)
  assert (p.copied, p.filled, p.kept) == (0, 0, 0)
  p.close()


def scripted(make_engine, monkeypatch, n_envs, what='scripted', env=(), cache=True, scribble=False, steps=16, tables=None):
  """SCRIPT, every environment at its own point of it.  `scribble`: the caller fills the whole frame buffer with 0xA5 before
  every launch -- every byte of every frame must be written by the launch itself.  tables(cfg): see Pair."""
  cfg, pool = build(n_envs)
  p = Pair(make_engine, monkeypatch, cfg, pool, what, env, cache=cache, tables=tables and tables(cfg))
  p.scribble = scribble
  for t in range(steps):
    p.step(scripted_hits(n_envs, t), keeps=None if cache or not any(k == 'SWB_NO_KEEP_LISTS' for k, _ in env) else False)
  if cache:
    assert p.copied > 0 and p.filled > p.tasks * n_envs and p.resampled > p.tasks * n_envs     # (every path, more than once)
  else:
    assert (p.copied, p.filled) == (0, 0)
  p.close()
  return p.frames


def episode_ends(make_engine, monkeypatch, n_envs):
  """Episodes of four steps inside one long still period: the step that resets builds and resamples, the next fills."""
  cfg, pool = build(n_envs, max_episode_length=4)
  p = Pair(make_engine, monkeypatch, cfg, pool, 'episode_ends')
  kinds = [int(p.step(False)['step_type'][0]) for _ in range(12)]
  assert kinds.count(_abi.STEP_FIRST) == 3
  T = p.tasks * n_envs
  assert (p.copied, p.filled, p.resampled) == (6 * T, 3 * T, 3 * T)
  p.close()


def alternating_buffers(make_engine, monkeypatch, n_envs):
  """Three frame buffers of the caller's take turns through swb_outputs::obs, the third 4 bytes off 16-byte alignment (the
  mover's dword path).  Each is filled with garbage before the launch that writes it: a copy never relies on its content."""
  cfg, pool = build(n_envs)
  p = Pair(make_engine, monkeypatch, cfg, pool, 'alternating_buffers')
  eng = p.eng
  shape, nbytes = tuple(eng.obs.shape), eng.obs.numel()
  raw = [torch.zeros(nbytes + 64, dtype=torch.uint8, device=eng.device) for _ in range(3)]
  bufs = []
  for i, r in enumerate(raw):
    off = (-r.data_ptr()) % 16 + (4 if i == 2 else 0)
    bufs.append(r[off:off + nbytes].view(shape))
  assert [b.data_ptr() % 16 for b in bufs] == [0, 0, 4]
  for t in range(14):
    b = bufs[t % 3]
    b.fill_(0x3C + t)
    eng.obs = b
    eng._outs.obs = b.data_ptr()
    p.step(scripted_hits(n_envs, t))
  assert p.copied > 0 and p.filled > 0
  p.close()


def call_between(make_engine, monkeypatch, n_envs, which):
  """reset, miss (fills), miss (copies) | the call | three misses that must neither copy a stale frame nor lose one."""
  cfg, pool = build(n_envs)
  p = Pair(make_engine, monkeypatch, cfg, pool, 'between ' + which, canvases=(which == 'upload_tables'))
  for _ in range(3):
    p.step(False)
  rebuilt = True
  fills = 2
  if which == 'render':            # a render of an unchanged state keeps, and copies: into the same buffer, scribbled first
    p.scribble = True
    p.render(True)
    p.render(True)
    rebuilt = False
  elif which == 'evaluate':        # lists nothing, counts nothing
    np.testing.assert_array_equal(p.eng.evaluate().cpu().numpy(), p.ora.evaluate())
    p.check_counts()
    rebuilt = False
  elif which == 'step_without_frame':
    p.step(True, render=False)
  elif which == 'set_positions':
    st = p.ora.state()
    x, y = st['x'].copy(), st['y'].copy()
    y[:, 0] = np.where(y[:, 0] < 0.5, y[:, 0] + 0.2, y[:, 0] - 0.2)
    p.ora.set_positions(x, y)
    p.eng.set_positions(x, y)
  elif which == 'sprite_setter':
    for e in range(0, n_envs, 2):
      p.ora.set_sprite_attr(e, 1, _abi.ATTR_SCALE, 0.2)
      p.eng.set_sprite_attr(e, 1, _abi.ATTR_SCALE, 0.2)
  elif which == 'trim':
    cap = p.eng.variant()['run_cap']
    assert p.eng.trim() < cap
  elif which == 'rollout_frames':  # frames of candidate states go through the engine's own lists and headers: all resampled
    M = 2
    acts = np.stack([actions(p.ora.state(), np.ones(n_envs, bool), motion=(0.9, 0.1 + 0.2 * m)) for m in range(M)], axis=1)[None]
    p.eng.rollout(acts)
    cand = p.eng.rollout_frames()['obs'].cpu().numpy()
    assert all((cand[:, m] != p.frames[-1]).any() for m in range(M))
    p.built += M * n_envs
    p.resampled += M * n_envs * p.tasks
    p.word[:] = 0
    p.check_counts()
  elif which == 'upload_tables':   # another family of tables (BICUBIC, the whole canvas), then the same tables once more: an
    # upload always makes lists and cached frames stale -- build and resample under the new tables, a fill, a copy, both times
    aa = cfg.anti_aliasing
    tabs = tuple(_resample_tables.tables(aa * n, n, 'bicubic') for n in (cfg.image_h, cfg.image_w))
    old = p.frames[-1]
    p.upload(*tabs)
    p.scribble = True
    p.step(False, keeps=False)
    assert (p.frames[-1] != old).any()                                  # (the same scene: the tables are what changed)
    p.step(False)
    p.step(False)
    assert p.word.tolist() == [2] * n_envs and p.filled == 2 * p.tasks * n_envs
    assert p.frames[-1].tobytes() == p.frames[-3].tobytes()
    p.upload(*tabs)
    fills = 3
  else:
    raise ValueError(which)
  p.scribble = True
  p.step(False, keeps=False if rebuilt else None)
  p.step(False)
  p.step(False)
  T = p.tasks * n_envs
  if rebuilt:      # the step after the call resampled everything; then a fill, then a copy
    assert p.word.tolist() == [2] * n_envs and p.filled == fills * T
  else:
    assert p.filled == T
  p.close()


def geometry(make_engine, monkeypatch, n_envs, which):
  """SCRIPT on the other ways a frame is cut into rectangles."""
  if which == 'two_column_groups':   # a 128-column image, the smallest with two: rectangles of 192-byte segments in 384-byte rows
    cfg, pool = build(n_envs, size=(128, 64))
    env = ()
  elif which == 'bands_default':     # what a small batch gets by itself: several bands
    cfg, pool = build(n_envs)
    env = ()
  elif which == 'one_band':
    cfg, pool = build(n_envs)
    env = (('SWB_BANDS', '1'),)
  elif which == 'band_tasks_8':      # every band a task of its own, filed under the copy cost where its environment copies
    cfg, pool = build(n_envs)
    env = (('SWB_BANDS', '8'), ('SWB_BAND_TASKS', '1'))
  elif which == 'background':        # no untouched rows
    cfg, pool = build(n_envs, bg=(7, 30, 110))
    env = ()
  else:
    raise ValueError(which)
  p = Pair(make_engine, monkeypatch, cfg, pool, which, env)
  v = p.eng.variant()
  if which == 'two_column_groups':
    assert v['n_column_groups'] == 2
  if which == 'bands_default':
    assert v['n_bands'] > 1
  if which == 'one_band':
    assert v['n_bands'] == 1
  if which == 'band_tasks_8':
    assert v['n_bands'] == 8
  p.scribble = True
  for t in range(12):
    p.step(scripted_hits(n_envs, t))
  assert p.copied > 0 and p.filled > 0
  p.close()


def switches(make_engine, monkeypatch, n_envs):
  """SWB_NO_FRAME_CACHE and SWB_NO_KEEP_LISTS: no cache, no copy, and every frame what it is with the cache."""
  with_cache = scripted(make_engine, monkeypatch, n_envs, 'switches: default')
  no_cache = scripted(make_engine, monkeypatch, n_envs, 'switches: SWB_NO_FRAME_CACHE', env=(('SWB_NO_FRAME_CACHE', '1'),), cache=False)
  monkeypatch.delenv('SWB_NO_FRAME_CACHE')
  no_keep = scripted(make_engine, monkeypatch, n_envs, 'switches: SWB_NO_KEEP_LISTS', env=(('SWB_NO_KEEP_LISTS', '1'),), cache=False)
  assert len(with_cache) == len(no_cache) == len(no_keep) == 16
  for a, b, c in zip(with_cache, no_cache, no_keep):
    assert a.tobytes() == b.tobytes() == c.tobytes()


def anti_aliasing_1(make_engine, monkeypatch, n_envs, paint):
  """anti_aliasing 1: the painting cover build (64 columns) and the fill kernel (128 columns) have no cache and count nothing."""
  cfg, pool = build(n_envs, aa=1, size=(64, 64) if paint else (128, 64))
  p = Pair(make_engine, monkeypatch, cfg, pool, 'anti_aliasing_1 paint=%s' % paint, cache=False)
  assert p.eng.variant()['paint_in_cover'] == (1 if paint else 0)
  for _ in range(6):
    p.step(False, keeps=False if paint else None)
  assert (p.copied, p.filled, p.resampled) == (0, 0, 0)
  p.close()
