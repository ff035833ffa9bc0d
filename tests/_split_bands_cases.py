"""Scenes for split bands (tests/test_emulated_split_bands.py, tests/test_gpu_split_bands.py).

A handle in split-bands mode builds its lists for B bands; an environment whose frame is copied files one WHOLE task per column
group, one that resamples or fills files its B band tasks when the launch's decision word says split and one whole task
otherwise.  The word a launch reads was written by the launch before it: split when that launch had at most SWB_SPLIT_WHEN
frames that resampled or filled.  Every case steps beside oracle.Engine through the bar of tests/_parity.py at every step --
frames +-0 -- and holds swb_list_stats, swb_frame_stats (FRAMES, not waves) and swb_split_stats to a model driven by the
oracle's step types and the script's clicks: the model of the header word of tests/_frame_cache_cases.py, plus the decision word.

The scene, SCRIPT, `scripted_hits` and BETWEEN are those of tests/_frame_cache_cases.py; the forced mode is SWB_SPLIT_BANDS=B.
"""
import numpy as np

from spriteworld_amd import _abi
from tests import _frame_cache_cases as fc
from tests import _resample_tables
from tests import _resample_tables_cases

ALWAYS = 2 ** 31 - 1
PLACED_24_ROWS_OF_8 = 6       # bands a 24-row image at anti_aliasing 5 takes of eight asked for (cannot_honour)
BETWEEN = fc.BETWEEN


class Pair(fc.Pair):
  """tests/_frame_cache_cases.py's pair with the decision word: `prev` is the number of frames that resampled or filled in the
  last rendering launch of the live state (to begin with: all of them), `when` the threshold."""

  def __init__(self, make_engine, monkeypatch, cfg, pool, what, bands, when, env=(), **kw):
    env = (('SWB_SPLIT_BANDS', str(bands)), ('SWB_SPLIT_WHEN', str(when))) + tuple(env)
    fc.Pair.__init__(self, make_engine, monkeypatch, cfg, pool, what, env, **kw)
    v = self.eng.variant()
    assert v['n_bands'] == 1 and v['split_bands'] == min(bands, cfg.image_h), v
    self.ncg = v['n_column_groups']
    assert self.tasks == self.ncg                       # (frames: the nominal one band)
    self.when = when
    self.prev = self.N * self.ncg
    self.whole = self.bands = self.whole_copies = 0
    self.lagged = 0                                     # launches that split while more frames resampled than `when`
    self.scribble = True                                # the caller's buffer is garbage before every launch

  def splits(self):
    return self.when > 0 and self.prev <= self.when        # (a threshold of 0: never)

  def placed(self):
    return self.eng.variant()['split_bands']            # (after a launch: the bands the tables allowed)

  def launch(self, keeps):
    split = self.splits()
    fc.Pair.launch(self, keeps)                         # (moves self.word; holds list_stats and frame_stats)
    busy = int((self.word != 2).sum())
    self.whole_copies += self.ncg * (self.N - busy)
    if split:
      self.bands += self.placed() * self.ncg * busy
      self.lagged += int(busy * self.ncg > self.when)
    else:
      self.whole += self.ncg * busy
    self.prev = busy * self.ncg
    self.check_split()

  def view_launches(self, n):
    """n launches on a state view: every frame resamples, under the word the next live launch will read; nothing moves it."""
    if self.splits():
      self.bands += n * self.placed() * self.ncg * self.N
    else:
      self.whole += n * self.ncg * self.N
    self.check_split()

  def check_split(self):
    got, want = self.eng.split_stats(), (self.whole, self.bands, self.whole_copies)
    assert got == want, (self.what, self.t, got, want)


def thresholds(make_engine, monkeypatch, n_envs, bands, which, tables=None, what=None, steps=12, **scene):
  """which = 'always' / 'never': SCRIPT under SWB_SPLIT_WHEN huge / 0 -- band tasks only / whole resampling tasks over lists that
  carry band starts.  'half': the threshold is half the batch and every fourth step hits all environments but two, the others
  hit two: most environments build, fill, copy, copy -- the word flips, and lags by one launch (the step that hits many is read
  the word of a launch in which two frames resampled)."""
  cfg, pool = fc.build(n_envs, **scene)
  when = {'always': ALWAYS, 'never': 0, 'half': n_envs // 2}[which]
  p = Pair(make_engine, monkeypatch, cfg, pool, what or 'thresholds %s B=%d' % (which, bands), bands, when, tables=tables and tables(cfg))
  e = np.arange(n_envs)
  for t in range(steps):
    p.step(fc.scripted_hits(n_envs, t) if which != 'half' else (e < n_envs - 2 if t % 4 == 0 else e < 2))
  assert p.whole_copies > 0
  if which == 'always':
    assert p.whole == 0 and p.bands > 0
  elif which == 'never':
    assert p.bands == 0 and p.whole > 0
  else:
    assert p.whole > 0 and p.bands > 0 and p.lagged >= 2
  placed = p.placed()
  p.close()
  return placed


def all_reset(make_engine, monkeypatch, n_envs, bands):
  """Episodes of four steps in a still period under a threshold of half the batch: the launches before a reset copy, the word
  says split, and the step that resets EVERY environment files bands x n_envs band tasks."""
  cfg, pool = fc.build(n_envs, max_episode_length=4)
  p = Pair(make_engine, monkeypatch, cfg, pool, 'all_reset', bands, n_envs // 2)
  before = None
  for t in range(12):
    was = p.bands
    want = p.step(False)
    if t > 0 and (want['step_type'] == _abi.STEP_FIRST).all():
      before = p.bands - was
      assert before == p.placed() * n_envs, (t, before)
  assert before is not None and p.lagged >= 2
  p.close()


def two_column_groups(make_engine, monkeypatch, n_envs, bands):
  placed = thresholds(make_engine, monkeypatch, n_envs, bands, 'half', what='two_column_groups', size=(128, 128))
  assert placed == bands


def band_starts(bounds, bands, vs):
  """The first output rows of the bands a vertical table (`bounds`: (ymin, count) per output row) allows when `bands` are asked
  for -- worked out here from the table alone: band b wants row b * rows / bands and takes the nearest row (the later one first
  at equal distance) behind the band before it at whose first canvas row the output rows still open, counted from the oldest,
  are a multiple of `vs` (the band's oldest row then accumulates in slot 0); a band that finds no such row is left out."""
  rows = len(bounds)
  ymin = [int(b[0]) for b in bounds]
  vend = [int(b[0] + b[1] - 1) for b in bounds]

  def oldest_open(o):
    f = o
    while f > 0 and vend[f - 1] >= ymin[o]:
      f -= 1
    return f

  starts = [0]
  for b in range(1, bands):
    want = b * rows // bands
    for d in range(rows):
      ok = [c for c in (want + d, want - d) if starts[-1] < c < rows and oldest_open(c) % vs == 0]
      if ok:
        starts.append(ok[0])
        break
  return starts


def cannot_honour(make_engine, monkeypatch, n_envs, bands=8):
  """A 24-row image at anti_aliasing 5 (LANCZOS: six rows in flight) has no eight band starts at which the rows in flight are a
  multiple of six: the engine places the bands the table allows -- worked out here from the table, and pinned: 6 --, and the
  counts follow the number placed."""
  cfg, pool = fc.build(n_envs, size=(24, 24))
  tab_v = _resample_tables.tables(cfg.anti_aliasing * cfg.image_h, cfg.image_h, 'lanczos')[0]
  assert _resample_tables.rows_in_flight(tab_v, cfg.anti_aliasing * cfg.image_h) <= 6
  expected = len(band_starts(tab_v, bands, 6))
  p = Pair(make_engine, monkeypatch, cfg, pool, 'cannot_honour', bands, ALWAYS)
  for t in range(8):
    p.step(fc.scripted_hits(n_envs, t))
  placed = p.placed()
  assert placed == expected == PLACED_24_ROWS_OF_8, (placed, expected)
  assert p.bands > 0 and p.whole_copies > 0
  p.close()
  return placed


def eight_rows_in_flight(make_engine, monkeypatch, n_envs, bands, which):
  """swb_resample_kernel<8> (LANCZOS at 0.82 canvas pixels per output pixel): band starts align to eight rows in flight."""
  vs = set()

  def tables(cfg):
    tabs = _resample_tables_cases.tables_for(cfg, ('lanczos', 0.82), ('lanczos', 0.82))
    assert _resample_tables.rows_in_flight(tabs[1][0], cfg.anti_aliasing * cfg.image_w) == 8
    return tabs

  def make(cfg, pool):
    eng = make_engine(cfg, pool)
    step = eng.step

    def stepping(*args, **kwargs):
      vs.add(eng.variant()['vs'])
      return step(*args, **kwargs)

    eng.step = stepping
    return eng

  placed = thresholds(make, monkeypatch, n_envs, bands, which, tables=tables, what='eight rows in flight, %s' % which)
  assert vs == {8} and placed > 1, (vs, placed)


def call_between(make_engine, monkeypatch, n_envs, which, bands=4):
  """tests/_frame_cache_cases.py's calls between steps, in split mode under a threshold of half the batch: reset (whole), miss
  (whole: fills), miss (copies) | the call | three misses."""
  cfg, pool = fc.build(n_envs)
  p = Pair(make_engine, monkeypatch, cfg, pool, 'between ' + which, bands, n_envs // 2, canvases=(which == 'upload_tables'))
  for _ in range(3):
    p.step(False)
  assert (p.whole, p.bands, p.whole_copies) == (2 * n_envs, 0, n_envs) and p.splits()
  rebuilt = True
  if which == 'render':
    p.render(True)
    p.render(True)
    rebuilt = False
  elif which == 'evaluate':
    np.testing.assert_array_equal(p.eng.evaluate().cpu().numpy(), p.ora.evaluate())
    p.check_counts()
    p.check_split()
    rebuilt = False
  elif which == 'step_without_frame':   # no second kernel: the host hands the word on
    p.step(True, render=False)
    p.check_split()
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
  elif which == 'rollout_frames':       # launches on a state view: all resampled, in bands (the word says split), the word kept
    M = 2
    acts = np.stack([fc.actions(p.ora.state(), np.ones(n_envs, bool), motion=(0.9, 0.1 + 0.2 * m)) for m in range(M)], axis=1)[None]
    p.eng.rollout(acts)
    cand = p.eng.rollout_frames()['obs'].cpu().numpy()
    assert all((cand[:, m] != p.frames[-1]).any() for m in range(M))
    p.built += M * n_envs
    p.resampled += M * n_envs * p.tasks
    p.word[:] = 0
    p.check_counts()
    p.view_launches(M)
  elif which == 'upload_tables':
    aa = cfg.anti_aliasing
    tabs = tuple(_resample_tables.tables(aa * n, n, 'bicubic') for n in (cfg.image_h, cfg.image_w))
    p.upload(*tabs)
    p.step(False, keeps=False)
    p.step(False)
    p.step(False)
    p.upload(*tabs)
  else:
    raise ValueError(which)
  bands_were = p.bands
  p.step(False, keeps=False if rebuilt else None)
  if rebuilt:                            # every environment builds while the word says split
    assert p.bands - bands_were == p.placed() * n_envs
  p.step(False)
  p.step(False)
  assert p.word.tolist() == [2] * n_envs
  p.close()


def mode_absent(make_engine, monkeypatch, n_envs, which):
  """Where the mode must not be: variant() says so, swb_split_stats refuses, and the frames are still the oracle's."""
  env, scene, cache = (), {}, True
  if which == 'anti_aliasing_1':
    scene, cache = dict(aa=1, size=(128, 64)), False
  elif which == 'no_frame_cache':
    env, cache = (('SWB_NO_FRAME_CACHE', '1'),), False
  elif which == 'bands_set':
    env = (('SWB_BANDS', '2'),)
  elif which == 'small_batch':            # the existing rule: a small batch takes several bands by itself, and is not forced
    pass
  else:
    raise ValueError(which)
  if which != 'small_batch':
    env = env + (('SWB_SPLIT_BANDS', '4'),)
  cfg, pool = fc.build(n_envs, **scene)
  p = fc.Pair(make_engine, monkeypatch, cfg, pool, 'mode_absent ' + which, env, cache=cache)
  v = p.eng.variant()
  assert v['split_bands'] == 0, v
  if which == 'small_batch':
    assert v['n_bands'] > 1, v
  if which == 'bands_set':
    assert v['n_bands'] == 2, v
  try:
    p.eng.split_stats()
  except Exception as e:  # pylint: disable=broad-except
    assert 'split' in str(e), e
  else:
    raise AssertionError('swb_split_stats on a handle without the mode')
  for t in range(6):
    p.step(fc.scripted_hits(n_envs, t))
  assert p.eng.variant()['split_bands'] == 0
  p.close()
