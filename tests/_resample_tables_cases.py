"""Every family of Pillow coefficient tables swb_upload_resample accepts (tests/test_emulated_resample_tables.py,
tests/test_gpu_resample_tables.py; DESIGN.md sections 3 and 24) -- the one place swb_resample_kernel<8> runs.

The engine itself uploads one family: LANCZOS over the whole canvas at an integer anti_aliasing, six output rows in flight,
swb_resample_kernel<6>, one prefix vector shared by all interior columns.  Here the tables of tests/_resample_tables.py -- five
filters, with and without a source box (fractional phases: a prefix vector per column; parts of the canvas no output sees), one
to eight rows in flight -- are uploaded over them after Engine.__init__, axis by axis as it pairs them, and every step is held to
  - tests/_parity.compare(frames=False) against the oracle: state, rewards, step types, success and error flags;
  - frames +-0 against tests/_resample_tables.expected_frames: numpy's two integer passes over the canvases a second oracle
    paints (tests/test_resample_tables_cpu.py holds both to Pillow and to the oracle's own renderer).
A family is (filter, canvas pixels per output pixel of the source box; None: the whole canvas), tests/_resample_tables.REGIMES
its rows in flight.  The engines never trim their lists by themselves unless the case says so.
"""
import re

import numpy as np

from spriteworld_amd import workloads
from tests import _frame_cache_cases
from tests import _parity
from tests import _resample_tables as rt

SWB_ERR_INVALID = -1      # include/swb.h
# name -> (workload, anti_aliasing): one column group on a 64-pixel canvas / the headline's geometry / two column groups, not square
GEOMETRIES = {'32x32_aa2': ('geom_32x32', 2), '64x64_aa5': ('cluster_s5', 5), '128x32_aa2': ('geom_128x32', 2)}
FAMILIES = tuple(rt.REGIMES)
MIXED = ((('lanczos', 0.82), ('bicubic', None)), (('bicubic', None), ('lanczos', 0.82)))
LARGE = {'large_frames_32x32': ('geom_32x32', 2, (('SWB_LARGE_FRAMES', '1'),), {'large_frames': 1, 'many_sprites': 0}),
         'many_sprites_s40': ('cluster_s40', 2, (), {'large_frames': 1, 'many_sprites': 1})}


def family_id(fam):
  return '%s_%s' % (fam[0], 'whole' if fam[1] is None else ('box%g' % fam[1]))


def tables_for(cfg, fam_h, fam_v):
  """(horizontal, vertical) tables of a configuration: the horizontal axis has cfg.image_h outputs (Engine.__init__)."""
  aa = cfg.anti_aliasing
  return (rt.family(aa * cfg.image_h, cfg.image_h, *fam_h), rt.family(aa * cfg.image_w, cfg.image_w, *fam_v))


class Run(object):
  """An engine with uploaded tables beside the oracle (state) and the oracle of its canvases (frames)."""

  def __init__(self, make_engine, workload, aa, n_envs, what, seed=2):
    from oracle import oracle
    self.cfg, self.pool, self.sample = workloads.build(workload, n_envs, episodes_per_env=2, seed=seed, anti_aliasing=aa)
    self.ora, self.big = oracle.Engine(self.cfg, self.pool), rt.canvases(self.cfg, self.pool)
    self.eng = make_engine(self.cfg, self.pool)
    self.eng.TRIM_AFTER = 0
    self.rng = np.random.default_rng(seed + 100)
    self.what, self.t, self.tabs = what, 0, None

  def upload(self, fam_h, fam_v):
    self.tabs = tables_for(self.cfg, fam_h, fam_v)
    rt.upload(self.eng, *self.tabs)

  def step(self, scribble=True):
    """One step of all three; the engine's frame buffer filled with garbage first: every byte must be written."""
    a = self.sample(self.rng)
    want, canv = self.ora.step(a, render=False), self.big.step(a)
    if scribble:
      self.eng.obs.fill_(0xA5)
    self.eng.step(a)
    got = self.eng.outputs_host()
    _parity.compare(self.t, self.ora, self.eng, want, got, frames=False, what=self.what)
    np.testing.assert_array_equal(canv['step_type'], want['step_type'], err_msg='%s canvases t=%d' % (self.what, self.t))
    frames = rt.expected_frames(canv['obs'], *self.tabs)
    diff = np.abs(got['obs'].astype(np.int16) - frames.astype(np.int16))
    assert diff.max() == 0, ('frame diff', self.what, self.t, int(diff.max()), int((diff > 0).sum()), np.argwhere(diff > 0)[:5].tolist())
    self.t += 1
    return frames

  def close(self):
    self.eng.close()


def shows_sprites(frames):
  """bool[N]: the frame has more colours than a background and one flat sprite (resampled edges)."""
  return np.array([len(np.unique(f.reshape(-1, 3), axis=0)) > 8 for f in frames])


def expected_vs(rows):
  return 6 if rows <= 6 else 8


def families(make_engine, geometry, fam_h, fam_v, n_envs, steps=3):
  """One pair of families on one geometry: the build of the resample kernel follows the VERTICAL rows in flight."""
  workload, aa = GEOMETRIES[geometry]
  r = Run(make_engine, workload, aa, n_envs, '%s h=%s v=%s' % (geometry, family_id(fam_h), family_id(fam_v)))
  r.upload(fam_h, fam_v)
  rows = rt.rows_in_flight(r.tabs[1][0], aa * r.cfg.image_w)
  assert rows == rt.REGIMES[fam_v], (rows, fam_v)
  v = r.eng.variant()
  assert v['large_frames'] == 0 and v['vs'] == expected_vs(rows), (rows, v)
  assert v['n_column_groups'] == (r.cfg.image_h + 63) // 64
  in_view = np.zeros(n_envs, dtype=bool)
  for _ in range(steps):
    in_view |= shows_sprites(r.step())
  assert in_view.sum() >= 2, in_view            # (a source box sees a part of the canvas: the seed puts sprites there)
  r.close()
  return rows, v['vs']


def bands(make_engine, monkeypatch, geometry, n_bands, band_tasks, n_envs, steps=3):
  """LANCZOS at 0.82 canvas pixels per output pixel, eight rows in flight, cut into bands: a band must start where the rows in
  flight are a multiple of eight.  Returns the number of bands the engine made of the `n_bands` asked for."""
  monkeypatch.setenv('SWB_BANDS', str(n_bands))
  monkeypatch.setenv('SWB_BAND_TASKS', str(band_tasks))
  workload, aa = GEOMETRIES[geometry]
  r = Run(make_engine, workload, aa, n_envs, '%s bands=%d band_tasks=%d' % (geometry, n_bands, band_tasks))
  r.upload(('lanczos', 0.82), ('lanczos', 0.82))
  assert rt.rows_in_flight(r.tabs[1][0], aa * r.cfg.image_w) == 8
  in_view = np.zeros(n_envs, dtype=bool)
  for _ in range(steps):
    in_view |= shows_sprites(r.step())
  assert in_view.sum() >= 2, in_view
  v = r.eng.variant()                                                   # (after a launch: the bands the tables allowed)
  assert v['vs'] == 8
  got = v['n_bands']
  assert 1 <= got <= n_bands
  if n_bands == 1:
    assert got == 1
  else:
    assert got > 1, 'no band start with a multiple of 8 rows in flight: %d bands asked for, 1 made' % n_bands
  r.close()
  return got


def _lanczos_082(cfg):
  return tables_for(cfg, ('lanczos', 0.82), ('lanczos', 0.82))


def kept_lists_and_frame_cache(make_engine, monkeypatch, n_envs, which):
  """tests/_frame_cache_cases.py's `never_hit` and `scripted` on swb_resample_kernel<8>: kept lists, fills and copies counted by
  the same model of the header word, the frames those of the uploaded tables."""
  checked = []

  def tables(cfg):
    tabs = _lanczos_082(cfg)
    assert rt.rows_in_flight(tabs[1][0], cfg.anti_aliasing * cfg.image_w) == 8
    checked.append(True)
    return tabs

  made, vs = [], set()

  def make(cfg, pool):
    eng = make_engine(cfg, pool)
    made.append(eng)
    step = eng.step

    def stepping(*args, **kwargs):                  # (the build every step of the script launches)
      vs.add(eng.variant()['vs'])
      return step(*args, **kwargs)

    eng.step = stepping
    return eng

  if which == 'never_hit':
    frames = _frame_cache_cases.never_hit(make, monkeypatch, n_envs, what='never_hit, eight rows in flight', steps=6, tables=tables)
  elif which == 'scripted':
    frames = _frame_cache_cases.scripted(make, monkeypatch, n_envs, what='scripted, eight rows in flight', scribble=True, steps=12, tables=tables)
  else:
    raise ValueError(which)
  assert checked and len(made) == 1 and vs == {8}
  assert shows_sprites(frames[0]).sum() >= 2      # (the source box sees the upper left of the scene: some of its sprites)


def large_paths(make_engine, monkeypatch, which, fam, n_envs, steps=3):
  """The large-frame kernels (forced on a small image; by themselves for more than 16 sprites) take the tables as they are: any
  number of rows in flight."""
  workload, aa, env, expect = LARGE[which]
  for k, v in env:
    monkeypatch.setenv(k, v)
  r = Run(make_engine, workload, aa, n_envs, '%s %s' % (which, family_id(fam)))
  v = r.eng.variant()
  for k, value in expect.items():
    assert v[k] == value, (k, v)
  r.upload(fam, fam)
  rows = rt.rows_in_flight(r.tabs[1][0], aa * r.cfg.image_w)
  assert rows == rt.REGIMES[fam] if fam in rt.REGIMES else rows > 8
  in_view = np.zeros(n_envs, dtype=bool)
  for _ in range(steps):
    in_view |= shows_sprites(r.step())
  assert in_view.sum() >= 2, in_view
  r.close()
  return rows


def _refused(r, message, axis, tab, out_size=None, ksize=None):
  sizes = (r.cfg.image_h, r.cfg.image_w, r.cfg.image_h)
  rc = rt.upload_axis(r.eng, axis, sizes[axis] if out_size is None else out_size, tab, ksize)
  text = r.eng.lib.swb_last_error().decode()
  assert rc == SWB_ERR_INVALID, (message, rc, text)
  assert re.search(message, text), (message, text)
  r.step()                                        # the tables the handle had: a refused upload changes nothing


def refusals(make_engine, n_envs):
  """Everything swb_upload_resample refuses on the tuned path, each with its message, and after each a step that renders +-0 with
  the tables uploaded before (BICUBIC with a source box horizontally, LANCZOS with another vertically: not the engine's own)."""
  workload, aa = GEOMETRIES['64x64_aa5']
  r = Run(make_engine, workload, aa, n_envs, 'refusals')
  r.upload(('bicubic', 0.9), ('lanczos', 0.9))
  assert shows_sprites(r.step()).sum() >= 2
  W, H, Wc, Hc = r.cfg.image_h, r.cfg.image_w, aa * r.cfg.image_h, aa * r.cfg.image_w
  assert (W, H) == (64, 64)
  good_h, good_v = tables_for(r.cfg, ('hamming', None), ('bilinear', 0.9))     # what a wrongly accepted upload would install

  def edited(tab, row, xmin=None, count=None):
    b, k = tab[0].copy(), tab[1].copy()
    if xmin is not None:
      b[row, 0] = xmin
    if count is not None:
      b[row, 1] = count
    return b, k

  ks_h, ks_v = good_h[1].shape[1], good_v[1].shape[1]
  _refused(r, r'horizontal table has 63 outputs, image width is 64', 0, (good_h[0][:63], good_h[1][:63]), out_size=63)
  _refused(r, r'vertical table has 65 outputs, image height is 64', 1, (np.concatenate([good_v[0], good_v[0][-1:]]), np.concatenate([good_v[1], good_v[1][-1:]])), out_size=65)
  _refused(r, r'axis must be 0 or 1', 2, good_h)
  _refused(r, r'bad horizontal bounds at 5$', 0, edited(good_h, 5, xmin=-1))
  _refused(r, r'bad vertical bounds at 7$', 1, edited(good_v, 7, xmin=-1))
  _refused(r, r'bad horizontal bounds at 63$', 0, edited(good_h, 63, xmin=Wc - good_h[0][63, 1] + 1))
  _refused(r, r'bad vertical bounds at 63$', 1, edited(good_v, 63, xmin=Hc - good_v[0][63, 1] + 1))
  _refused(r, r'bad horizontal bounds at 30$', 0, edited(good_h, 30, count=ks_h + 1))
  _refused(r, r'bad vertical bounds at 30$', 1, edited(good_v, 30, count=ks_v + 1))
  _refused(r, r'bad vertical bounds at 12$', 1, edited(good_v, 12, count=0))
  swapped = (good_v[0].copy(), good_v[1].copy())
  swapped[0][[20, 21]] = swapped[0][[21, 20]]
  swapped[1][[20, 21]] = swapped[1][[21, 20]]
  assert not rt.monotone(swapped[0])
  _refused(r, r'vertical windows are not monotone', 1, swapped)
  many = rt.family(Hc, H, *rt.TOO_MANY)
  assert rt.rows_in_flight(many[0], Hc) > 8
  _refused(r, r'more than 8 output rows in flight at canvas row \d+$', 1, many)
  # 64 columns of 200 taps, every column's running sums its own: 64 * 201 words, more than the 32 KB the prefix table may take
  wide = (np.zeros((64, 2), np.int32), np.zeros((64, 200), np.int32))
  wide[0][:, 0] = np.arange(64)
  wide[0][:, 1] = 200
  wide[1][:] = ((1 << rt.PRECISION_BITS) // 200) + np.arange(64)[:, None]
  assert rt.prefix_bytes(*wide) == 4 * 64 * 201 and Wc >= 63 + 200
  _refused(r, r'horizontal prefix table too large \(12864 entries\)', 0, wide)
  r.close()
