"""Pillow's 8-bit resampling tables for every filter and source box, and the two-pass resample they drive, restated in numpy
(TEST INFRASTRUCTURE ONLY; no GPU, no Pillow import -- tests/test_resample_tables_cpu.py holds this module to Pillow itself).

`tables` is libImaging/Resample.c `precompute_coeffs` + `normalize_coeffs_8bpc`, written the way spriteworld_amd/lanczos.py writes
the one case the product uploads (LANCZOS, the whole canvas): per output index a window (xmin, count) of source pixels and `count`
weights filter((x + xmin - center + 0.5) / filterscale), normalised by their float64 running sum and rounded to 22-bit fixed
point.  Pillow holds the source box as float[4]: x0 and x1 are rounded to float32, and their difference is a float32 one.

`two_pass` is ImagingResample for 8-bit pixels: the horizontal pass first, a uint8 intermediate, then the vertical pass; per value
clip8(((1 << 21) + sum(pixel * k)) >> 22).

`canvases` gives the canvases a configuration draws before it shrinks them: an oracle.Engine on a copy of the configuration with
the image `anti_aliasing` times as large and anti_aliasing 1 paints them itself (vertices are (int)(canvas size * v) either way),
upside down as every frame is (np.flipud).  The frame any pair of tables must give is `expected_frames`.
"""
import ctypes as C
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
# output rows in flight per family of tables (filter, canvas pixels per output pixel; None: the whole canvas), at integer
# anti_aliasing: the families the tuned resample kernels accept (tests/test_resample_tables_cpu.py asserts every count)
REGIMES = {('lanczos', None): 6, ('lanczos', 0.9): 7, ('lanczos', 0.82): 8, ('bicubic', None): 4, ('bicubic', 0.9): 5,
           ('bilinear', None): 2, ('bilinear', 0.9): 3, ('hamming', None): 2, ('hamming', 0.9): 3, ('box', None): 1}
TOO_MANY = ('lanczos', 0.6)        # more than 8: the large-frame path only
# a = -0.5 in Pillow's bicubic_filter
_A = -0.5


def _box(x):
  return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
  x = abs(x)
  return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
  x = abs(x)
  if x == 0.0:
    return 1.0
  if x >= 1.0:
    return 0.0
  x = x * math.pi
  return math.sin(x) / x * (float(np.float32(0.54)) + float(np.float32(0.46)) * math.cos(x))    # (0.54f, 0.46f in Resample.c)


def _bicubic(x):
  x = abs(x)
  if x < 1.0:
    return ((_A + 2.0) * x - (_A + 3.0)) * x * x + 1
  if x < 2.0:
    return (((x - 5) * x + 8) * x - 4) * _A
  return 0.0


def _sinc(x):
  if x == 0.0:
    return 1.0
  x = x * math.pi
  return math.sin(x) / x


def _lanczos(x):
  if -3.0 <= x < 3.0:
    return _sinc(x) * _sinc(x / 3)
  return 0.0


# name -> (filter, support)
FILTERS = {'box': (_box, 0.5), 'bilinear': (_bilinear, 1.0), 'hamming': (_hamming, 1.0), 'bicubic': (_bicubic, 2.0),
           'lanczos': (_lanczos, 3.0)}


def tables(in_size, out_size, filter='lanczos', x0=0.0, x1=None):    # pylint: disable=redefined-builtin
  """Returns (bounds i32[out, 2] = (xmin, count), coeffs i32[out, ksize]) of `out_size` outputs from the source box [x0, x1) of
  `in_size` pixels (x1 None: in_size)."""
  fn, fsupport = FILTERS[filter]
  in0 = np.float32(x0)
  in1 = np.float32(in_size if x1 is None else x1)
  scale = float(in1 - in0) / out_size
  filterscale = max(scale, 1.0)
  support = fsupport * filterscale
  ksize = int(math.ceil(support)) * 2 + 1
  bounds = np.zeros((out_size, 2), dtype=np.int32)
  coeffs = np.zeros((out_size, ksize), dtype=np.int32)
  inv = 1.0 / filterscale
  for o in range(out_size):
    center = float(in0) + (o + 0.5) * scale
    xmin = max(int(center - support + 0.5), 0)
    count = min(int(center + support + 0.5), in_size) - xmin
    weights = [fn((x + xmin - center + 0.5) * inv) for x in range(count)]
    total = 0.0
    for w in weights:
      total += w
    for x, w in enumerate(weights):
      if total != 0.0:
        w = w / total
      coeffs[o, x] = int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS))
    bounds[o] = (xmin, count)
  return bounds, coeffs


def box(in_size, out_size, scale):
  """The source box every case uses per axis, `scale` canvas pixels per output pixel: (x0, x1), both float32 (None: whole canvas)."""
  if scale is None:
    return 0.0, None
  x0 = np.float32(0.07 * in_size + 0.3)
  x1 = np.float32(x0 + np.float32(scale * out_size))
  assert 0 <= x0 < x1 <= in_size, (in_size, out_size, scale, x0, x1)
  return float(x0), float(x1)


def family(in_size, out_size, filter='lanczos', scale=None):    # pylint: disable=redefined-builtin
  x0, x1 = box(in_size, out_size, scale)
  return tables(in_size, out_size, filter, x0, x1)


def rows_in_flight(bounds, in_size):
  """The most output rows whose windows are open at one canvas row, counted from the oldest that is not complete there: the count
  swb_upload_resample makes of a vertical table (`used`), without its limit."""
  ymin = bounds[:, 0].astype(np.int64)
  vend = ymin + bounds[:, 1] - 1
  used = 1
  for y in range(in_size):
    open_ = np.flatnonzero(vend >= y)
    rf = int(open_[0]) if len(open_) else len(vend)      # rows completed before canvas row y
    live = np.flatnonzero((ymin <= y) & (y <= vend))
    if len(live):
      used = max(used, int(live.max()) - rf + 1)
  return used


def monotone(bounds):
  ymin = bounds[:, 0].astype(np.int64)
  vend = ymin + bounds[:, 1] - 1
  return bool((np.diff(ymin) >= 0).all() and (np.diff(vend) >= 0).all())


def prefix_bytes(bounds, coeffs):
  """Bytes of the horizontal prefix table swb_upload_resample builds: per DISTINCT vector of running coefficient sums, count + 1
  words of four bytes."""
  seen = set()
  for (_, count), k in zip(bounds, coeffs):
    seen.add(tuple(np.concatenate([[0], np.cumsum(k[:count], dtype=np.int64)]).tolist()))
  return 4 * sum(len(v) for v in seen)


def upload_axis(eng, axis, out_size, tab, ksize=None):
  """swb_upload_resample of one axis on a live engine; returns the status (0: accepted)."""
  bounds, coeffs = (np.ascontiguousarray(a, dtype=np.int32) for a in tab)
  return eng.lib.swb_upload_resample(eng._h, int(axis), int(out_size), int(coeffs.shape[1] if ksize is None else ksize),    # pylint: disable=protected-access
                                     bounds.ctypes.data_as(C.c_void_p), coeffs.ctypes.data_as(C.c_void_p))


def upload(eng, tab_h, tab_v):
  """Both axes, paired with the image sizes as Engine.__init__ pairs them; raises the engine's error where one is refused."""
  for axis, out_size, tab in ((0, eng.cfg.image_h, tab_h), (1, eng.cfg.image_w, tab_v)):
    eng._check(upload_axis(eng, axis, out_size, tab))    # pylint: disable=protected-access


def _pass(src, tab):
  """One pass along axis 1 of src u8[A, in, 3] -> u8[A, out, 3]."""
  bounds, coeffs = tab
  out = np.empty((src.shape[0], len(bounds), src.shape[2]), dtype=np.uint8)
  src = src.astype(np.int64)
  for o, (xmin, count) in enumerate(bounds):
    acc = np.tensordot(src[:, xmin:xmin + count, :], coeffs[o, :count].astype(np.int64), axes=([1], [0]))
    out[:, o, :] = np.clip(((1 << (PRECISION_BITS - 1)) + acc) >> PRECISION_BITS, 0, 255)
  return out


def two_pass(canvas, tab_h, tab_v):
  """canvas u8[Hc, Wc, 3] -> u8[H, W, 3]: the horizontal pass with tab_h, a uint8 intermediate, the vertical pass with tab_v."""
  canvas = np.ascontiguousarray(canvas, dtype=np.uint8)
  tmp = _pass(canvas, tab_h)                                             # [Hc, W, 3]
  return np.ascontiguousarray(_pass(tmp.transpose(1, 0, 2), tab_v).transpose(1, 0, 2))


def canvas_config(cfg):
  """A copy of `cfg` that paints what `cfg` draws before it shrinks it."""
  big = type(cfg).from_buffer_copy(cfg)
  big.image_h, big.image_w, big.anti_aliasing = cfg.image_h * cfg.anti_aliasing, cfg.image_w * cfg.anti_aliasing, 1
  return big


def canvases(cfg, pool):
  """An oracle.Engine whose frames, stepped with the actions `cfg`'s engine is stepped with, are np.flipud of the canvases."""
  from oracle import oracle
  return oracle.Engine(canvas_config(cfg), pool)


def expected_frames(big_obs, tab_h, tab_v):
  """u8[N, Hc, Wc, 3] frames of `canvases` -> the frames u8[N, H, W, 3] an engine with these tables renders."""
  return np.stack([np.flipud(two_pass(np.flipud(c), tab_h, tab_v)) for c in big_obs])
