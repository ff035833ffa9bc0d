"""tests/_resample_tables.py held to Pillow and to the oracle (CPU; pins the helper the resample-table cases stand on, not the
engine): its tables and two passes are Pillow's Image.resize for every filter and source box, its canvases are the oracle's, and
every family of tables the cases upload has the number of output rows in flight its case is about."""
import numpy as np
import pytest

from spriteworld_amd import lanczos
from spriteworld_amd import workloads
from tests import _resample_tables as rt

# (image width, image height, anti_aliasing)
SIZES = ((32, 32, 2), (64, 64, 5), (128, 32, 2), (16, 48, 3))
# output rows in flight per (filter, canvas pixels per output pixel), stated here a second time on purpose: the figures the cases
# rely on (tests/_resample_tables.REGIMES) must be these
REGIMES = {('lanczos', None): 6, ('lanczos', 0.9): 7, ('lanczos', 0.82): 8, ('bicubic', None): 4, ('bicubic', 0.9): 5,
           ('bilinear', None): 2, ('bilinear', 0.9): 3, ('hamming', None): 2, ('hamming', 0.9): 3, ('box', None): 1}


def _images(rng, wc, hc):
  noise = rng.integers(0, 256, size=(hc, wc, 3), dtype=np.uint8)
  blocks = rng.integers(0, 2, size=(hc // 5 + 1, wc // 7 + 1, 3), dtype=np.uint8) * 255
  blocky = np.kron(blocks, np.ones((5, 7, 1), dtype=np.uint8))[:hc, :wc]
  return (('random', noise), ('blocky', np.ascontiguousarray(blocky)))


@pytest.mark.parametrize('w,h,aa', SIZES)
@pytest.mark.parametrize('name', sorted(rt.FILTERS))
def test_two_pass_is_pillow_resize(name, w, h, aa):
  Image = pytest.importorskip('PIL.Image')
  resample = getattr(Image.Resampling, name.upper())
  rng = np.random.default_rng(w * 1000 + h * 10 + aa)
  wc, hc = aa * w, aa * h
  for scale in (None, 0.9, 0.82, (1 + aa) / 2.0):
    x0, x1 = rt.box(wc, w, scale)
    y0, y1 = rt.box(hc, h, scale)
    tab_h, tab_v = rt.tables(wc, w, name, x0, x1), rt.tables(hc, h, name, y0, y1)
    pil_box = None if scale is None else (x0, y0, x1, y1)
    for kind, src in _images(rng, wc, hc):
      want = np.array(Image.fromarray(src).resize((w, h), resample=resample, box=pil_box))
      got = rt.two_pass(src, tab_h, tab_v)
      diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
      assert diff.max() == 0, (name, (w, h, aa), scale, kind, int(diff.max()), int((diff > 0).sum()))


@pytest.mark.parametrize('n,m', [(64, 32), (320, 64), (256, 128), (640, 128), (48, 16), (300, 100), (7, 7)])
def test_whole_canvas_lanczos_is_the_product_table(n, m):
  got, want = rt.tables(n, m), lanczos.resample_tables(n, m)
  for g, w in zip(got, want):
    assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


@pytest.mark.parametrize('name,aa', [('geom_32x32', 2), ('cluster_s5', 5)])
def test_canvases_and_two_pass_are_the_oracle_renderer(name, aa):
  """The harness by itself: canvases shrunk with the tables the product uploads are the oracle's frames."""
  from oracle import oracle
  cfg, pool, sample = workloads.build(name, 3, episodes_per_env=2, seed=2, anti_aliasing=aa)
  ora, big = oracle.Engine(cfg, pool), rt.canvases(cfg, pool)
  tab_h, tab_v = rt.tables(aa * cfg.image_h, cfg.image_h), rt.tables(aa * cfg.image_w, cfg.image_w)
  rng = np.random.default_rng(11)
  for t in range(4):
    a = sample(rng)
    want, canv = ora.step(a), big.step(a)
    for k in ('step_type', 'success'):
      np.testing.assert_array_equal(canv[k], want[k], err_msg='%s t=%d' % (k, t))
    assert canv['obs'].shape == (3, aa * cfg.image_w, aa * cfg.image_h, 3)
    np.testing.assert_array_equal(rt.expected_frames(canv['obs'], tab_h, tab_v), want['obs'], err_msg='t=%d' % t)
    assert len(np.unique(want['obs'].reshape(-1, 3), axis=0)) > 2                  # (not a flat frame)


@pytest.mark.parametrize('out,aa', [(32, 2), (64, 5), (128, 2)])
def test_regimes(out, aa):
  """Rows in flight per family, on every axis length the engine cases use: no case passes by never reaching its subject."""
  n = aa * out
  seen = {}
  for (name, scale), want in REGIMES.items():
    bounds, coeffs = rt.family(n, out, name, scale)
    seen[name, scale] = rt.rows_in_flight(bounds, n)
    assert bounds[:, 1].min() >= 1 and bounds[:, 0].min() >= 0 and (bounds[:, 0] + bounds[:, 1]).max() <= n, (name, scale)
    assert rt.monotone(bounds), (name, scale)
    assert rt.prefix_bytes(bounds, coeffs) < 32 * 1024, (name, scale)
  assert seen == REGIMES == rt.REGIMES
  assert rt.TOO_MANY == ('lanczos', 0.6)
  bounds, coeffs = rt.family(n, out, *rt.TOO_MANY)
  assert rt.rows_in_flight(bounds, n) > 8 and rt.monotone(bounds) and bounds[:, 1].min() >= 1
  assert rt.prefix_bytes(bounds, coeffs) < 32 * 1024


def test_rows_in_flight_counts_from_the_oldest_open_row():
  """Hand-made windows: three rows open at canvas row 4 (rows 1..3, row 0 complete), and a gap no row sees."""
  bounds = np.array([[0, 3], [2, 3], [3, 2], [4, 4], [9, 2]], dtype=np.int32)
  assert rt.rows_in_flight(bounds, 12) == 3
  assert rt.monotone(bounds)
  assert not rt.monotone(bounds[[0, 2, 1, 3, 4]])
  coeffs = np.array([[1, 2, 3, 0], [1, 2, 3, 0], [4, 5, 0, 0], [1, 1, 1, 1], [4, 5, 0, 0]], dtype=np.int32)
  assert rt.prefix_bytes(bounds, coeffs) == 4 * (4 + 3 + 5)                      # three distinct vectors
