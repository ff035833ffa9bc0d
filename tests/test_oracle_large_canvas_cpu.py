"""The oracle's Pillow restatements at the canvas sizes of the large-frame path (1280 and 2560 px: 256 x 256 images at
anti_aliasing 5 and 10, the reference demo's renderer), against the installed Pillow -- the spec the large-frame kernels
are held to."""
import math

import numpy as np
import pytest

from oracle import oracle
from spriteworld_amd import lanczos, shapes

PIL = pytest.importorskip('PIL')
from PIL import Image, ImageDraw  # noqa: E402


def _sprite_polygon(rng, W, H):
  verts, offs = shapes.packed_table()
  si = rng.integers(len(offs) - 1)
  v = verts[offs[si]:offs[si + 1]]
  sc = rng.choice([0.05, 0.13, 0.2, 0.4])
  th = math.radians(float(rng.integers(0, 360)))
  a, b = math.cos(th), math.sin(th)
  px, py = rng.uniform(-0.1, 1.1, 2)
  return np.stack([a * sc * v[:, 0] - b * sc * v[:, 1] + px,
                   b * sc * v[:, 0] + a * sc * v[:, 1] + py], 1) * np.array([W, H])


@pytest.mark.parametrize('W,H', [(1280, 1280), (2560, 2560), (2560, 640), (1024, 4096)])
def test_polygon_fill_equals_pillow_on_large_canvases(W, H):
  rng = np.random.default_rng(W + H)
  im = Image.new('RGB', (W, H))
  mine = np.zeros((H, W, 3), np.uint8)
  for k in range(24):                       # painted over each other, back to front, as a scene is
    P = _sprite_polygon(rng, W, H)
    ink = tuple(int(c) for c in rng.integers(0, 256, 3))
    ImageDraw.Draw(im).polygon([tuple(q) for q in P], fill=ink)
    oracle.fill_polygon(W, H, np.trunc(P).astype(np.int32), ink, image=mine)
  assert np.array_equal(np.array(im), mine)


@pytest.mark.parametrize('size,aa', [(256, 5), (256, 10), (128, 10), (512, 4)])
def test_lanczos_resize_equals_pillow_on_large_canvases(size, aa):
  rng = np.random.default_rng(size * aa)
  src = np.zeros((aa * size, aa * size, 3), np.uint8)
  src[:] = rng.integers(0, 256, 3)
  for _ in range(20):                       # constant-colour regions, as a rendered canvas is
    y0, y1 = sorted(rng.integers(0, aa * size, 2))
    x0, x1 = sorted(rng.integers(0, aa * size, 2))
    src[y0:y1, x0:x1] = rng.integers(0, 256, 3)
  src[:aa * 8] = rng.integers(0, 256, size=(aa * 8, aa * size, 3), dtype=np.uint8)    # and a band of noise
  ref = np.array(Image.fromarray(src, 'RGB').resize((size, size), resample=Image.LANCZOS))
  assert np.array_equal(ref, oracle.resample(src, size, size))


@pytest.mark.parametrize('sizes', [(1280, 256), (2560, 256), (4096, 1024), (4096, 256)])
def test_host_coefficient_tables_equal_oracle_on_large_canvases(sizes):
  b1, k1 = oracle.lanczos_tables(*sizes)
  b2, k2 = lanczos.resample_tables(*sizes)
  assert np.array_equal(b1, b2) and np.array_equal(k1, k2)


# ---- at the limits of the large-frame path (4096 canvas pixels in either direction) and with 64 sprites: what the GPU tests of
# ---- tests/test_gpu_many_sprites_large_frames.py lean on the oracle for
def _canvas_like(rng, W, H):
  src = np.zeros((H, W, 3), np.uint8)
  src[:] = rng.integers(0, 256, 3)
  for _ in range(20):                       # constant-colour regions, as a rendered canvas is
    y0, y1 = sorted(rng.integers(0, H, 2))
    x0, x1 = sorted(rng.integers(0, W, 2))
    src[y0:y1, x0:x1] = rng.integers(0, 256, 3)
  nh = max(H // 32, 1)
  src[:nh] = rng.integers(0, 256, size=(nh, W, 3), dtype=np.uint8)    # and a band of noise
  return src


@pytest.mark.parametrize('canvas,out', [((4096, 4096), (256, 256)), ((4096, 256), (1024, 64)), ((256, 4096), (64, 1024))])
def test_lanczos_resize_equals_pillow_at_4096_pixels(canvas, out):
  """Anti_aliasing 16 (windows of 97 taps) on a square, anti_aliasing 4 on a 4096 px wide and on a 4096 px tall canvas."""
  src = _canvas_like(np.random.default_rng(sum(canvas)), *canvas)
  ref = np.array(Image.fromarray(src, 'RGB').resize(out, resample=Image.LANCZOS))
  assert np.array_equal(ref, oracle.resample(src, *out))


def test_polygon_fill_equals_pillow_at_4096_pixels_square():
  W = H = 4096
  rng = np.random.default_rng(4096)
  im = Image.new('RGB', (W, H))
  mine = np.zeros((H, W, 3), np.uint8)
  for k in range(16):
    P = _sprite_polygon(rng, W, H)
    ink = tuple(int(c) for c in rng.integers(0, 256, 3))
    ImageDraw.Draw(im).polygon([tuple(q) for q in P], fill=ink)
    oracle.fill_polygon(W, H, np.trunc(P).astype(np.int32), ink, image=mine)
  assert np.array_equal(np.array(im), mine)


def test_scene_of_64_sprites_equals_pillow_on_a_1280_pixel_canvas():
  """A whole frame as the reference's renderer makes it -- the background pasted, 64 sprites painted back to front with
  ImageDraw.polygon on the 1280 px canvas, Image.resize(LANCZOS) to 256 x 256, np.flipud -- equals oracle.render_sprites."""
  from tests import _many_sprites_cases as cases
  cfg, pool, _ = cases.scene(64, (256, 256), 5, 2, episodes_per_env=1, ragged=False, seed=7)
  size = np.array([1280, 1280])
  for e in range(2):
    canvas = Image.new('RGB', tuple(size), cases.BG)
    draw = ImageDraw.Draw(canvas)
    for s in range(64):
      v = oracle.vertices(int(pool.shape[e, s]), pool.scale[e, s], pool.angle[e, s], pool.x[e, s], pool.y[e, s])
      draw.polygon([tuple(q) for q in size * v], fill=tuple(int(c) for c in pool.rgb[e, s, :3]))
    ref = np.flipud(np.array(canvas.resize((256, 256), resample=Image.LANCZOS)))
    got = oracle.render_sprites(cfg, pool.x[e], pool.y[e], pool.shape[e], pool.scale[e], pool.cos_a[e], pool.sin_a[e], pool.rgb[e, :, :3])
    assert np.array_equal(ref, got), e
