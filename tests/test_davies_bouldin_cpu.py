"""The oracle's Davies-Bouldin score against a numpy restatement of scikit-learn 1.7.2's function against scikit-learn itself,
over the whole input space of the ABI: up to 64 sprites, up to 63 clusters, label values up to 127, both position dtypes,
and every degeneracy the reference turns into an exception.

Three links, each bit for bit (score, ValueError, exact zero):
  model(dots='blas')     == scikit-learn          everywhere: the restatement is faithful;
  oracle                 == model(dots='explicit') everywhere: the oracle is that function with the documented dot orders;
  model(dots='explicit') == model(dots='blas')    for float32 positions and for float64 positions with fewer than 12 clusters:
                                                  the domain on which the project claims parity with the reference.
Beyond that domain (float64, 12 clusters or more) the BLAS numpy ships evaluates some entries of the centroid Gram matrix
in another order; which ones depends on the BLAS build and the CPU, so nothing is asserted there about the third link."""
import collections

import numpy as np
import pytest

from tests import _clustering_cases as cc
from tests import _davies_bouldin_model as model
from tests import _parity

metrics = pytest.importorskip('sklearn.metrics')


def _sklearn(X, labels):
  try:
    score = metrics.davies_bouldin_score(X, labels)
  except ValueError:
    return 2, float('nan')
  return (1 if score == 0.0 else 0), score


def _same(a, b):
  """(error, score) pairs equal: the error code, and the bits of the score where there is one."""
  return a[0] == b[0] and (a[0] == 2 or _parity.bits(a[1]) == _parity.bits(b[1]))


def _regular_path_zero(X, labels):
  """The score is exactly 0.0 and neither np.allclose early-out of scikit-learn fired."""
  classes = np.unique(labels)
  lab = np.searchsorted(classes, labels)
  cen = np.array([X[lab == k].mean(axis=0) for k in range(len(classes))], dtype=float)
  intra = np.array([np.average(model._member_distances(X[lab == k], X[lab == k].mean(axis=0), 'blas')) for k in range(len(classes))])
  return not (np.allclose(intra, 0) or np.allclose(model._centroid_distances(cen, 'blas'), 0))


def check(g, seen):
  """One geometry through scikit-learn, both modes of the model and the oracle; counts what it was into `seen`."""
  keep = g['label'] >= 0
  X = g['pos'][keep].astype(np.float32 if g['f32'] else np.float64)
  labels = g['label'][keep].astype(np.int64)
  f = cc.facts(g)
  what = (g['family'], g['f32'], f)
  sk, blas, explicit, ora = _sklearn(X, labels), model.davies_bouldin(X, labels, 'blas'), \
      model.davies_bouldin(X, labels, 'explicit'), cc.oracle_score(g)
  assert _same(blas, sk), ('model(blas) != scikit-learn', what, blas, sk)
  assert _same(ora, explicit), ('oracle != model(explicit)', what, ora, explicit)
  claimed = g['f32'] or f['k'] < 12
  if claimed:
    assert _same(explicit, blas), ('model(explicit) != model(blas) inside the claimed domain', what, explicit, blas)
  dt = 'f32' if g['f32'] else 'f64'
  seen['cases'] += 1
  seen[dt] += 1
  seen['error_%d' % ora[0]] += 1
  seen[(dt, 'k', f['k'])] += 1
  seen['outside_claim'] += int(not claimed and ora[0] != 2)
  seen['outside_claim_differs'] += int(not claimed and not _same(explicit, blas))
  if ora[0] == 1:
    seen['zero_regular_path' if _regular_path_zero(X, labels) else 'zero_early_out'] += 1
  if ora[0] != 2:
    seen['unassigned'] += int(f['m'] < f['n'])
    seen['label_32_up'] += int(f['top_label'] >= 32)
    seen['label_96_up'] += int(f['top_label'] >= 96)
    seen['k_33_up'] += int(f['k'] >= 33)
    seen['k_22_up'] += int(f['k'] >= 22)
    seen['k_is_n_minus_1'] += int(f['k'] == f['m'] - 1)
    seen['k_is_2'] += int(f['k'] == 2)
    for size in (8, 9, 16, 17):
      seen['cluster_of_%d_beside_singletons' % size] += int(f['largest'] == size and f['singletons'] > 0)
    seen['cluster_of_40_up_beside_singletons'] += int(f['largest'] >= 40 and f['singletons'] > 0)
  return ora


def _floors(seen, floors):
  """Every class of case occurred: floors of about half of what the seeded sweep yields (each sweep prints its counts, `pytest -s`)."""
  for key, floor in floors.items():
    assert seen[key] >= floor, (key, seen[key], floor)


def test_random_sweep():
  """n = 3 .. 64, k = 2 .. n - 1, label values from 0 .. 127 without replacement, some sprites unassigned, both dtypes."""
  rng = np.random.default_rng(20)
  seen = collections.Counter()
  for i in range(1600):
    check(cc.geometry(rng, 'random', f32=(i % 2 == 0), n_max=64 if i % 4 < 3 else 16), seen)
  print(sorted((k, v) for k, v in seen.items() if not isinstance(k, tuple)))
  _floors(seen, FLOORS_RANDOM)


# what seed 20 yields: cases 1600, f32 800, f64 800, error_0 1574, error_2 26 (k = m: every spare sprite unassigned),
# unassigned 1049, label_32_up 1555, label_96_up 1313, k_22_up 343, k_33_up 181, k_is_2 175, k_is_n_minus_1 190,
# outside_claim (float64, 12 clusters or more) 241 -- of which 42 differ between the two modes on numpy 2.2.6's bundled BLAS
FLOORS_RANDOM = dict(cases=1600, f32=800, f64=800, error_0=1500, error_2=10, unassigned=500, label_32_up=800, label_96_up=650,
                     k_22_up=170, k_33_up=90, k_is_2=85, k_is_n_minus_1=95, outside_claim=120)


def test_shaped_sweeps():
  """Clusters of 8, 9, 16, 17 and 40 or more members beside singletons (numpy's pairwise sum leaves its sequential branch at
  8 and unrolls by 8; a singleton's member distance takes the dot kernel's order); k = n - 1; k = 2; every k from 2 to 63 in
  each dtype."""
  rng = np.random.default_rng(21)
  seen = collections.Counter()
  for i in range(600):
    check(cc.geometry(rng, 'big_and_singletons', f32=(i % 2 == 0), n_max=64 if i % 3 else 16), seen)
  for i in range(200):
    check(cc.geometry(rng, 'k_n_minus_1', f32=(i % 2 == 0), n_max=64), seen)
    check(cc.geometry(rng, 'k2', f32=(i % 2 == 0), n_max=64), seen)
  for k in range(2, 64):
    for i in range(8):
      check(cc.geometry(rng, 'every_k', f32=(i % 2 == 0), n_max=64, k=k), seen)
  print(sorted((k, v) for k, v in seen.items() if not isinstance(k, tuple)))
  for dt in ('f32', 'f64'):
    for k in range(2, 64):
      assert seen[(dt, 'k', k)] >= 4, (dt, k, seen[(dt, 'k', k)])
  _floors(seen, FLOORS_SHAPED)


# what seed 21 yields: 1496 cases, none an error; cluster of 8 / 9 / 16 / 17 / 40 or more beside singletons 148 / 139 / 76 / 85 /
# 83, k_is_n_minus_1 236, k_is_2 317, k_33_up 362, outside_claim 291
FLOORS_SHAPED = dict(cluster_of_8_beside_singletons=70, cluster_of_9_beside_singletons=70, cluster_of_16_beside_singletons=40,
                     cluster_of_17_beside_singletons=40, cluster_of_40_up_beside_singletons=40, k_is_n_minus_1=200, k_is_2=200,
                     k_33_up=180, error_0=1496, outside_claim=150)


def test_degenerate_sweeps():
  """Every cluster on a point of its own; all sprites on one point; one cluster collapsed beside spread ones; a quarter grid
  on which two clusters share a centroid exactly; all sprites within 10**e of one point, e = -12 .. -6; the label failures
  (k = 1, k = m, no sprite assigned, no sprite at all)."""
  rng = np.random.default_rng(22)
  seen = collections.Counter()
  by_family = collections.defaultdict(collections.Counter)
  for i in range(300):
    f32, n_max = i % 2 == 0, 64 if i % 3 else 16
    for family in ('all_collapsed', 'one_point', 'one_collapsed', 'quarter_grid', 'k1', 'k_equals_m', 'none_assigned', 'empty'):
      by_family[family][check(cc.geometry(rng, family, f32, n_max), seen)[0]] += 1
    for e in range(-12, -5):
      by_family['near_point'][check(cc.geometry(rng, 'near_point', f32, n_max, e=e), seen)[0]] += 1
  for i in range(1500):             # where float64 scores fall to exactly 0.0 through the regular path
    by_family['near_1e-8'][check(cc.geometry(rng, 'near_point', False, 8, e=rng.uniform(-8.6, -7.4)), seen)[0]] += 1
  print(sorted((k, v) for k, v in seen.items() if not isinstance(k, tuple)), {k: dict(v) for k, v in by_family.items()})
  # what seed 22 yields, as {error code: cases}: all_collapsed {1: 203, 0: 97}, one_point {1: 236, 0: 64} (coincident members
  # need not be at distance exactly 0 from their centroid: a float32 mean rounds, and the expanded formula leaves up to about
  # 1e-8, just beyond np.allclose's bound -- scikit-learn, the model and the oracle then return the same meaningless score),
  # one_collapsed {0: 300}, quarter_grid {0: 220, 1: 80} (1: the two clusters that share a centroid are the only ones),
  # near_point {1: 1101, 0: 999}, the 1500 float64 scenes around 1e-8 {1: 913, 0: 587}
  for family in ('all_collapsed', 'one_point'):
    assert by_family[family][1] >= 150 and by_family[family][2] == 0, family      # ZeroDivisionError
  for family in ('k1', 'k_equals_m', 'none_assigned', 'empty'):
    assert by_family[family] == {2: 300}, family                    # ValueError, every one
  assert by_family['one_collapsed'] == {0: 300}
  assert by_family['quarter_grid'][0] >= 150 and by_family['quarter_grid'][1] >= 40 and by_family['quarter_grid'][2] == 0
  assert by_family['near_point'][0] >= 500 and by_family['near_point'][1] >= 500
  _floors(seen, FLOORS_DEGENERATE)


# what seed 22 yields: zero_early_out 2531, zero_regular_path 2 (both among the 1500 float64 scenes around 1e-8: the recorded
# fixtures below do not hang on this), error_2 1200
FLOORS_DEGENERATE = dict(zero_early_out=1500, zero_regular_path=1, error_2=1200)


@pytest.mark.parametrize('i', range(len(cc.ZERO_SCORE_FIXTURES)))
def test_exact_zero_through_the_regular_path_is_an_error(i):
  """The recorded scenes (hex floats, no seed): scikit-learn returns exactly 0.0 with neither early-out taken; the oracle flags
  SWB_ENV_ERR_DB_ZERO, as for the early-outs, instead of a score whose reciprocal is an infinite reward."""
  g = cc.fixture_geometry(i)
  X, labels = g['pos'], g['label'].astype(np.int64)
  assert metrics.davies_bouldin_score(X, labels) == 0.0
  assert _regular_path_zero(X, labels)
  assert model.davies_bouldin(X, labels, 'blas') == (1, 0.0) and model.davies_bouldin(X, labels, 'explicit') == (1, 0.0)
  assert cc.oracle_score(g) == (1, 0.0)


@pytest.mark.parametrize('i', range(len(cc.ZERO_SCORE_FIXTURES)))
def test_reference_raises_zero_division_on_the_fixtures(i):
  """The unmodified reference's Clustering.reward on the same scenes: ZeroDivisionError at `1. / score` (tasks.py:215)."""
  from oracle import ref_harness
  if not ref_harness.reference_available():
    pytest.skip('reference tree not present')
  ref_harness.load_reference()
  from spriteworld import factor_distributions as distribs
  from spriteworld import sprite, tasks
  g = cc.fixture_geometry(i)
  values = sorted(set(int(v) for v in g['label']))
  task = tasks.Clustering([distribs.Continuous('c0', v / 128., (v + 1) / 128.) for v in values])
  sprites = [sprite.Sprite(x=float(x), y=float(y), c0=(int(v) + 0.5) / 128.) for (x, y), v in zip(g['pos'], g['label'])]
  assert np.array([s.position for s in sprites]).dtype == np.float64
  with pytest.raises(ZeroDivisionError):
    task.reward(sprites)
  with pytest.raises(ZeroDivisionError):
    task.success(sprites)
