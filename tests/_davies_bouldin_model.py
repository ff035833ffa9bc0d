"""scikit-learn 1.7.2 `davies_bouldin_score`, restated line by line in numpy (TEST INFRASTRUCTURE ONLY).

The function and what it calls (LabelEncoder, check_number_of_labels, pairwise_distances -> euclidean_distances with its
float32 upcast path, row_norms) are short; this file writes them out with nothing between the caller and the arithmetic, so
that the three length-2 dot products they hide can be switched:

  dots='blas'      np.einsum and numpy matmul themselves, as scikit-learn calls them: whatever order the BLAS numpy was built
                   with takes.  This mode must equal scikit-learn bit for bit (tests/test_davies_bouldin_cpu.py).
  dots='explicit'  the orders oracle/sw_oracle.c documents (norm2, dot2_hi, dot2_lo) with an exactly rounded fused
                   multiply-add.  This mode must equal the oracle and the kernels bit for bit.

Where the two modes agree, the oracle equals the reference; where they do not, the difference is the BLAS build's."""
import math

import numpy as np


def fma(a, b, c):
  """round(a * b + c), one rounding: from exact integer arithmetic (int / int is correctly rounded), or math.fma where the
  interpreter has it."""
  if hasattr(math, 'fma'):
    return math.fma(a, b, c)
  (na, da), (nb, db), (nc, dc) = float(a).as_integer_ratio(), float(b).as_integer_ratio(), float(c).as_integer_ratio()
  num = na * nb * dc + nc * da * db
  if num == 0:      # an exact zero: +0.0 under round-to-nearest unless product and addend are both -0.0
    return -0.0 if math.copysign(1.0, a) * math.copysign(1.0, b) < 0 and math.copysign(1.0, c) < 0 else 0.0
  return num / (da * db * dc)


_fma = np.frompyfunc(fma, 3, 1)


def norm2(a):
  """row_norms(a, squared=True) for rows of two: a0*a0 + a1*a1, two products and a sum, each rounded."""
  return a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]


def dot2_hi(a, b):
  """fma(a1, b1, a0*b0) for every pair of rows -> [len(a), len(b)]."""
  return _fma(a[:, None, 1], b[None, :, 1], a[:, None, 0] * b[None, :, 0]).astype(np.float64)


def dot2_lo(a, b):
  """fma(a0, b0, a1*b1) for every pair of rows -> [len(a), len(b)]."""
  return _fma(a[:, None, 0], b[None, :, 0], a[:, None, 1] * b[None, :, 1]).astype(np.float64)


def _row_norms(a, dots):
  return np.einsum('ij,ij->i', a, a) if dots == 'blas' else norm2(a)


def _members_dot_centroid(x, c, dots):
  """x @ c.T for x [n, 2] and c [1, 2], float64: one member takes the dot kernel's order, two or more the gemv kernel's."""
  if dots == 'blas':
    return x @ c.T
  return dot2_hi(x, c) if len(x) == 1 else dot2_lo(x, c)


def _gram(c, dots):
  """c @ c.T for the centroids [k, 2], float64."""
  return c @ c.T if dots == 'blas' else dot2_hi(c, c)


def _member_distances(cluster, centroid, dots):
  """pairwise_distances(cluster_k, [centroid]): euclidean_distances by the expanded formula, in the dtype of the positions."""
  y = np.asarray([centroid])                                      # check_pairwise_arrays: float32 if both are, else float64
  if cluster.dtype == np.float32 and y.dtype == np.float32:
    # _euclidean_distances_upcast (one chunk): float64 arithmetic, the result stored as float32
    xc, yc = cluster.astype(np.float64), y.astype(np.float64)
    d = -2 * _members_dot_centroid(xc, yc, dots)
    d += _row_norms(xc, dots)[:, None]
    d += _row_norms(yc, dots)[None, :]
    distances = d.astype(np.float32)
  else:
    xc, yc = cluster.astype(np.float64), y.astype(np.float64)
    distances = -2 * _members_dot_centroid(xc, yc, dots)
    distances += _row_norms(xc, dots)[:, None]
    distances += _row_norms(yc, dots)[None, :]
  np.maximum(distances, 0, out=distances)
  return np.sqrt(distances, out=distances)


def _centroid_distances(centroids, dots):
  """pairwise_distances(centroids): X is Y, float64."""
  xx = _row_norms(centroids, dots)[:, None]
  distances = -2 * _gram(centroids, dots)
  distances += xx
  distances += xx.T
  np.maximum(distances, 0, out=distances)
  np.fill_diagonal(distances, 0)
  return np.sqrt(distances, out=distances)


def davies_bouldin(X, labels, dots='blas'):
  """(error, score) of davies_bouldin_score(X, labels).  error: 2 where scikit-learn raises ValueError (score nan), 1 where the
  score it returns is exactly 0.0 -- by an early-out or by the regular path: the reference's `1. / score` raises
  ZeroDivisionError on either -- else 0."""
  assert dots in ('blas', 'explicit'), dots
  X, labels = np.asarray(X), np.asarray(labels)
  if X.ndim != 2 or X.shape[0] == 0:                              # check_X_y
    return 2, math.nan
  classes = np.unique(labels)                                     # LabelEncoder.fit_transform
  labels = np.searchsorted(classes, labels)
  n_samples, n_labels = X.shape[0], len(classes)
  if not 1 < n_labels < n_samples:                                # check_number_of_labels
    return 2, math.nan
  intra_dists = np.zeros(n_labels)
  centroids = np.zeros((n_labels, len(X[0])), dtype=float)
  for k in range(n_labels):
    cluster_k = X[labels == k]
    centroid = cluster_k.mean(axis=0)
    centroids[k] = centroid
    intra_dists[k] = np.average(_member_distances(cluster_k, centroid, dots))
  centroid_distances = _centroid_distances(centroids, dots)
  if np.allclose(intra_dists, 0) or np.allclose(centroid_distances, 0):
    return 1, 0.0
  centroid_distances[centroid_distances == 0] = np.inf
  combined_intra_dists = intra_dists[:, None] + intra_dists
  scores = np.max(combined_intra_dists / centroid_distances, axis=1)
  score = float(np.mean(scores))
  return (1 if score == 0.0 else 0), score
