"""Brute force for the point-set calls (include/winmad_rt.h wr_points_*), in
numpy float32 with the operation order of the definition:

  d2(q, p) = dx*dx + dy*dy + dz*dz, d = q - p per component, every step a
             float32 operation (Vector3::sqrLength; no dot / einsum, which
             could fuse or reorder)
  radius:    point i is reported iff sqrt(d2) < r (numpy's float32 sqrt is
             correctly rounded, as sqrtf)
  k-nearest: the points with d2 < max_sqr_dist, the k smallest by (d2, index)

A point with a non-finite coordinate is never reported; a query with one
reports nothing.  tests/test_points_host.py pins these functions to the
reference's KdTree (cr_kat_vkd).
"""
import numpy as np

F = np.float32


def sqr_dist(q, pts):
    """(nq, n) float32 d2 of every query against every point."""
    q = np.ascontiguousarray(q, F).reshape(-1, 3)
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = q[:, None, 0] - pts[None, :, 0]
        dy = q[:, None, 1] - pts[None, :, 1]
        dz = q[:, None, 2] - pts[None, :, 2]
        d2 = dx * dx + dy * dy + dz * dz
    assert d2.dtype == F
    return d2


def _usable(q, pts):
    q = np.asarray(q, F).reshape(-1, 3)
    pts = np.asarray(pts, F).reshape(-1, 3)
    return np.isfinite(q).all(1)[:, None] & np.isfinite(pts).all(1)[None, :]


def radius_mask(q, pts, radius):
    """(nq, n) bool: point i reported for query j.  radius: a scalar or (nq,)."""
    d2 = sqr_dist(q, pts)
    r = np.broadcast_to(np.asarray(radius, F), (d2.shape[0],))[:, None]
    with np.errstate(invalid="ignore"):
        m = np.sqrt(d2) < r
    return m & _usable(q, pts)


def radius_sets(q, pts, radius):
    """(count (nq,) int32, lists): lists[j] the ascending indices of query j."""
    m = radius_mask(q, pts, radius)
    return m.sum(1).astype(np.int32), [np.nonzero(row)[0].astype(np.int32) for row in m]


def knn(q, pts, k, max_sqr_dist):
    """(index (nq, k) int32, sqr_dist (nq, k) float32, count (nq,) int32) as
    wr_points_knn_dev defines them: unused slots -1 and 0."""
    d2 = sqr_dist(q, pts)
    nq, n = d2.shape
    with np.errstate(invalid="ignore"):
        ok = (d2 < F(max_sqr_dist)) & _usable(q, pts)
    index = np.full((nq, k), -1, np.int32)
    sqr = np.zeros((nq, k), F)
    count = np.zeros(nq, np.int32)
    for j in range(nq):
        cand = np.nonzero(ok[j])[0]
        order = np.lexsort((cand, d2[j, cand]))[:k]  # by d2, then by index
        c = len(order)
        index[j, :c] = cand[order]
        sqr[j, :c] = d2[j, cand[order]]
        count[j] = c
    return index, sqr, count
