"""Point sets on the device, the part that needs no device (include/winmad_rt.h
wr_points_*): the symbols, the refusals that come before any HIP
call, the wrappers' validation, the brute force of tests/_points_ref.py pinned
to the reference's KdTree (cr_kat_vkd restates searchInRadius), and the photon
script of tests/_script_photons.py over the oracle's own primitives.  The
device answers are checked in tests/test_gpu_points.py.
"""
import ctypes as C

import numpy as np
import pytest

import _oracle
import _points_ref
import _scenes
import _script_photons
from winmad_rt import native

NEW = ("wr_points_build_dev", "wr_points_info_get", "wr_points_free", "wr_points_count_dev",
       "wr_points_in_radius_dev", "wr_points_knn_dev")


def test_symbols_are_exported_and_the_version_stays():
    L = native.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in native.EXPORTS
    assert L.wr_api_version() == 8


@pytest.mark.parametrize("n", [1, -1])
def test_null_context_and_negative_sizes_are_refused_before_any_device_call(n):
    """The context comes first, then n / nq: with a context that is not null but
    is never dereferenced (a negative size is refused before it is looked at)
    the answer is WR_E_ARG as well, and the message names the call."""
    L = native.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)  # never read
    fake = C.c_void_p(buf.ctypes.data)  # stands for a context / an index; only compared with NULL when n < 0
    out = C.c_void_p()
    for ctx in ((None,) if n > 0 else (None, fake)):
        calls = {
            "wr_points_build_dev": lambda: L.wr_points_build_dev(ctx, p, n, 1.0, C.byref(out)),
            "wr_points_count_dev": lambda: L.wr_points_count_dev(ctx, fake, p, n, 1.0, None, p),
            "wr_points_in_radius_dev": lambda: L.wr_points_in_radius_dev(ctx, fake, p, n, 1.0, None, p, 4, p),
            "wr_points_knn_dev": lambda: L.wr_points_knn_dev(ctx, fake, p, n, 4, 1.0, p, p, p),
        }
        for name, call in calls.items():
            assert call() == native.WR_E_ARG, name
            assert name in L.wr_last_error().decode(), name
    assert not buf.any() and not out.value
    assert L.wr_points_info_get(None, None) == native.WR_E_ARG
    L.wr_points_free(None)  # a no-op


def test_wrappers_refuse_bad_arguments_before_any_device_call():
    """No context and no device: every wrapper raises before it touches either."""
    torch = pytest.importorskip("torch")
    ctx = native.Context.__new__(native.Context)  # no wr_create: validation comes first
    idx = native.PointsIndex.__new__(native.PointsIndex)
    idx.ctx, idx.h = ctx, None
    good = torch.zeros((6, 3), dtype=torch.float32)
    bad = {"numpy": np.zeros((6, 3), np.float32), "float64": good.double(),
           "shape": torch.zeros((6, 4), dtype=torch.float32),
           "non_contiguous": torch.zeros((6, 6), dtype=torch.float32)[:, ::2], "cpu_tensor": good}
    for name, x in bad.items():
        for call in (lambda: ctx.points_index_t(x, 1.0), lambda: idx.count_t(x, radius=1.0),
                     lambda: idx.in_radius_t(x, radius=1.0), lambda: idx.knn_t(x, 4, 1.0)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError, match="float32"):
        native._dev_tensor(bad["float64"], "q", (None, 3), "float32", None)
    with pytest.raises(ValueError, match="shape"):
        native._dev_tensor(bad["shape"], "q", (None, 3), "float32", None)
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell"):
            native.PointsIndex(ctx, good, cell)
    # both or neither of radius and radii (refused before q's device is looked at)
    radii = torch.zeros((6,), dtype=torch.float32)
    for kw in ({}, {"radius": 1.0, "radii": radii}):
        with pytest.raises(ValueError, match="exactly one"):
            idx.count_t(good, **kw)
        with pytest.raises(ValueError, match="exactly one"):
            idx.in_radius_t(good, **kw)
    with pytest.raises(ValueError, match="radii"):  # (through the helper the wrappers use: q is a host tensor here)
        native._dev_tensor(torch.zeros((5,), dtype=torch.float32), "radii", (6,), "float32", None)
    with pytest.raises(ValueError, match="radius"):
        idx.count_t(good, radius=-1.0)
    for k in (0, 65, -1, 2.0):
        with pytest.raises(ValueError, match="k must"):
            idx.knn_t(good, k, 1.0)
    with pytest.raises(ValueError, match="max_sqr_dist"):
        idx.knn_t(good, 4, float("nan"))


def _clouds():
    """(name, points): 1, 2, 65 and 1,000 points -- uniform, clustered, with duplicates."""
    rng = np.random.default_rng(18)
    out = [("one", rng.random((1, 3))), ("two", rng.random((2, 3))), ("uniform65", rng.random((65, 3))),
           ("uniform1000", rng.random((1000, 3)))]
    centres = rng.random((8, 3))
    out.append(("clustered1000", centres[rng.integers(0, 8, 1000)] + rng.normal(0, 0.01, (1000, 3))))
    dup = rng.random((500, 3))
    out.append(("duplicates1000", np.concatenate([dup, dup[rng.integers(0, 500, 500)]])))
    out.append(("duplicates65", np.repeat(rng.random((5, 3)), 13, 0)))
    return [(name, np.ascontiguousarray(p, np.float32)) for name, p in out]


@pytest.mark.parametrize("name,pts", _clouds(), ids=[c[0] for c in _clouds()])
def test_points_ref_is_the_reference_kd_tree(name, pts):
    """cr_kat_vkd builds the reference's point KD tree and runs searchInRadius
    per query: its count and index sum equal _points_ref's, query by query, so a
    gate against _points_ref is a gate against the reference's KdTree."""
    rng = np.random.default_rng(5)
    n = len(pts)
    q = np.concatenate([pts[rng.integers(0, n, 100)] + rng.normal(0, 0.02, (100, 3)).astype(np.float32),
                        rng.random((100, 3)).astype(np.float32)]).astype(np.float32)
    q[:20] = pts[rng.integers(0, n, 20)]  # queries on points: d2 = 0
    found = 0
    for r in (0.01, 0.07, 0.25):
        out = np.zeros((len(q), 4), np.int64)
        _oracle.lib().cr_kat_vkd(_oracle.fptr(pts), n, _oracle.fptr(np.ascontiguousarray(q)), len(q), r,
                                 out.ctypes.data_as(C.POINTER(C.c_int64)))
        cnt, lists = _points_ref.radius_sets(q, pts, np.float32(r))
        assert np.array_equal(out[:, 0], cnt), (name, r)
        assert np.array_equal(out[:, 1], [int(l.astype(np.int64).sum()) for l in lists]), (name, r)
        found += int(cnt.sum())
        # the k-nearest form agrees with the radius form: the points with d2 < r*r, nearest first
        ki, kd, kc = _points_ref.knn(q, pts, 8, np.float32(r) * np.float32(r))
        d2 = _points_ref.sqr_dist(q, pts)
        assert np.array_equal(kc, np.minimum((d2 < np.float32(r) * np.float32(r)).sum(1), 8))
        for j in range(0, len(q), 17):
            c = kc[j]
            assert np.all(np.diff(kd[j, :c]) >= 0) and np.all(ki[j, c:] == -1) and not kd[j, c:].any()
            assert np.array_equal(kd[j, :c], d2[j, ki[j, :c]])
            ties = np.diff(kd[j, :c]) == 0
            assert np.all(np.diff(ki[j, :c])[ties] > 0)
    assert found > 0


def test_points_ref_ignores_what_is_not_finite():
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [0.1, 0, 0], [np.inf, 0, 0]], np.float32)
    q = np.array([[0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [3e38, 0, 0]], np.float32)
    cnt, lists = _points_ref.radius_sets(q, pts, 0.5)
    assert cnt.tolist() == [2, 0, 0, 0] and lists[0].tolist() == [0, 2]
    ki, kd, kc = _points_ref.knn(q, pts, 3, 1e30)
    assert kc.tolist() == [2, 0, 0, 0] and ki[0].tolist() == [0, 2, -1]


def test_photon_script_over_the_oracle():
    """tests/_script_photons.py over the oracle's primitives and the numpy brute
    force: Cornell box 32 x 24, 4,096 particles.  Finite, non-negative, and lit somewhere."""
    sc = _oracle.Scene(_scenes.cbox(32, 24))
    est, stored = _script_photons.estimate(_script_photons.OraclePhotons(sc, 77), 4096, 32, 24, 16, 0.25)
    assert est.dtype == np.float32 and est.shape == (32 * 24, 3)
    assert 0 < stored <= 4096
    assert np.isfinite(est).all() and (est >= 0).all()
    assert (est.sum(1) > 0).sum() > 32 * 24 // 4
