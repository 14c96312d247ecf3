"""Point sets on the GPU (include/winmad_rt.h wr_points_*).

The gate is equality with the brute force of tests/_points_ref.py, which
tests/test_points_host.py pins to the reference's KdTree: counts equal, every
query's index list equal as a sorted list, k-nearest index and count equal and
sqr_dist equal bit for bit.  Nothing is excluded: the definition leaves no tie
open.  Shapes are the smallest at which each piece can go wrong.
"""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import _oracle
import _points_ref
import _scenes
import _script_photons
from winmad_rt import native

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
F = np.float32

_state = {}


def ctx():
    if "ctx" not in _state:
        s = native.Scene(_scenes.torus(64, 64))
        _state["ctx"] = (s, native.Context(s, 0))
    return _state["ctx"][1]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def lists_of(offset, index):
    offset, index = host(offset), host(index)
    return [index[offset[j]:offset[j + 1]] for j in range(len(offset) - 1)]


def check_radius(idx, pts, q, radius=None, radii=None):
    """count_t and in_radius_t against the brute force; returns the lists in the index's order."""
    want_cnt, want = _points_ref.radius_sets(q, pts, radius if radii is None else radii)
    kw = {"radius": radius} if radii is None else {"radii": dev(np.asarray(radii, F))}
    tq = dev(q)
    cnt = host(idx.count_t(tq, **kw))
    assert cnt.dtype == np.int32 and np.array_equal(cnt, want_cnt), np.argwhere(cnt != want_cnt)[:5].ravel()
    offset, index = idx.in_radius_t(tq, **kw)
    assert np.array_equal(host(offset), np.concatenate([[0], np.cumsum(want_cnt, dtype=np.int64)]))
    got = lists_of(offset, index)
    for j, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(np.sort(g), w), (j, g, w)
    return got


def check_knn(idx, pts, q, k, max_sqr_dist):
    wi, wd, wc = _points_ref.knn(q, pts, k, max_sqr_dist)
    gi, gd, gc = (host(t) for t in idx.knn_t(dev(q), k, float(max_sqr_dist)))
    assert np.array_equal(gc, wc), np.argwhere(gc != wc)[:5].ravel()
    assert np.array_equal(gi, wi), np.argwhere(gi != wi)[:5]
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), np.argwhere(gd != wd)[:5]
    return gi, gd, gc


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_sizes(n):
    rng = np.random.default_rng(100 + n)
    pts = rng.random((n, 3)).astype(F)
    with ctx().points_index_t(dev(pts), 0.1) as idx:
        info = idx.info()
        assert info["n"] == n and info["cell"] == F(0.1) and info["buckets"] >= 2 * n and info["max_bucket"] <= n
        assert info["device_bytes"] >= 16 * n
        if n:
            assert np.array_equal(np.array(info["origin"], F), pts.min(0))
        for nq in (0, 1, 65, 257):
            q = rng.random((nq, 3)).astype(F)
            if nq and n:
                q[0] = pts[0]
            check_radius(idx, pts, q, radius=0.15)
            check_knn(idx, pts, q, 8, 0.09)


def test_all_points_identical():
    """One bucket holds everything; d2 = 0 at a query there; the k-nearest order is by index."""
    pts = np.tile(np.array([[0.3, -0.7, 0.2]], F), (130, 1))
    q = np.array([[0.3, -0.7, 0.2], [0.3, -0.7, 0.25], [5, 5, 5]], F)
    with ctx().points_index_t(dev(pts), 0.1) as idx:
        assert idx.info()["max_bucket"] == 130
        check_radius(idx, pts, q, radius=0.1)
        gi, gd, gc = check_knn(idx, pts, q, 64, 1.0)
        assert gi[0].tolist() == list(range(64)) and not gd[0].any() and gc.tolist() == [64, 64, 0]


# ------------------------------------------------------------------ 2. strictness
def test_strict_inequalities():
    pts = np.zeros((1, 3), F)
    below = np.nextafter(F(0.5), F(0))
    q = np.array([[0.5, 0, 0], [below, 0, 0], [0, -0.5, 0], [0, 0, -below]], F)
    with ctx().points_index_t(dev(pts), 0.5) as idx:
        got = check_radius(idx, pts, q, radius=0.5)
        assert [len(g) for g in got] == [0, 1, 0, 1]
        _, _, gc = check_knn(idx, pts, q, 1, 0.25)
        assert gc.tolist() == [0, 1, 0, 1]


# ------------------------------------------------------------------ 3. cell boundaries and signs
def test_cell_boundaries_and_signs():
    cell = F(0.25)
    m = np.arange(5)
    g = np.stack(np.meshgrid(m, m, m, indexing="ij"), -1).reshape(-1, 3)
    pts = (F(-0.5) + g.astype(F) * cell).astype(F)  # origin + m * cell exactly, negative coordinates included
    vals = []
    for b in (F(-0.5), F(-0.25), F(0.0), F(0.25)):
        vals += [b, np.nextafter(b, F(-np.inf)), np.nextafter(b, F(np.inf))]
    v = np.array(vals, F)
    q = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    with ctx().points_index_t(dev(pts), float(cell)) as idx:
        assert idx.info()["origin"] == (-0.5, -0.5, -0.5)
        for r in (0.25, 0.1, float(np.nextafter(F(0.25), F(1)))):
            check_radius(idx, pts, q, radius=r)
        check_knn(idx, pts, q, 9, 0.0625)
        check_knn(idx, pts, q[::7], 64, 1.0)


# ------------------------------------------------------------------ 4. shared buckets
def test_shared_buckets_report_every_point_once():
    """4,096 points in 64 tight clusters over 10^6 cells: distinct cells share
    buckets and rows wrap in cx.  Equal sorted lists mean no point twice, none lost."""
    rng = np.random.default_rng(4)
    centres = rng.uniform(0, 1e6, (64, 3))
    pts = (centres[np.arange(4096) % 64] + rng.normal(0, 1.5, (4096, 3))).astype(F)
    q = (pts[::8] + rng.normal(0, 0.5, (512, 3))).astype(F)
    with ctx().points_index_t(dev(pts), 1.0) as idx:
        got = check_radius(idx, pts, q, radius=2.0)
        assert sum(len(g) for g in got) > 2000
        check_knn(idx, pts, q, 16, 16.0)


# ------------------------------------------------------------------ 5. wide and narrow
def test_wide_and_narrow_radii():
    rng = np.random.default_rng(5)
    pts = rng.random((300, 3)).astype(F)
    q = np.concatenate([pts[:40], rng.random((60, 3)).astype(F)])
    cell = 0.05
    with ctx().points_index_t(dev(pts), cell) as idx:
        wide = check_radius(idx, pts, q, radius=1e6 * cell)  # the linear scan: everything, promptly
        assert all(len(g) == 300 for g in wide)
        check_radius(idx, pts, q, radius=cell / 1024)
        assert all(len(g) == 0 for g in check_radius(idx, pts, q, radius=0.0))
        radii = np.resize(np.array([1e6 * cell, cell / 1024, 0.0, 0.07, np.inf, 0.3], F), len(q))
        check_radius(idx, pts, q, radii=radii)
        bad = radii.copy()
        bad[::5] = np.nan  # in an array a NaN or negative radius reports nothing (sqrt(d2) < r is false)
        bad[1::5] = -1.0
        check_radius(idx, pts, q, radii=bad)
        check_knn(idx, pts, q, 64, 1e30)
        check_knn(idx, pts, q, 64, np.inf)


# ------------------------------------------------------------------ 6. far and non-finite
def test_far_and_non_finite():
    rng = np.random.default_rng(6)
    pts = rng.random((200, 3)).astype(F)
    pts[17] = [np.nan, 0.5, 0.5]
    pts[18] = [0.5, np.inf, 0.5]
    pts[19] = [0.5, 0.5, -np.inf]
    q = np.array([[1e7, 0, 0], [-1e7, 1e7, -1e7], [3e38, 0, 0], [0, -3e38, 3e38], [np.nan, 0.5, 0.5],
                  [0.5, np.inf, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]], F)
    q[7] = pts[16]
    with ctx().points_index_t(dev(pts), 0.1) as idx:
        assert np.array_equal(np.array(idx.info()["origin"], F), pts[np.isfinite(pts).all(1)].min(0))
        for r in (0.2, 2e7, np.inf):
            got = check_radius(idx, pts, q, radius=r)
            assert not any(i in g for g in got for i in (17, 18, 19))
            assert len(got[4]) == 0 and len(got[5]) == 0
        assert len(check_radius(idx, pts, q, radius=0.2)[6]) > 0  # the neighbours of the bad records are unharmed
        for m2 in (0.04, 1e30, np.inf):
            check_knn(idx, pts, q, 10, m2)
    far = (rng.random((100, 3)) * 10 + np.array([3e7, -3e7, 1e7])).astype(F)  # cells past what an int holds
    with ctx().points_index_t(dev(np.concatenate([pts, far])), 1e-3) as idx:
        both = np.concatenate([pts, far])
        qq = np.concatenate([q, far[:10], both[20:30]])
        check_radius(idx, both, qq, radius=3.0)
        check_knn(idx, both, qq, 5, 100.0)


# ------------------------------------------------------------------ 7. k
def test_k():
    rng = np.random.default_rng(7)
    pts = rng.random((150, 3)).astype(F)
    q = rng.random((70, 3)).astype(F)
    with ctx().points_index_t(dev(pts), 0.08) as idx:
        for k, m2 in ((1, 0.3), (64, 3.0), (64, 0.02), (17, 0.01), (50, 0.1)):
            gi, gd, gc = check_knn(idx, pts, q, k, m2)
            slots = np.arange(k)[None, :] >= gc[:, None]
            assert np.all(gi[slots] == -1) and not gd[slots].any()
        assert (check_knn(idx, pts, q, 64, 0.02)[2] < 64).any()
    few = pts[:5]
    with ctx().points_index_t(dev(few), 0.08) as idx:  # k > n
        assert np.all(check_knn(idx, few, q, 8, 10.0)[2] == 5)
    tie = np.array([[1, 0, 0], [0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], F)  # 0, 2, 3, 4 at d2 = 1 from the origin
    with ctx().points_index_t(dev(tie[[0, 2, 3, 4]]), 0.5) as idx:
        gi, gd, _ = check_knn(idx, tie[[0, 2, 3, 4]], np.zeros((1, 3), F), 1, 4.0)
        assert gi[0, 0] == 0 and gd[0, 0] == 1.0  # equal d2: the lower index
        gi, _, _ = check_knn(idx, tie[[0, 2, 3, 4]], np.zeros((1, 3), F), 3, 4.0)
        assert gi[0].tolist() == [0, 1, 2]


# ------------------------------------------------------------------ 8. the caller's offsets
def test_callers_offsets():
    rng = np.random.default_rng(8)
    pts = rng.random((400, 3)).astype(F)
    q = rng.random((64, 3)).astype(F)
    SENT = -7
    with ctx().points_index_t(dev(pts), 0.1) as idx:
        full = check_radius(idx, pts, q, radius=0.2)  # correct offsets: equal to the reference's
        cnt = np.array([len(g) for g in full], np.int64)
        assert cnt.min() >= 1 and cnt.max() >= 4  # truncation by half cuts something
        tq = dev(q)

        def run(offset, capacity):
            index = torch.full((capacity + 1,), SENT, dtype=torch.int32, device=DEV)[1:]  # a 4-byte aligned slice
            idx.fill_t(tq, dev(offset.astype(np.int64)), index, radius=0.2)
            want = np.full(capacity, SENT, np.int32)
            for j in range(len(q)):
                o0, o1 = int(offset[j]), int(offset[j + 1])
                if 0 <= o0 <= o1 <= capacity:
                    m = min(o1 - o0, len(full[j]))
                    want[o0:o0 + m] = full[j][:m]
            got = host(index)
            assert np.array_equal(got, want), np.argwhere(got != want)[:8].ravel()

        # understated: truncated lists, the words after each list still the sentinel
        room = cnt // 2
        run(np.concatenate([[0], np.cumsum(room)]), int(room.sum()) + 3)
        # generous ranges (count + 2), then broken ones: negative, past capacity, decreasing
        slack = np.concatenate([[0], np.cumsum(cnt + 2)])
        cap = int(slack[-1])
        run(slack, cap)
        bad = slack.copy()
        bad[3] = -5
        bad[10] = cap + 100
        bad[20] = bad[19] - 1
        run(bad, cap)
        run(bad, cap - int(cnt[-1]) - 3)  # the last ranges pass the capacity
        run(np.full(len(q) + 1, np.iinfo(np.int64).max), cap)
        run(np.full(len(q) + 1, np.iinfo(np.int64).min), cap)


# ------------------------------------------------------------------ 9. determinism
def test_determinism_across_builds_and_runs():
    rng = np.random.default_rng(9)
    centres = rng.random((16, 3))
    pts = (centres[rng.integers(0, 16, 3000)] + rng.normal(0, 0.02, (3000, 3))).astype(F)
    tp, tq = dev(pts), dev(rng.random((300, 3)).astype(F) * 0.2 + centres[3].astype(F) - F(0.1))
    outs = []
    for _ in range(2):
        with ctx().points_index_t(tp, 0.03) as idx:
            for _ in range(2):
                off, index = idx.in_radius_t(tq, radius=0.06)
                ki, kd, kc = idx.knn_t(tq, 50, 0.01)
                outs.append([host(t).tobytes() for t in (off, index, ki, kd, kc)])
    assert len(outs[0][1]) > 4 * 3000
    assert all(o == outs[0] for o in outs[1:])


# ------------------------------------------------------------------ 10. slices and overlap
def test_slices_overlap_and_foreign_arguments():
    rng = np.random.default_rng(10)
    pts, q = rng.random((100, 3)).astype(F), rng.random((33, 3)).astype(F)
    big_p = torch.zeros((301,), dtype=torch.float32, device=DEV)
    big_q = torch.zeros((100,), dtype=torch.float32, device=DEV)
    big_p[1:] = dev(pts).reshape(-1)
    big_q[1:] = dev(q).reshape(-1)
    tp, tq = big_p[1:].view(100, 3), big_q[1:].view(33, 3)
    assert tp.data_ptr() % 8 == 4 and tq.data_ptr() % 8 == 4  # 4-byte aligned only
    L, c = native.lib(), ctx()
    with c.points_index_t(tp, 0.1) as idx:
        big_p.zero_()  # the build copied what it needs
        want_cnt, want = _points_ref.radius_sets(q, pts, 0.2)
        out = torch.zeros((34,), dtype=torch.int32, device=DEV)
        idx.count_t(tq, radius=0.2, out=out[1:])
        assert np.array_equal(host(out)[1:], want_cnt) and host(out)[0] == 0
        check_radius(idx, pts, q, radius=0.2)
        # an output over an input
        with pytest.raises(native.WrError) as e:
            idx.count_t(tq, radius=0.2, out=tq.view(torch.int32).view(-1)[:33])
        assert e.value.code == native.WR_E_ARG and "overlaps" in str(e.value)
        # host memory
        hq, hc = np.zeros((33, 3), F), np.zeros(33, np.int32)
        assert L.wr_points_count_dev(c.h, idx.h, hq.ctypes.data_as(C.c_void_p), 33, 0.2, None,
                                     hc.ctypes.data_as(C.c_void_p)) == native.WR_E_ARG
        h = C.c_void_p()
        assert L.wr_points_build_dev(c.h, hq.ctypes.data_as(C.c_void_p), 33, 0.1, C.byref(h)) == native.WR_E_ARG
        assert not h.value
        # a misaligned offset array, arguments out of range
        cnt = torch.zeros((33,), dtype=torch.int32, device=DEV)
        off8 = torch.zeros((70,), dtype=torch.int32, device=DEV)[1:]
        ind = torch.zeros((64,), dtype=torch.int32, device=DEV)
        args = (c.h, idx.h, C.c_void_p(tq.data_ptr()), 33)
        assert L.wr_points_in_radius_dev(*args, 0.2, None, C.c_void_p(off8.data_ptr()), 64,
                                         C.c_void_p(ind.data_ptr())) == native.WR_E_ARG
        assert "aligned" in L.wr_last_error().decode()
        p = C.c_void_p(cnt.data_ptr())
        assert L.wr_points_count_dev(*args, -1.0, None, p) == native.WR_E_ARG
        assert L.wr_points_count_dev(*args, float("nan"), None, p) == native.WR_E_ARG
        assert L.wr_points_count_dev(*args, 0.2, None, None) == native.WR_E_ARG
        for k, m2 in ((0, 1.0), (65, 1.0), (4, -1.0), (4, float("nan"))):
            assert L.wr_points_knn_dev(*args, k, m2, p, p, p) == native.WR_E_ARG
        assert L.wr_points_count_dev(c.h, idx.h, C.c_void_p(tq.data_ptr()), (1 << 28) + 1, 0.2, None, p) == native.WR_E_ARG
        for cell in (0.0, -1.0, float("nan"), float("inf")):
            assert L.wr_points_build_dev(c.h, C.c_void_p(tp.data_ptr()), 100, cell, C.byref(h)) == native.WR_E_ARG
        # another context
        other = native.Context(c.scene, 0)
        try:
            assert L.wr_points_count_dev(other.h, idx.h, C.c_void_p(tq.data_ptr()), 33, 0.2, None, p) == native.WR_E_ARG
            assert "another context" in L.wr_last_error().decode()
        finally:
            other.close()
        assert np.array_equal(host(idx.count_t(tq, radius=0.2)), want_cnt)  # the index is unharmed


# ------------------------------------------------------------------ 11. a real distribution
def scene_radius(scene):
    """sceneSphere.sceneRadius (scene.cpp:483-487) from the scene dump."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "scene.txt")
        scene.dump(path)
        for line in open(path):
            if line.startswith("sphere"):
                return float.fromhex(line.split()[4])
    raise AssertionError("no sphere line in the scene dump")


def test_torus_camera_hits():
    c = ctx()
    hits = native.hit_fields(c.trace_closest_t(c.camera_rays_t(64, 64)))
    tp = hits["p"][hits["prim"] >= 0].contiguous()
    pts = host(tp)
    assert len(pts) > 2000
    radius = F(0.003) * F(scene_radius(c.scene))  # VertexCM::init, vertexcm.cpp:13
    rng = np.random.default_rng(11)
    dirs = rng.normal(size=pts.shape)
    q = (pts + dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * (0.5 * radius)).astype(F)
    with c.points_index_t(tp, float(radius)) as idx:
        got = check_radius(idx, pts, q, radius=float(radius))
        assert min(len(g) for g in got) >= 1
        check_knn(idx, pts, q, 50, (4 * radius) ** 2)
        check_knn(idx, pts, q, 50, 1e30)
    out = np.zeros((len(q), 4), np.int64)
    _oracle.lib().cr_kat_vkd(_oracle.fptr(pts), len(pts), _oracle.fptr(q), len(q), float(radius),
                             out.ctypes.data_as(C.POINTER(C.c_int64)))
    assert np.array_equal(out[:, 0], [len(g) for g in got])
    assert np.array_equal(out[:, 1], [int(g.astype(np.int64).sum()) for g in got])


# ------------------------------------------------------------------ 12. lifetime
def test_build_query_close_returns_device_memory():
    """50 rounds of build / query / close, some closed by the context instead:
    free device memory returns to where it was after the first round (the
    margin is tests/test_gpu_context.py's; one leaked index is 5 MB here)."""
    rng = np.random.default_rng(12)
    tp = dev(rng.random((200000, 3)).astype(F))
    tq = dev(rng.random((1000, 3)).astype(F))
    sc = ctx().scene
    L = native.lib()
    free = []
    for i in range(50):
        c = native.Context(sc, 0) if i % 10 == 0 else ctx()
        idx = c.points_index_t(tp, 0.02)
        assert idx.info()["device_bytes"] >= 5 << 20
        idx.count_t(tq, radius=0.03)
        idx.knn_t(tq, 8, 0.01)
        if c is ctx():
            idx.close()
        else:  # left open across the context's close: one through the wrapper, one in wr_destroy itself
            h = C.c_void_p()
            assert L.wr_points_build_dev(c.h, C.c_void_p(tp.data_ptr()), 200000, 0.02, C.byref(h)) == 0
            c.close()
            assert idx.h is None
        free.append(int(torch.cuda.mem_get_info(0)[0]))
    print("free bytes after rounds 1, 2, 50:", free[0], free[1], free[-1])
    assert min(free[2:]) >= free[1] - (8 << 20), (free[1], min(free[2:]))


# ------------------------------------------------------------------ 13. the script
def test_photon_script_index_equals_brute_force():
    """tests/_script_photons.py over knn_t and over the torch brute force on the
    same device arrays: the same neighbours in the same order, so the same sums."""
    s = native.Scene(_scenes.cbox(32, 24))
    c = native.Context(s, 0)
    try:
        a, na = _script_photons.estimate(_script_photons.DevicePhotons(c, 77, "index"), 4096, 32, 24, 16, 0.25)
        b, nb = _script_photons.estimate(_script_photons.DevicePhotons(c, 77, "brute"), 4096, 32, 24, 16, 0.25)
    finally:
        c.close()
        s.close()
    a, b = host(a), host(b)
    assert na == nb and 0 < na <= 4096
    assert np.isfinite(a).all() and (a >= 0).all() and (a.sum(1) > 0).sum() > 32 * 24 // 4
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), np.argwhere(a != b)[:5]
