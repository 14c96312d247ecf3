"""Hit compaction in the BDPT vertex kernels (csrc/wr_bdpt.h: compact_hits,
HitList, hit_chunk_r).

k_light_shade and the shading half of k_camera_step list, per block and in
LDS, the queue entries of a chunk whose ray hit something, and shade only
those, in full waves; a missed light entry loses its lvc alive bit in the
compaction pass.  The same rays are traced and the same vertices made, so
every case is a render against the oracle on the film gates of
tests/_parity.py with equal ray counts, on the smallest films at which the
list can go wrong: one wave, partial waves, tiled and untiled order, more than
one entry per thread and more than one chunk per block, chunks without a hit,
chunks of hits only, group members, the sequential schedule, overflowing
pools.  Each case first asserts, from an oracle trace of the first rays, that
its film has the mix of hits and misses it is there for.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle
import _scenes
from _parity import assert_film_parity, assert_ray_counts
from winmad_rt import native

pytestmark = pytest.mark.gpu

SEED = 5489


@functools.lru_cache(maxsize=None)
def _ref(path, W, H, it, ctl):
    """The oracle's render, computed once per case and shared (read only)."""
    film, st = _oracle.Scene(path).bdpt(W, H, it, SEED, mode=1, control_length=ctl)
    film.setflags(write=False)
    return film, st


def _render(path, W, H, it, ctl, pipes=None):
    c = native.Context(native.Scene(path), 0)
    if pipes:
        c.set_pipelines(pipes)
    try:
        return c.render_bdpt(W, H, iterations=it, seed=SEED, control_length=ctl)
    finally:
        c.close()


def _check(path, W, H, it, ctl, case, film_st=None):
    film, st = film_st or _render(path, W, H, it, ctl)
    ref, rst = _ref(path, W, H, it, ctl)
    print(f"{case}: closest {st.closest_rays} shadow {st.shadow_rays} (oracle {rst.closest_rays} {rst.shadow_rays})")
    assert rst.shadow_rays > 0  # the case makes connections / shadow rays at all
    assert_film_parity(film, ref, case=case)
    assert_ray_counts(st, rst)
    return film, st


def _same(a, b):
    """Two GPU renders of the same paths: equal up to the order of float atomics."""
    (fa, sa), (fb, sb) = a, b
    assert sa.closest_rays == sb.closest_rays and sa.shadow_rays == sb.shadow_rays
    assert np.allclose(fa, fb, rtol=1e-4, atol=1e-6)


# ---------------------------------------------------------------- the first rays on the CPU
def _u24(L, kind, P, n):
    """The first n floats of the streams (SEED, iteration 0, kind, p), p < P:
    RNG::randFloat's k / 2^24."""
    u = np.array([[L.cr_stream_u32(key, j) for j in range(n)]
                  for key in (L.cr_stream_key(SEED, 0, kind, p) for p in range(P))], np.int64)
    return (u & 0xFFFFFF).astype(np.float32) / np.float32(16777216.0)


def _first_hits(sc, od):
    """The rays (origin + direction * EPS, direction normalised) of (P, 6) od, traced by the oracle."""
    rays = np.zeros((len(od), 9), np.float32)
    rays[:, 0:3] = od[:, 0:3] + od[:, 3:6] * 1e-3
    rays[:, 3:6] = od[:, 3:6] / np.linalg.norm(od[:, 3:6], axis=1, keepdims=True)
    oi, _, _, _ = sc.trace(rays)
    return oi[:, 0] >= 0


def _at(a, i):
    return C.cast(a.ctypes.data + i * a.strides[0], C.POINTER(C.c_float))


@functools.lru_cache(maxsize=None)
def _light_first_hits(path, P):
    """hit[p]: the first ray of the oracle's light subpath p of iteration 0 hits
    something (generateLightSample with the render's own streams, :267-311:
    light index, then posRand3, then dirRand3; the ray leaves pos + dir * EPS)."""
    sc = _oracle.Scene(path)
    L = sc.L
    nl = L.cr_scene_nlights(sc.h)
    f = _u24(L, 0, P, 7)
    lid = np.minimum((f[:, 0] * np.float32(nl)).astype(np.int64), nl - 1).tolist()
    pr, dr = np.ascontiguousarray(f[:, 1:4]), np.ascontiguousarray(f[:, 4:7])
    zp = _oracle.fptr(_oracle.f32(0, 0, 0))
    out = np.zeros((P, 27), np.float32)
    for p in range(P):
        L.cr_kat_light(sc.h, lid[p], zp, zp, _at(dr, p), _at(pr, p), zp, _at(out, p))
    return _first_hits(sc, out[:, 13:19].astype(np.float64))


@functools.lru_cache(maxsize=None)
def _camera_path_hits(path, W, H):
    """hit[p]: the primary ray of iteration 0's path p hits something
    (generateCameraSample, :418-452: path p is raster x = p / W, y = p % W,
    jittered by the first two floats of its stream; camera.cpp:37-42)."""
    sc = _oracle.Scene(path)
    L = sc.L
    P = W * H
    f = _u24(L, 1, P, 2)
    p = np.arange(P)
    xs, ys = ((p // W).astype(np.float32) + f[:, 0]).tolist(), ((p % W).astype(np.float32) + f[:, 1]).tolist()
    wp = _oracle.fptr(np.zeros(3, np.float32))
    out = np.zeros((P, 10), np.float32)
    for k in range(P):
        L.cr_kat_camera(sc.h, xs[k], ys[k], wp, _at(out, k))
    return _first_hits(sc, out[:, 0:6].astype(np.float64))


def _camera_first_hits(path, W, H):
    """_camera_path_hits in the library's queue order: 8 x 8 tiles per wave
    when both sides are multiples of 8 (camera_gen_one), else path order."""
    hit = _camera_path_hits(path, W, H)
    if W % 8 == 0 and H % 8 == 0:
        s = np.arange(W * H)
        t, w = s >> 6, s & 63
        ty = W // 8
        hit = hit[((t // ty) * 8 + (w >> 3)) * W + (t % ty) * 8 + (w & 7)]
    return hit


def _waves(hit):
    """(hits, waves of 64 without a hit, waves of hits only, waves of both)."""
    n = len(hit)
    per = np.add.reduceat(hit.astype(np.int64), np.arange(0, n, 64))
    size = np.minimum(64, n - np.arange(0, n, 64))
    return int(hit.sum()), int((per == 0).sum()), int((per == size).sum()), int(((per > 0) & (per < size)).sum())


def _mix(path, W, H, case):
    lh, ch = _waves(_light_first_hits(path, W * H)), _waves(_camera_first_hits(path, W, H))
    print(f"{case}: of {W * H} first rays, light hits {lh[0]} (waves: {lh[1]} empty, {lh[2]} full, {lh[3]} mixed), "
          f"camera hits {ch[0]} (waves: {ch[1]} empty, {ch[2]} full, {ch[3]} mixed)")
    return lh, ch


# 1. one wave, partial waves, tiled and untiled order.  Control length 0 makes
# the lvc alive bit matter: a miss that does not clear it changes which camera
# vertices are stored, and with them the connections and the shadow-ray count.
TORUS_MIX = {(8, 8): (23, 46), (24, 20): (176, 361), (40, 8): (118, 239)}


@pytest.mark.parametrize("W,H", list(TORUS_MIX))
@pytest.mark.parametrize("ctl", [0, 3])
def test_mixed_waves(W, H, ctl):
    path = _scenes.torus(W, H)
    lh, ch = _mix(path, W, H, f"torus{W}x{H}")
    assert (lh[0], ch[0]) == TORUS_MIX[(W, H)]
    nw = (W * H + 63) // 64
    assert lh[3] == nw and ch[3] == nw  # every wave is mixed
    _check(path, W, H, 2, ctl, f"hits_torus{W}x{H}_i2_ctl{ctl}")


# 2. more than one entry per thread (82,944 entries against the default grid's
# 65,536 lanes), more than one chunk per block, chunks without a hit
def test_long_chunks_and_chunks_without_a_hit():
    W, H = 384, 216
    path = _scenes.torus(W, H)
    lh, ch = _mix(path, W, H, f"torus{W}x{H}")
    assert lh[0] == 31358 and lh[3] == 1296
    # waves without a hit: 214 with the primaries in path order; the queue is in
    # tiles, which have more of them
    assert _waves(_camera_path_hits(path, W, H))[1] == 214 and ch[1] > 0
    # (a chunk of 2 x 256 entries is 8 waves: a run of 8 empty waves aligned to
    # it is a chunk without a hit)
    per = np.add.reduceat(_camera_first_hits(path, W, H).astype(np.int64), np.arange(0, W * H, 512))
    print(f"camera chunks of 512 entries without a hit: {int((per == 0).sum())} of {len(per)}")
    assert (per == 0).any()
    _check(path, W, H, 1, 3, f"hits_torus{W}x{H}_i1_ctl3", _render(path, W, H, 1, 3, pipes=1))


# 3. every entry a hit (the compaction is the identity), the sphere branch of
# the stored vertex; and the Cornell box: both connection sides, every length
@pytest.mark.parametrize("ctl", [0, 3])
def test_every_entry_a_hit(ctl):
    path = _scenes.spheres(32, 32)
    ch = _waves(_camera_first_hits(path, 32, 32))
    assert ch[0] == 1024 and ch[2] == 16
    _check(path, 32, 32, 2, ctl, f"hits_spheres32x32_i2_ctl{ctl}")


def test_cornell_box():
    path = _scenes.cbox(32, 24, "bdpt")
    lh, _ = _mix(path, 32, 24, "cbox32x24")
    assert lh[0] == 621
    _check(path, 32, 24, 2, 0, "hits_cbox32x24_i2_ctl0")


# 4. group members: three iterations on one pipeline, so a launch carries more
# than one member in blockIdx.y
def test_group_members():
    path = _scenes.torus(24, 20)
    _check(path, 24, 20, 3, 0, "hits_torus24x20_i3_ctl0_1pipe", _render(path, 24, 20, 3, 0, pipes=1))


# 5. the sequential schedule
def test_sequential_schedule(monkeypatch):
    path = _scenes.torus(24, 20)
    base = _render(path, 24, 20, 2, 0)
    monkeypatch.setenv("WR_BDPT_OVERLAP", "0")
    seq = _render(path, 24, 20, 2, 0)
    _same(seq, base)
    _check(path, 24, 20, 2, 0, "hits_torus24x20_i2_ctl0_sequential", seq)
    _check(path, 24, 20, 2, 0, "hits_torus24x20_i2_ctl0_overlapped", base)


# 6. pools that overflow: the render is redone in pieces, untiled
def test_pools_that_overflow(monkeypatch):
    path = _scenes.cbox(32, 24, "bdpt")
    monkeypatch.setenv("WR_BDPT_POOL_SCALE", "0.02")
    small = _render(path, 32, 24, 2, 0, pipes=1)
    monkeypatch.setenv("WR_BDPT_POOL_SCALE", "0")
    full = _render(path, 32, 24, 2, 0, pipes=1)
    print(f"redone: small pools {small[1].redone}, worst-case layout {full[1].redone}")
    assert small[1].redone == 1 and full[1].redone == 0, (small[1].redone, full[1].redone)
    _same(small, full)
    _check(path, 32, 24, 2, 0, "hits_cbox32x24_i2_ctl0_smallpools", small)


# 7. twice the same render
def test_twice_the_same_render():
    path = _scenes.torus(40, 8)
    a, b = _render(path, 40, 8, 2, 0), _render(path, 40, 8, 2, 0)
    _same(a, b)
    _check(path, 40, 8, 2, 0, "hits_torus40x8_i2_ctl0_again", b)
