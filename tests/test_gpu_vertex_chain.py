"""The BDPT vertex kernels' loads and stores by whole records (csrc/wr_bdpt.h:
vertex_inputs, BqRec, BvRec, WR_BDPT_TABLES).

The vertex kernels read a vertex's inputs in two stages with no branch in
front of a load (lanes without work read a valid record and drop it), move the
32-byte path state and the 64-byte stored vertices as 16-byte words, and keep
the material and light tables in LDS when they fit.  None of that changes a
float, so every case here is a render against the oracle on the film gates of
tests/_parity.py with equal ray counts -- on the smallest films at which the
moved loads can go wrong: one wave, a partial last wave, tiled and untiled
path orders, both connection sides, the sphere branch of a stored vertex's
normal, pools that overflow (slot -1), the sequential schedule, and an emitter of
more than 32,768 faces (the stored vertex's material word, and a light table
above the LDS cap).
"""
import functools
import os

import numpy as np
import pytest

import _oracle
import _scenes
from _parity import assert_film_parity, assert_ray_counts
from winmad_rt import native, scenes

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


# 1. partial waves and blocks: one wave; 480 paths in plain path order (24 is
# no multiple of 8) whose last wave is partial; a tiled film of 320 paths
@pytest.mark.parametrize("W,H", [(8, 8), (24, 20), (40, 8)])
@pytest.mark.parametrize("ctl", [0, 3])
def test_partial_waves_and_blocks(W, H, ctl):
    _check(_scenes.torus(W, H), W, H, 2, ctl, f"chain_torus{W}x{H}_i2_ctl{ctl}")


# 2. every record path: both connection sides (the Cornell box with every
# path length), and the sphere branch of the stored vertex's normal
@pytest.mark.parametrize("name,maker,W,H,ctl", [
    ("cbox", lambda: _scenes.cbox(32, 24), 32, 24, 0),
    ("spheres", lambda: _scenes.spheres(32, 32), 32, 32, 0),
    ("spheres", lambda: _scenes.spheres(32, 32), 32, 32, 3),
])
def test_every_record_path(name, maker, W, H, ctl):
    _check(maker(), W, H, 2, ctl, f"chain_{name}{W}x{H}_i2_ctl{ctl}")


# 3. slot -1: pools that overflow (a full pool hands out slot -1, which is
# never dereferenced; the render is redone), and the worst-case layout
# (WR_BDPT_POOL_SCALE=0: no pools, vidx / cidx null)
def test_full_pools_and_the_worst_case_layout(monkeypatch):
    path = _scenes.cbox(32, 24)
    monkeypatch.setenv("WR_BDPT_POOL_SCALE", "0.02")
    small = _render(path, 32, 24, 2, 0, pipes=1)
    monkeypatch.setenv("WR_BDPT_POOL_SCALE", "0")
    full = _render(path, 32, 24, 2, 0, pipes=1)
    print(f"redone: small pools {small[1].redone}, worst-case layout {full[1].redone}")
    assert small[1].redone == 1 and full[1].redone == 0, (small[1].redone, full[1].redone)
    _same(small, full)
    _check(path, 32, 24, 2, 0, "chain_cbox32x24_i2_ctl0_smallpools", small)
    _check(path, 32, 24, 2, 0, "chain_cbox32x24_i2_ctl0_nopools", full)


# 4. the other schedule: sequential passes
@pytest.mark.parametrize("env,val", [("WR_BDPT_OVERLAP", "0")])
def test_other_schedules(env, val, monkeypatch):
    path = _scenes.torus(24, 20)
    s = native.Scene(path)

    def render():
        c = native.Context(s, 0)
        c.set_trace_mode(native.TRACE_BVH)
        try:
            return c.render_bdpt(24, 20, iterations=2, seed=SEED, control_length=0)
        finally:
            c.close()

    base = render()
    monkeypatch.setenv(env, val)
    other = render()
    _same(other, base)
    _check(path, 24, 20, 2, 0, f"chain_torus24x20_i2_ctl0_{env.lower()}{val}", other)
    _check(path, 24, 20, 2, 0, "chain_torus24x20_i2_ctl0_default", base)


# 5. the material word: an emitter of more than 32,768 faces
TENT_N = 128  # cells per side of a slope: 2 slopes x N x N x 2 = 65,536 triangles


def _tent_obj(path, n=TENT_N):
    """assets/tent_luminaire.obj (two slopes of a roof ridge along y, emitting
    faces turned inward and down), each slope cut into n x n cells of two
    triangles with the asset's winding."""
    A, B, D = np.array([-0.3, -0.3, 1.0]), np.array([0.0, -0.3, 1.2]), np.array([-0.3, 0.3, 1.0])
    E, F = np.array([0.3, -0.3, 1.0]), np.array([0.3, 0.3, 1.0])
    with open(path, "w") as f:
        f.write(f"# tent luminaire, {4 * n * n} faces\n")
        for o, du, dv in ((A, B - A, D - A), (E, B - E, F - E)):
            for i in range(n + 1):
                for j in range(n + 1):
                    p = o + du * (i / n) + dv * (j / n)
                    f.write(f"v {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n")
        idx = lambda s, i, j: s * (n + 1) * (n + 1) + i * (n + 1) + j + 1
        for s in range(2):
            for i in range(n):
                for j in range(n):
                    p00, p10, p11, p01 = idx(s, i, j), idx(s, i + 1, j), idx(s, i + 1, j + 1), idx(s, i, j + 1)
                    if s == 0:  # the asset's (1 3 2), (1 4 3)
                        f.write(f"f {p00} {p11} {p10}\nf {p00} {p01} {p11}\n")
                    else:  # (5 2 3), (5 3 6)
                        f.write(f"f {p00} {p10} {p11}\nf {p00} {p11} {p01}\n")
    return path


def _big_tent_scene(tmp_path, W, H):
    """tent_scene's Cornell-box walls and camera under the tessellated tent."""
    obj = _tent_obj(str(tmp_path / "tent_big.obj"))
    text = scenes.tent_scene(W, H).replace(os.path.join(scenes.ASSETS, "tent_luminaire.obj"), obj)
    assert obj in text
    return scenes.write(str(tmp_path / f"tent_big_{W}x{H}.scene"), text)


def _light_first_hits(path, P, it_index=0):
    """Material ids at the first hit of the oracle's light subpaths of one
    iteration (generateLightSample with the render's own random streams,
    :267-311: light index, then posRand3, then dirRand3; the first ray leaves
    pos + dir * EPS): -(light + 1) on an emitter face."""
    sc = _oracle.Scene(path)
    L = sc.L
    nl = L.cr_scene_nlights(sc.h)
    rays = np.zeros((P, 9), np.float32)
    z3 = _oracle.f32(0, 0, 0)
    out = np.zeros(27, np.float32)
    for p in range(P):
        key = L.cr_stream_key(SEED, it_index, 0, p)
        f = [np.float32(L.cr_stream_u32(key, j) & 0xFFFFFF) / np.float32(16777216.0) for j in range(7)]
        lid = min(int(np.float32(f[0] * np.float32(nl))), nl - 1)
        pr, dr = _oracle.f32(*f[1:4]), _oracle.f32(*f[4:7])
        L.cr_kat_light(sc.h, lid, _oracle.fptr(z3), _oracle.fptr(z3), _oracle.fptr(dr), _oracle.fptr(pr),
                       _oracle.fptr(z3), _oracle.fptr(out))
        pos, d = out[13:16].astype(np.float64), out[16:19].astype(np.float64)
        rays[p, 0:3] = pos + d * 1e-3
        rays[p, 3:6] = d / np.linalg.norm(d)
    oi, _, _, _ = sc.trace(rays)
    return oi[:, 0], oi[:, 2]


def test_material_word_of_a_large_emitter(tmp_path):
    W, H = 32, 24
    path = _big_tent_scene(tmp_path, W, H)
    # on the CPU first: light subpaths of this render do hit emitter faces
    # whose index is above 32,767 (material below -32,768), whose stored
    # vertex a 16-bit material field would decode as a positive material
    prim, mat = _light_first_hits(path, W * H)
    high = int(((prim >= 0) & (mat < -32768)).sum())
    print(f"light subpaths whose first hit is an emitter face above 32,767: {high} of {W * H} "
          f"(emitter hits {int(((prim >= 0) & (mat < 0)).sum())}, lowest material {int(mat.min())})")
    assert high > 0
    _check(path, W, H, 1, 0, "chain_tent65536_32x24_i1_ctl0")
