"""The device shading math by itself: csrc/wr_devmath.h and csrc/wr_libm.h as
the gfx950 code object computes them, one function at a time, through
libwr_devkat.so (tests/native/dev_kat.hip via tests/_devkat.py -- test
infrastructure, not part of libwinmad_rt.so), and the material zoo
(scenes.zoo_scene) through whole renders.

Everything is compared by bit pattern:
  * the harness against the reference's own answers (tests/golden/kat_*.txt, kat_zoo*.txt.gz);
  * the harness against the oracle's hooks on 4,000 seeded random cases per zoo
    material, light and sampler (tests/_kat.py; the CPU suite checks that these
    cases are not thin: test_oracle.py::test_zoo_random_cases_are_not_thin);
  * the counter RNG, and wr_sinf / wr_cosf / wr_sincosf / wr_powf against the
    same header compiled for the host (pinned to glibc by tests/test_libm.py);
  * BDPT / PT / VCM films of the zoo, with 13 and with 43 materials, against
    the oracle on the same counter-RNG streams (the gates of tests/_parity.py).

The hooks preset outputs that a function may leave unwritten to -7.  ONE_SIDED
names every output that only one side defines, by design; such an output is
compared where both sides hold a value, and nothing else is masked.
"""
import numpy as np
import pytest

import _devkat
import _kat
import _oracle
import _scenes
from _kat import F, same_bits
from _parity import assert_film_parity, assert_ray_counts
from winmad_rt import native, scenes

pytestmark = pytest.mark.gpu

UNSET = F(-7)
# (layout, slot): why only one side defines it
ONE_SIDED = {
    ("sampler", 7): "wr_devmath.h:127 sample_pow_cos_hemi returns no pdf (the reference's samplePowerCosHemisphere "
                    "does, sampler.cpp:123; the kernels take pow_cos_pdf, wr_devmath.h:135, slot 8)",
}
PI = F(3.14159274101257324)

_scene_cache = {}


def dev_scene(path):
    if path not in _scene_cache:
        _scene_cache[path] = _devkat.Scene(path)
    return _scene_cache[path]


def compare(layout, got, want, what):
    keep = np.ones(want.shape[1], bool)
    for (lay, slot) in ONE_SIDED:
        if lay == layout:
            keep[slot] = False
            both = (got[:, slot] != UNSET) & (want[:, slot] != UNSET)
            same_bits(got[both, slot], want[both, slot], f"{what} slot {slot}")
    return same_bits(got[:, keep], want[:, keep], what)


def run_cases(dev, k, what, tags):
    """The harness on the parsed / generated cases `k`; returns the number of values compared per tag."""
    n = {}
    if "sampler" in tags:
        s = k["sampler"]
        n["sampler"] = compare("sampler", _devkat.sampler(s["u"], s["power"], s["tri"], s["k"], s["tot"]), s["out"],
                               what + " sampler")
    if "frame" in tags:
        f = k["frame"]
        n["frame"] = compare("frame", _devkat.frame(f["z"], f["ci"], f["idx"]), f["out"], what + " frame")
    if "bsdf" in tags:
        b = k["bsdf"]
        out, valid = dev.bsdf(b["mat"], b["inp"], _kat.BSDF_PRESET)
        assert np.array_equal(valid, b["valid"]), (what, "valid flags", int((valid != b["valid"]).sum()))
        n["bsdf"] = compare("bsdf", out, b["out"], what + " bsdf")
    if "light" in tags:
        li = k["light"]
        n["light"] = compare("light", dev.light(li["li"], li["inp"]), li["out"], what + " light")
    return n


KAT_SCENES = {"kat_zoo": lambda: _scenes.zoo(24, 32), "kat_zoo_edges": lambda: _scenes.zoo(24, 32),
              "kat_torus64": lambda: _scenes.torus(64, 64), "kat_cbox64x48": lambda: _scenes.cbox(64, 48),
              "kat_spheres64": lambda: _scenes.spheres(64, 64)}


@pytest.mark.parametrize("name", list(KAT_SCENES))
def test_device_functions_equal_the_reference_answers(name):
    """Every line of the zoo's two kat files, and of the three older ones: the
    samplers, frames, Fresnel, BSDFs per material, the AreaLight calls and the
    camera's raster point and check, on tables the product's own loader and
    flattening made."""
    k = _kat.parse(name)
    dev = dev_scene(KAT_SCENES[name]())
    n = run_cases(dev, k, name, ("sampler", "frame", "bsdf", "light"))
    if "cam" in k:
        c = k["cam"]
        out = dev.camera(c["xy"], c["w"])
        n["cam"] = same_bits(out[:, 3:6], c["ras"], name + " raster point")
        assert np.array_equal(out[:, 6].astype(np.int32), c["check"])
    print(name, "values compared:", n, "invalid BSDFs:", int((k["bsdf"]["valid"] == 0).sum()))
    assert n["bsdf"] > 0 and n["light"] > 0 and n["sampler"] > 0


def test_device_functions_equal_the_oracle_on_random_cases():
    """4,000 seeded random cases per zoo material (with wi at the tangent plane,
    mirror and grazing wo mixed in), per light, and for the samplers, frames,
    Fresnel and the camera transforms."""
    c = _kat.zoo_random_cases()
    stats = _kat.check_zoo_random_cases(c)
    dev = dev_scene(_scenes.zoo(24, 32))
    n = run_cases(dev, c, "random", ("sampler", "frame", "bsdf", "light"))
    n["cam"] = same_bits(dev.camera(c["cam"]["xy"], c["cam"]["w"]), c["cam"]["out"], "random camera")
    print("values compared:", n, stats)
    # the same cases on the scene padded to 43 materials, through each material's last copy
    pad = dev_scene(_scenes.zoo(24, 32, "bdpt", 30))
    assert pad.nmats == 43
    b = c["bsdf"]
    ids = np.array([scenes.zoo_material_id(int(m), 30) for m in range(_kat.NMAT)], np.int32)[b["mat"]]
    assert ids.max() == 42 and (ids > 32).mean() > 0.8
    out, valid = pad.bsdf(ids, b["inp"], _kat.BSDF_PRESET)
    assert np.array_equal(valid, b["valid"])
    compare("bsdf", out, b["out"], "random bsdf, padded materials")


def test_harness_refuses_indices_outside_the_tables():
    dev = dev_scene(_scenes.zoo(24, 32))
    inp = np.zeros((1, 12), F)
    for m in (0, -1, dev.nmats):
        with pytest.raises(RuntimeError, match="material index"):
            dev.bsdf(np.array([m], np.int32), inp, _kat.BSDF_PRESET)
    for li in (-1, dev.nlights):
        with pytest.raises(RuntimeError, match="light index"):
            dev.light(np.array([li], np.int32), np.zeros((1, 15), F))


def test_counter_rng_streams_equal_the_oracle():
    """stream_key, Rng::u32 and Rng::f: 64 keys x 64 draws, with seed, iteration,
    subpath and path values at 0 and 2^32 - 1."""
    rng = np.random.default_rng(9)
    keys = rng.integers(0, 1 << 32, (64, 4), dtype=np.uint64).astype(np.uint32)
    edge = [0, 0xFFFFFFFF]
    k = 0
    for a in edge:
        for b in edge:
            for c in edge:
                for d in edge:
                    keys[k] = (a, b, c, d)
                    k += 1
    for col in range(4):  # one field at an edge, the others random
        keys[16 + 2 * col, col], keys[17 + 2 * col, col] = 0, 0xFFFFFFFF
    key, u, f = _devkat.rng(keys, 64)
    L = _oracle.lib()
    want_key = np.array([L.cr_stream_key(*map(int, r)) for r in keys], np.uint64)
    same_bits(key, want_key, "stream_key")
    want_u = np.array([[L.cr_stream_u32(int(kk), j) for j in range(64)] for kk in want_key], np.uint32)
    same_bits(u, want_u, "Rng::u32")
    want_f = ((want_u & 0xFFFFFF).astype(F) / F(16777216.0)).astype(F)  # rng.cpp:18-22, exact in float32
    same_bits(f, want_f, "Rng::f")
    assert len(set(want_key.tolist())) == 64


def _libm_equal(op, x, y=None, what=""):
    got = _devkat.libm(op, x, y)
    want = _devkat.libm(op, x, y, expected=True)
    if op == _devkat.SINCOS:
        return same_bits(got[0], want[0], what + " sin", nan_equal=True) + \
            same_bits(got[1], want[1], what + " cos", nan_equal=True)
    return same_bits(got, want, what, nan_equal=True)


def test_libm_cos_sin_of_every_sampler_input():
    """cos / sin of 2 PI k / 2^24 for all 2^24 k (sampler.cpp:97-100, 121-125):
    wr_sinf, wr_cosf and both halves of wr_sincosf on the device."""
    s = (np.arange(1 << 24, dtype=np.float64) / 2.0 ** 24).astype(F)
    u1 = (F(2) * PI) * s  # 2.f * PI * s in float
    sin = _devkat.libm(_devkat.SIN, u1, expected=True)
    cos = _devkat.libm(_devkat.COS, u1, expected=True)
    same_bits(_devkat.libm(_devkat.SIN, u1), sin, "wr_sinf, sampler inputs")
    same_bits(_devkat.libm(_devkat.COS, u1), cos, "wr_cosf, sampler inputs")
    s2, c2 = _devkat.libm(_devkat.SINCOS, u1)
    same_bits(s2, sin, "wr_sincosf sin, sampler inputs")
    same_bits(c2, cos, "wr_sincosf cos, sampler inputs")


@pytest.mark.parametrize("lo,hi,step", [(0.0, 256.0, 97), (0.0, 1e-3, 1009), (256.0, 3.4e38, 3001)])
def test_libm_cos_sin_over_the_float_range(lo, hi, step):
    """The three ranges of tests/test_libm.py: every step-th float in [lo, hi] and its negative."""
    a, b = (int(np.array([v], F).view(np.uint32)[0]) for v in (lo, hi))
    bits = np.arange(a, b + 1, step, dtype=np.uint32)
    x = np.concatenate([bits, bits | np.uint32(0x80000000)]).view(F)
    assert x.size > 100000
    for op, what in ((_devkat.SIN, "wr_sinf"), (_devkat.COS, "wr_cosf"), (_devkat.SINCOS, "wr_sincosf")):
        _libm_equal(op, x, what=f"{what} [{lo}, {hi}]")


@pytest.mark.parametrize("exponent", [0, 1, 3, 20, 90, 400])
def test_libm_powf_for_the_phong_exponents(exponent):
    """powf(c, e) over a stride of the float cosines in (0, 1] (bsdf.cpp:99,
    sampler.cpp:135) and powf(u, 1 / (e + 1)) over a stride of the sampler's u
    (sampler.cpp:119)."""
    c = np.arange(1, 0x3f800000 + 1, 6151, dtype=np.uint32).view(F)
    _libm_equal(_devkat.POW, c, np.full(c.size, exponent, F), f"wr_powf(c, {exponent})")
    u = (np.arange(0, 1 << 24, 61, dtype=np.float64) / 2.0 ** 24).astype(F)
    ie = F(1) / (F(exponent) + F(1))
    _libm_equal(_devkat.POW, u, np.full(u.size, ie, F), f"wr_powf(u, 1 / ({exponent} + 1))")
    _libm_equal(_devkat.POW, u, np.full(u.size, exponent, F), f"wr_powf(u, {exponent})")


def test_libm_specials():
    """0, -0, 1, denormals, infinities and NaN (a NaN equals a NaN of any payload, here only)."""
    x = np.array([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 1e-39, -1e-40, 1.1754942e-38, np.inf, -np.inf, np.nan,
                  1e30, -1e30, 0.5, 2.0, 3.4028235e38], F)
    for op, what in ((_devkat.SIN, "wr_sinf"), (_devkat.COS, "wr_cosf"), (_devkat.SINCOS, "wr_sincosf")):
        _libm_equal(op, x, what=what + " specials")
    y = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0, 3.0, 400.0, 1.0 / 401.0, 1e-40, np.inf, -np.inf, np.nan, -3.0,
                  2.5], F)
    xx, yy = (a.reshape(-1).copy() for a in np.meshgrid(x, y))
    _libm_equal(_devkat.POW, xx, yy, "wr_powf specials")


# ------------------------------------------------------------------ zoo films
_ctx_cache = {}


def zoo_ctx(W, H, mode, pad):
    key = (W, H, mode, pad)
    if key not in _ctx_cache:
        path = _scenes.zoo(W, H, mode, pad)
        s = native.Scene(path)
        assert s.info()["nmaterials"] == 13 + pad
        _ctx_cache[key] = (path, s, native.Context(s, 0))
    return _ctx_cache[key][0], _ctx_cache[key][2]


_ref_cache = {}


def zoo_ref(kind):
    """The oracle's film (counter RNG) of the unpadded zoo, once per kind: the
    padded scene's objects carry copies of the same materials, so its film is
    the same (test_oracle.py::test_zoo_films_mt_serial_bit_exact)."""
    if kind not in _ref_cache:
        if kind.startswith("bdpt"):
            cl = int(kind[-1])
            _ref_cache[kind] = _oracle.Scene(_scenes.zoo(24, 32)).bdpt(24, 32, 2, 5489, mode=1, control_length=cl)
        elif kind == "pt":
            _ref_cache[kind] = _oracle.Scene(_scenes.zoo(32, 24, "pt")).pt(32, 24, 4, 7, 5489, mode=1)
        else:
            _ref_cache[kind] = _oracle.Scene(_scenes.zoo(24, 32)).vcm(24, 32, 2, 3, mode=1, radius_factor=0.05)
    return _ref_cache[kind]


@pytest.mark.parametrize("pad", [0, 30])
@pytest.mark.parametrize("kind", ["bdpt_cl0", "bdpt_cl3", "pt", "vcm"])
def test_zoo_films_match_oracle_counter_rng(kind, pad):
    """BDPT 24x32 with every path length (control_length 0) and with the
    reference's 3, PT 32x24 spp 4, VCM 24x32 at radius factor 0.05; with 13
    materials (LDS tables) and with 43 (global tables, objects shaded through
    material ids up to 42)."""
    ref, rst = zoo_ref(kind)
    assert rst.closest_rays > 1000 and rst.shadow_rays > 1000
    if kind.startswith("bdpt"):
        _, c = zoo_ctx(24, 32, "bdpt", pad)
        film, st = c.render_bdpt(24, 32, iterations=2, seed=5489, control_length=int(kind[-1]))
    elif kind == "pt":
        _, c = zoo_ctx(32, 24, "pt", pad)
        film, st = c.render_path(32, 24, spp=4, max_depth=7, seed=5489)
        film = film * F(1.0 / 4)  # the oracle (like the reference) scales by 1 / spp
    else:
        _, c = zoo_ctx(24, 32, "bdpt", pad)
        film, st = c.render_vcm(24, 32, iterations=2, seed=3, radius_factor=0.05)
    assert_film_parity(film, ref, case=f"zoo_{kind}_pad{pad}")
    assert_ray_counts(st, rst)
    if kind == "vcm":
        assert rst.vm_merged > 1000
        for k in ("vm_queries", "vm_found", "vm_merged"):
            assert getattr(st, k) == getattr(rst, k), (k, getattr(st, k), getattr(rst, k))


def test_zoo_feature_films_of_the_padded_scene(tmp_path):
    """wr_render_features on the 43-material zoo against wr_trace_closest on the
    oracle's camera rays: the albedo film reads material ids above 32."""
    from test_gpu_denoise import _albedo_table, _camera_rays
    W, H = 24, 32
    path, c = zoo_ctx(W, H, "bdpt", 30)
    hits = c.trace_closest(_camera_rays(path, W, H, native.FILM_BDPT))
    hit, mat = hits["prim"] >= 0, hits["mat_id"]
    table = _albedo_table(c.scene, str(tmp_path))
    assert len(table) == 43 and (mat[hit] > 32).sum() > 100 and len(set(mat[hit & (mat > 32)].tolist())) >= 6
    alb = np.where((mat < 0)[:, None], F(1.0), table[np.clip(mat, 0, len(table) - 1)])
    got, st = c.render_features(W, H, native.FILM_BDPT)
    assert st.closest_rays == W * H
    same_bits(got["albedo"].reshape(-1, 3), np.where(hit[:, None], alb, F(0)).astype(F), "padded zoo albedo")
    same_bits(got["normal"].reshape(-1, 3), np.where(hit[:, None], hits["n"], F(0)).astype(F), "padded zoo normal")
    same_bits(got["depth"].reshape(-1), np.where(hit, hits["t"], F(0)).astype(F), "padded zoo depth")
