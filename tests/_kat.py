"""Known-answer cases of the shading math, shared by tests/test_oracle.py (CPU)
and tests/test_gpu_devkat.py (GPU): the parser of the reference's answers
(tests/golden/kat_*.txt and, gzip-compressed, kat_zoo*.txt.gz, written by
`refdrv kat` / `refdrv katin`), the
oracle's hooks (oracle/cpuref.c cr_kat_*) applied to arrays of cases, and the
seeded random cases of the material zoo.

Layouts (one row per case), the oracle hooks':
  sampler (15)  cr_kat_sampler 0-8 (cos dir, pdf, pow-cos dir, pdf, pow_cos_pdf), cr_kat_triangle 9-11, cr_kat_strat 12-14
  frame (10)    cr_kat_frame 0-8, cr_kat_fresnel 9
  bsdf (26)     cr_kat_bsdf 0-24 (slot 25 unused), rows preset to BSDF_PRESET, plus a valid flag
  light (27)    cr_kat_light
  camera (7)    raster-to-world point 0-2, world-to-raster point 3-5, checkRaster 6
"""
import ctypes as C
import functools
import gzip
import os

import numpy as np

import _oracle
import _scenes
from winmad_rt import scenes

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# what a row of bsdf outputs holds before the call: only rows of invalid BSDFs keep it
BSDF_PRESET = np.zeros(26, F)
T_REFL, T_TRANS, T_DIFF, T_GLOSSY = 1, 2, 4, 8
# classes of tests/golden/kat_zoo_edges_in.f32 (make_golden.py ZOO_EDGE_CLASSES), last float of a record
EDGE_CLASSES = ("sampler", "frame", "fresnel", "tangent", "below", "mirror", "otherhemi", "r3z", "tir", "normal", "light")
# the zoo's materials with more than one lobe, and the sample types each can produce (scenes.ZOO_MATERIALS)
ZOO_MIXED = {4: {T_DIFF, T_GLOSSY}, 5: {T_DIFF, T_GLOSSY, T_REFL, T_TRANS}, 6: {T_REFL, T_TRANS},
             7: {T_REFL, T_TRANS}, 11: {T_DIFF, T_GLOSSY}}
ZOO_TIR = (5, 6, 7)  # refraction indices 1.5, 2.4, 0.75


def hx(t):
    return F(float.fromhex(t))


def _hx(tokens):
    return [float.fromhex(t) for t in tokens]


@functools.lru_cache(maxsize=None)
def parse(name):
    """tests/golden/<name>.txt -> {tag: arrays}; inputs and expected outputs in the layouts above."""
    rows = {}
    path = os.path.join(GOLD, name + ".txt")
    for line in (open(path) if os.path.exists(path) else gzip.open(path + ".gz", "rt")):
        t = line.split()
        rows.setdefault(t[0], []).append(t[1:])
    out = {}
    n = len(rows.get("cosh", []))
    if n:
        assert all(len(rows[k]) == n for k in ("pcosh", "tri", "strat"))
        cosh = np.array([_hx(a) for a in rows["cosh"]], F)
        pcosh = np.array([_hx(a) for a in rows["pcosh"]], F)
        tri = np.array([_hx(a) for a in rows["tri"]], F)
        strat = np.array([_hx(a[2:]) for a in rows["strat"]], F)
        for other in (pcosh, tri, strat):
            assert np.array_equal(other[:, 0:3].view(np.uint32), cosh[:, 0:3].view(np.uint32))
        out["sampler"] = {"u": cosh[:, 0:3].copy(), "power": pcosh[:, 3].copy(), "tri": tri[:, 3:12].copy(),
                          "k": np.array([int(a[0]) for a in rows["strat"]], np.int32),
                          "tot": np.array([int(a[1]) for a in rows["strat"]], np.int32),
                          "out": np.concatenate([cosh[:, 3:7], pcosh[:, 4:9], tri[:, 12:15], strat[:, 3:6]], axis=1)}
    if "frame" in rows:
        fr = np.array([_hx(a) for a in rows["frame"]], F)
        fs = np.array([_hx(a) for a in rows["fresnel"]], F)
        assert len(fr) == len(fs)
        out["frame"] = {"z": fr[:, 0:3].copy(), "ci": fs[:, 0].copy(), "idx": fs[:, 1].copy(),
                        "out": np.concatenate([fr[:, 3:12], fs[:, 2:3]], axis=1)}
    if "bsdf" in rows:
        b = rows["bsdf"]
        exp = np.tile(BSDF_PRESET, (len(b), 1))
        valid = np.array([int(a[14]) for a in b], np.int32)
        for i, a in enumerate(b):
            if not valid[i]:
                continue
            r = a[15:]
            assert r[8] == "f" and r[15] == "pdf" and r[18] == "smp" and len(r) == 28, a
            exp[i, 0] = float(r[0])
            exp[i, 1:8] = _hx(r[1:8])
            exp[i, 8:14] = _hx(r[9:15])
            exp[i, 14:16] = _hx(r[16:18])
            exp[i, 16] = float(r[19])
            exp[i, 17:25] = _hx(r[20:28])
        out["bsdf"] = {"mat": np.array([int(a[0]) for a in b], np.int32),
                       "inp": np.array([_hx(a[1:13]) for a in b], F), "valid": valid, "out": exp}
    if "illu" in rows:
        il = np.array([_hx(a[1:]) for a in rows["illu"]], F)
        em = np.array([_hx(a[1:]) for a in rows["emit"]], F)
        ra = np.array([_hx(a[1:]) for a in rows["rad"]], F)
        assert len(il) == len(em) == len(ra)
        out["light"] = {"li": np.array([int(a[0]) for a in rows["illu"]], np.int32),
                        "inp": np.concatenate([il[:, 0:6], em[:, 0:6], ra[:, 0:3]], axis=1),
                        "out": np.concatenate([il[:, 6:16], em[:, 6:18], ra[:, 6:11]], axis=1)}
    if "cam" in rows:
        c = np.array([_hx(a[:-1]) for a in rows["cam"]], F)
        out["cam"] = {"xy": c[:, 0:2].copy(), "ray": c[:, 2:8].copy(), "w": c[:, 8:11].copy(),
                      "ras": c[:, 11:14].copy(), "check": np.array([int(a[-1]) for a in rows["cam"]], np.int32)}
    return out


def edge_classes():
    """{kind: class name of each of its cases, in file order} of kat_zoo_edges_in.f32
    (record: kind, id, values, class; kinds: 0 sampler, 1 frame + fresnel, 2 bsdf, 3 light)."""
    recs = np.fromfile(os.path.join(GOLD, "kat_zoo_edges_in.f32"), F).reshape(-1, 20)
    return {name: np.array([EDGE_CLASSES[int(r[19])] for r in recs if int(r[0]) == kind])
            for kind, name in enumerate(("sampler", "frame", "bsdf", "light"))}


def same_bits(got, want, what, nan_equal=False):
    """Equal bit patterns (nan_equal: a NaN equals a NaN of any payload); reports the first rows that differ."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    u = np.uint64 if got.dtype.itemsize == 8 else np.uint32
    bad = got.view(u) != want.view(u)
    if nan_equal:
        bad &= ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        idx = np.argwhere(bad)
        lines = [f"{tuple(i)}: got {got[tuple(i)]!r} want {want[tuple(i)]!r}" for i in idx[:8]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ\n" + "\n".join(lines))
    return int(bad.size)


# ------------------------------------------------------------------ the oracle's hooks over arrays
_FP = C.POINTER(C.c_float)


def _at(a, row):
    return C.cast(a.ctypes.data + row * a.strides[0], _FP)


def oracle_sampler(u, power, tri, k, tot):
    L = _oracle.lib()
    u, tri = np.ascontiguousarray(u, F), np.ascontiguousarray(tri, F)
    n = len(u)
    out = np.zeros((n, 15), F)
    for i in range(n):
        o = _at(out, i)
        L.cr_kat_sampler(_at(u, i), float(power[i]), o)
        L.cr_kat_triangle(_at(u, i), _at(tri, i), C.cast(C.addressof(o.contents) + 36, _FP))
        L.cr_kat_strat(_at(u, i), int(k[i]), int(tot[i]), C.cast(C.addressof(o.contents) + 48, _FP))
    return out


def oracle_frame(z, ci, idx):
    L = _oracle.lib()
    z = np.ascontiguousarray(z, F)
    out = np.zeros((len(z), 10), F)
    for i in range(len(z)):
        L.cr_kat_frame(_at(z, i), _at(out, i))
        out[i, 9] = L.cr_kat_fresnel(float(ci[i]), float(idx[i]))
    return out


def oracle_bsdf(scene, mat, inp):
    inp = np.ascontiguousarray(inp, F)
    n = len(inp)
    out = np.ascontiguousarray(np.tile(BSDF_PRESET, (n, 1)))
    valid = np.zeros(n, np.int32)
    fn, h = scene.L.cr_kat_bsdf, scene.h
    base, st = inp.ctypes.data, inp.strides[0]
    for i in range(n):
        p = base + i * st
        valid[i] = fn(h, int(mat[i]), C.cast(p, _FP), C.cast(p + 12, _FP), C.cast(p + 24, _FP), C.cast(p + 36, _FP),
                      _at(out, i))
    return out, valid


def oracle_light(scene, li, inp):
    inp = np.ascontiguousarray(inp, F)
    n = len(inp)
    out = np.zeros((n, 27), F)
    fn, h = scene.L.cr_kat_light, scene.h
    base, st = inp.ctypes.data, inp.strides[0]
    for i in range(n):
        p = base + i * st
        fn(h, int(li[i]), C.cast(p, _FP), C.cast(p + 12, _FP), C.cast(p + 24, _FP), C.cast(p + 36, _FP),
           C.cast(p + 48, _FP), _at(out, i))
    return out


def oracle_camera(scene, xy, w):
    w = np.ascontiguousarray(w, F)
    n = len(w)
    out = np.zeros((n, 7), F)
    o10 = np.zeros(10, F)
    for i in range(n):
        scene.L.cr_kat_raster_to_world(scene.h, float(xy[i, 0]), float(xy[i, 1]), _at(out, i))
        scene.L.cr_kat_camera(scene.h, float(xy[i, 0]), float(xy[i, 1]), _at(w, i), _oracle.fptr(o10))
        out[i, 3:7] = o10[6:10]
    return out


# ------------------------------------------------------------------ seeded random cases on the zoo
N_RANDOM = 4000
NMAT = len(scenes.ZOO_MATERIALS) + 1  # with the reference's material 0


def _u24(rng, *shape):
    """RNG::randFloat's values: k / 2^24."""
    return (rng.integers(0, 1 << 24, shape).astype(np.float64) / 2.0 ** 24).astype(F)


def _dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def _tangent(n):
    """A unit vector perpendicular to each row of n."""
    t = np.cross(n, np.where(np.abs(n[:, 0:1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]]))
    return t / np.linalg.norm(t, axis=1, keepdims=True)


def random_bsdf_inputs(seed, n=N_RANDOM):
    """(n, 12) n, wi, wo, r3: directions uniform on the sphere; every 32nd wi lies
    within EPS of the tangent plane (an invalid BSDF, bsdf.h:75), every 8th wo is
    the mirror direction of wi, every 16th lies in the tangent plane."""
    rng = np.random.default_rng(seed)
    nrm, wi, wo = _dirs(rng, n).astype(np.float64), _dirs(rng, n).astype(np.float64), _dirs(rng, n).astype(np.float64)
    k = np.arange(n)
    flat = k % 32 == 5
    t = _tangent(nrm)
    wi[flat] = (t + nrm * rng.uniform(-0.9e-3, 0.9e-3, (n, 1)))[flat]
    mirror = k % 8 == 3
    wo[mirror] = (2 * nrm * (nrm * wi).sum(axis=1, keepdims=True) - wi)[mirror]
    graze = k % 16 == 9
    wo[graze] = (np.cross(nrm, t) + nrm * rng.uniform(-2e-3, 2e-3, (n, 1)))[graze]
    return np.concatenate([nrm.astype(F), wi.astype(F), wo.astype(F), _u24(rng, n, 3)], axis=1)


@functools.lru_cache(maxsize=None)
def zoo_random_cases():
    """The random cases of the GPU test, with the oracle's answers: N_RANDOM per
    zoo material, per light and for the samplers / frames / camera."""
    sc = _oracle.Scene(_scenes.zoo(24, 32))
    rng = np.random.default_rng(424242)
    c = {}
    mat = np.repeat(np.arange(1, NMAT, dtype=np.int32), N_RANDOM)
    inp = np.concatenate([random_bsdf_inputs(1000 + m) for m in range(1, NMAT)])
    out, valid = oracle_bsdf(sc, mat, inp)
    c["bsdf"] = {"mat": mat, "inp": inp, "out": out, "valid": valid}
    nl = sc.L.cr_scene_nlights(sc.h)
    li = np.repeat(np.arange(nl, dtype=np.int32), N_RANDOM)
    n = len(li)
    pos = (F(-1.3) + F(2.6) * _u24(rng, n, 3)).astype(F)
    linp = np.concatenate([pos, _u24(rng, n, 3), _u24(rng, n, 3), _u24(rng, n, 3), _dirs(rng, n)], axis=1)
    c["light"] = {"li": li, "inp": linp, "out": oracle_light(sc, li, linp)}
    n = N_RANDOM
    u = _u24(rng, n, 3)
    power = np.where(np.arange(n) % 2 == 0, rng.choice([0, 1, 3, 20, 90, 400], n), 1 + 200 * _u24(rng, n)).astype(F)
    tri = _u24(rng, n, 9)
    tot = rng.choice([1, 4, 16, 512], n).astype(np.int32)
    k = (rng.integers(0, 1 << 30, n) % tot).astype(np.int32)
    c["sampler"] = {"u": u, "power": power, "tri": tri, "k": k, "tot": tot, "out": oracle_sampler(u, power, tri, k, tot)}
    z = _dirs(rng, n).astype(np.float64)
    near = np.arange(n) % 16 == 0  # |z.x| within 1e-3 of 0.99, the tangent choice of frame.cpp:6
    x = rng.choice([-1, 1], n) * (0.99 + rng.uniform(-1e-3, 1e-3, n))
    phi = rng.uniform(0, 2 * np.pi, n)
    z[near] = np.stack([x, np.sqrt(1 - x * x) * np.cos(phi), np.sqrt(1 - x * x) * np.sin(phi)], axis=1)[near]
    z = (z * (0.25 + 4 * rng.random((n, 1)))).astype(F)  # frame_from_z normalises
    ci = (2 * _u24(rng, n) - 1).astype(F)
    idx = np.where(np.arange(n) % 2 == 0, rng.choice([0.75, 1.0, 1.5, 2.4, -1.0], n), 1 + _u24(rng, n)).astype(F)
    ci[(ci == 0) & (idx == 1)] = F(0.5)  # 0 / 0 in fresnel.cpp: no BSDF has cos 0
    c["frame"] = {"z": z, "ci": ci, "idx": idx, "out": oracle_frame(z, ci, idx)}
    xy = ((F(-0.1) + F(1.2) * _u24(rng, n, 2)) * np.array([32, 24], F)).astype(F)  # xres 32 (height), yres 24
    w = (F(-1.3) + F(2.6) * _u24(rng, n, 3)).astype(F)
    c["cam"] = {"xy": xy, "w": w, "out": oracle_camera(sc, xy, w)}
    return c


def check_zoo_random_cases(c):
    """What the oracle's answers must show for the random cases not to pass empty
    (returns the counts for the record)."""
    stats = {"nonfinite": 0}
    for k in ("bsdf", "light", "sampler", "frame", "cam"):
        stats["nonfinite"] += int((~np.isfinite(c[k]["out"])).sum())
    assert stats["nonfinite"] == 0, stats
    b = c["bsdf"]
    stats["bsdf_cases"], stats["bsdf_invalid"] = len(b["valid"]), int((b["valid"] == 0).sum())
    assert stats["bsdf_invalid"] >= 0.01 * len(b["valid"]), stats
    stats["types"] = {}
    for m, types in ZOO_MIXED.items():
        sel = (b["mat"] == m) & (b["valid"] == 1)
        ty = b["out"][sel, 16].astype(int)
        frac = {t: float((ty == t).mean()) for t in sorted(set(ty.tolist()) | types)}
        stats["types"][m] = frac
        assert set(frac) == types, (m, frac)
        assert min(frac.values()) >= 0.05, (m, frac)
    return stats


def check_zoo_edge_cases(classes, e):
    """At least 8 cases per material (or light) of every edge class took the
    branch the class aims at, read from the oracle's answers `e` (the layouts
    above, in file order per kind).  Returns the counts."""
    b = e["bsdf"]
    cls = classes["bsdf"]
    assert len(cls) == len(b["mat"]) and len(classes["frame"]) == len(e["frame"]["out"])
    o, v = b["out"], b["valid"] == 1
    cw_set = o[:, 11] != F(-7)
    took = {
        "tangent": ~v,                                                  # cmpf(wi.z) == 0: no BSDF
        "below": v & (o[:, 1] < 0),                                     # cosWi < 0
        "mirror": v & cw_set & (np.abs(o[:, 11] - np.abs(o[:, 1])) < 1e-5),  # wo.z == wi.z up to rounding
        "otherhemi": v & ~cw_set,                                       # f returns before it writes cosWo
        "r3z": v & (o[:, 16] != F(-7)),                                 # a component was chosen
        "tir": v & (o[:, 3] == F(1)),                                   # Fresnel reflectance 1: cosT = 0
        "normal": v,
    }
    counts = {}
    for m in range(1, NMAT):
        for name, hit in took.items():
            if name == "tir" and m not in ZOO_TIR:
                continue
            k = int((hit & (cls == name) & (b["mat"] == m)).sum())
            counts[(name, m)] = k
            assert k >= 8, (name, m, k)
        # the r3.z cases reach every component the material's probabilities allow
        sel = v & (cls == "r3z") & (b["mat"] == m)
        reach = set()
        for row in o[sel]:
            pd, pg, pr = row[4], row[5], row[6]
            ends = (F(0), pd, F(pd + pg), F(F(pd + pg) + pr), F(1))  # r3.z < 1
            reach |= {t for t, lo, hi in zip((T_DIFF, T_GLOSSY, T_REFL, T_TRANS), ends, ends[1:]) if hi > lo}
        assert set(o[sel, 16].astype(int).tolist()) == reach, (m, reach)
    fr = e["frame"]["out"][classes["frame"] == "frame"]
    up = (fr[:, 4] == 0) & (fr[:, 3] != 0)  # tangent (0, 1, 0): y = normalize(-z.z, 0, z.x)
    counts[("frame", "|z.x| > 0.99")], counts[("frame", "|z.x| <= 0.99")] = int(up.sum()), int((~up).sum())
    assert up.sum() >= 8 and (~up).sum() >= 8, counts
    li = e["light"]
    for l in sorted(set(li["li"].tolist())):
        k = int(((li["li"] == l) & (li["out"][:, 7] == 0) & ~li["out"][:, 0:3].any(axis=1)).sum())
        counts[("light behind / in plane", l)] = k
        assert k >= 8, (l, k)
    return counts
