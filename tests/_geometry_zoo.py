"""The geometry zoo: eight tiny scenes of the geometry clean meshes never have
(test infrastructure, in the style of _tiny_scenes.py; DESIGN.md 4b lists what
each family is for).

Every scene is z-up: a two-triangle diffuse floor at z = -3, the family's
geometry around the origin (one diffuse and one glass material), an area-light
triangle at z = 6 whose normal points down at the geometry, and a camera at
(1.3, -12, 3.1) looking at the geometry.  Everything is a closed form or drawn
from random.Random(seed), and every float is written with %r, so the files are
the same wherever they are written.

    scene(name)        the .scene file (32 x 32), written into _scenes._DIR
    primitives(name)   every triangle (n, 3, 3) and sphere (m, 4) as float32 data
    aim_points(name)   the family's vertices (first) and, for spheres, centres and poles
"""
import math
import os
import random

import numpy as np

import _scenes
from winmad_rt import scenes

NAMES = ("degenerate", "duplicates", "crowd", "axisgrid", "slivers", "scales", "fan", "spheremix")
FAR = ("duplicates", "crowd", "fan")  # corpora with a second, `far` half (tests/golden/make_golden.py)

FLOOR_Z = -3.0
FLOOR = [((-8.0, -8.0, FLOOR_Z), (8.0, -8.0, FLOOR_Z), (8.0, 8.0, FLOOR_Z)),
         ((-8.0, -8.0, FLOOR_Z), (8.0, 8.0, FLOOR_Z), (-8.0, 8.0, FLOOR_Z))]  # normal +z
LIGHT = [((-1.5, 1.5, 6.0), (1.5, -1.5, 6.0), (-1.5, -1.5, 6.0))]              # normal -z, towards the geometry
CAMERA_POS, CAMERA_AT = (1.3, -12.0, 3.1), (0.0, 0.0, -0.5)
DIFFUSE, GLASS = 1, 2


def _rnd(rng, lo, hi):
    return tuple(rng.uniform(lo, hi) for _ in range(3))


def _add(a, b, s=1.0):
    return tuple(x + s * y for x, y in zip(a, b))


def _degenerate():
    rng = random.Random(101)
    d, g = [], []
    for k in range(24):  # valid triangles
        p = _rnd(rng, -2.0, 2.0)
        (g if k % 6 == 5 else d).append((p, _add(p, _rnd(rng, -1.2, 1.2)), _add(p, _rnd(rng, -1.2, 1.2))))
    for k in range(5):
        p, q = _rnd(rng, -2.0, 2.0), _rnd(rng, -2.0, 2.0)
        d.append(((p, p, q), (p, q, p), (q, p, p))[k % 3])           # two equal vertices
        d.append((p, _add(p, _add(q, p, -1.0), 0.5), q))             # three collinear vertices (midpoint)
        d.append((p, q, _add(p, _add(q, p, -1.0), 2.0)))             # collinear, the third beyond the second
        d.append((q, q, q))                                         # three equal vertices
    # zero-area triangles lying inside valid ones, and sharing their vertices
    a, b, c = d[0]
    d.append((a, b, b))
    d.append((a, _add(a, _add(b, a, -1.0), 0.25), _add(a, _add(b, a, -1.0), 0.75)))
    return d, g, []


def _duplicates():
    t = ((-2.0, 0.0, -1.0), (0.5, 0.0, -1.0), (-0.75, 0.0, 1.75))            # in the plane y = 0
    u = ((-1.0, 0.0, -0.25), (1.5, 0.0, -0.25), (0.25, 0.0, 2.25))           # coplanar, overlaps t
    rev = lambda x: (x[0], x[2], x[1])
    s = ((0.5, 1.0, -2.0), (2.25, 2.0, -1.5), (1.0, 1.75, 0.5))              # a tilted plane
    e1, e2 = _add(s[1], s[0], -1.0), _add(s[2], s[0], -1.0)
    v = tuple(_add(_add(s[0], e1, a), e2, b) for a, b in ((0.25, 0.25), (1.25, 0.0), (0.0, 1.25)))  # coplanar with s
    w = ((-2.25, -1.5, -2.5), (-0.5, -1.0, -2.25), (-1.5, -2.0, -0.75))      # twice, nothing else on it
    return [t, t, rev(t), u, s, v, w, w], [rev(s)], []


def _crowd():
    t = ((-2.0, 0.5, -1.5), (-0.25, -0.5, -1.0), (-1.25, 0.25, 1.25))
    d = [t] * 12
    # nine coplanar triangles (plane x + y = 1.5), each turned a little about the group's centre
    c, ex, ez = (1.0, 0.5, 0.0), (math.sqrt(0.5), -math.sqrt(0.5), 0.0), (0.0, 0.0, 1.0)
    g = []
    for k in range(9):
        tri = []
        for j in range(3):
            a = 2.0 * math.pi * j / 3.0 + 0.07 * k
            r = 1.5 - 0.05 * k
            tri.append(_add(_add(c, ex, r * math.cos(a)), ez, r * math.sin(a)))
        (g if k == 8 else d).append(tuple(tri))
    return d, g, []


def _axisgrid():
    d, g = [], []
    for axis in range(3):
        for i in range(-2, 2):
            for j in range(-2, 2):
                def p(a, b):
                    q = [float(a), float(b)]
                    q.insert(axis, 0.0)
                    return tuple(q)
                quad = (p(i, j), p(i + 1, j), p(i + 1, j + 1), p(i, j + 1))
                (g if axis == 1 else d).extend([(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])])
    return d, g, []


def _slivers():
    rng = random.Random(505)
    d, g = [], []
    for k in range(40):
        p = _rnd(rng, -2.0, 2.0)
        e = _rnd(rng, -1.0, 1.0)
        n = math.sqrt(sum(x * x for x in e))
        q = _add(p, e, rng.uniform(1.0, 4.0) / n)
        r = _add(p, _rnd(rng, -5e-7, 5e-7))
        (g if k % 8 == 7 else d).append((p, q, r))
    return d, g, []


def _scales():
    rng = random.Random(606)
    e = 4.0e5
    d = [((-0.5 * e, -e / (2.0 * math.sqrt(3.0)), -1.0), (0.5 * e, -e / (2.0 * math.sqrt(3.0)), -1.0),
          (0.0, e / math.sqrt(3.0), -1.0))]
    g = []
    for k in range(60):
        c = (rng.uniform(-2.0, 2.0), rng.uniform(-2.0, 2.0), rng.uniform(-0.99, 1.5))
        a0 = rng.uniform(0.0, 2.0 * math.pi)
        u, v = _rnd(rng, -1.0, 1.0), _rnd(rng, -1.0, 1.0)
        un = math.sqrt(sum(x * x for x in u))
        u = tuple(x / un for x in u)
        w = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
        wn = math.sqrt(sum(x * x for x in w))
        w = tuple(x / wn for x in w)
        r = 1e-4 / math.sqrt(3.0)
        tri = tuple(_add(_add(c, u, r * math.cos(a0 + 2.0 * math.pi * j / 3.0)), w,
                         r * math.sin(a0 + 2.0 * math.pi * j / 3.0)) for j in range(3))
        (g if k % 10 == 9 else d).append(tri)
    return d, g, []


def _fan():
    hub = (0.0, 0.0, 0.0)
    n = 600
    golden = math.pi * (3.0 - math.sqrt(5.0))
    pts = []
    for k in range(n + 1):
        z = 1.0 - 2.0 * (k + 0.5) / (n + 1)
        r = math.sqrt(1.0 - z * z)
        pts.append((2.5 * r * math.cos(golden * k), 2.5 * r * math.sin(golden * k), 2.5 * z))
    d, g = [], []
    for k in range(n):
        (g if k % 12 == 11 else d).append((hub, pts[k], pts[k + 1]))
    return d, g, []


def _spheremix():
    d = [((0.25, -1.0, -1.5), (2.25, -0.5, -1.25), (1.25, 0.5, 1.0))]  # cut by the sphere at (1.25, -0.25, -0.5)
    spheres = [((-1.25, 0.0, 0.75), 0.75, DIFFUSE),    # concentric pair: outer
               ((-1.25, 0.0, 0.75), 0.375, GLASS),     # ... inner
               ((-1.25, 0.0, 0.75), 0.75, DIFFUSE),    # coincident with the outer one
               ((-1.5, -1.5, -1.5), 0.625, GLASS),     # two intersecting spheres
               ((-0.75, -1.5, -1.5), 0.5, DIFFUSE),
               ((1.25, -0.25, -0.5), 0.5, GLASS),      # cuts the triangle
               ((0.5, 1.5, FLOOR_Z + 0.5), 0.5, DIFFUSE),  # rests tangent on the floor
               ((0.0, -1.0, 1.0), 1e-4, DIFFUSE)]      # tiny
    return d, [], spheres


_BUILD = {"degenerate": _degenerate, "duplicates": _duplicates, "crowd": _crowd, "axisgrid": _axisgrid,
          "slivers": _slivers, "scales": _scales, "fan": _fan, "spheremix": _spheremix}
_made = {}


def geometry(name):
    """(diffuse triangles, glass triangles, spheres (centre, radius, material)) of a family."""
    if name not in _made:
        _made[name] = _BUILD[name]()
    return _made[name]


def _write_obj(fname, tris):
    p = os.path.join(_scenes._DIR, fname)
    if not os.path.exists(p):
        with open(p, "w") as f:
            for t in tris:
                for v in t:
                    f.write("v %r %r %r\n" % v)
            for k in range(len(tris)):
                f.write("f %d %d %d\n" % (3 * k + 1, 3 * k + 2, 3 * k + 3))
    return p


def scene(name, W=32, H=32):
    """The scene file of a family (objects in the order floor, diffuse, glass,
    spheres, light)."""
    d, g, spheres = geometry(name)
    fwd = [b - a for a, b in zip(CAMERA_POS, CAMERA_AT)]
    n = math.sqrt(sum(x * x for x in fwd))
    fwd = [x / n for x in fwd]
    dz = fwd[2]
    up = [-dz * fwd[0], -dz * fwd[1], 1.0 - dz * fwd[2]]  # z made orthogonal to forward
    n = math.sqrt(sum(x * x for x in up))
    up = [x / n for x in up]
    text = "<scene>\n"
    text += scenes._camera(tuple(map(repr, CAMERA_POS)), tuple(map(repr, fwd)), tuple(map(repr, up)), H, W, 40)
    text += scenes._mat()
    text += scenes._mat(d=("0.7", "0.7", "0.7"))
    text += scenes._mat(s=("1", "1", "1"), n="1.5")
    text += scenes._obj(_write_obj("geozoo_floor.obj", FLOOR), DIFFUSE)
    if d:
        text += scenes._obj(_write_obj(f"geozoo_{name}_d.obj", d), DIFFUSE)
    if g:
        text += scenes._obj(_write_obj(f"geozoo_{name}_g.obj", g), GLASS)
    for c, r, m in spheres:
        text += scenes._sphere(tuple(map(repr, c)), repr(r), m)
    text += scenes._area(_write_obj("geozoo_light.obj", LIGHT), 25)
    text += "</scene>\n"
    return _scenes.path(f"geozoo_{name}_{W}x{H}.scene", text)


def primitives(name):
    """Every triangle of the scene, floor and light included, as (n, 3, 3), and
    every sphere as (m, 4) = centre, radius: the float32 values the loaders read."""
    d, g, spheres = geometry(name)
    tris = np.array(FLOOR + d + g + LIGHT, np.float32).reshape(-1, 3, 3)
    sph = np.array([(*c, r) for c, r, _ in spheres], np.float32).reshape(-1, 4)
    return tris, sph


def aim_points(name):
    """(corners, segments): the points the corpus' first quarter aims at -- every
    triangle corner of the family (one entry per corner, so a shared vertex is
    drawn as often as it is used) and, for spheres, centres and the six poles --
    and the corner pairs (edges of one triangle) of its second quarter."""
    d, g, spheres = geometry(name)
    tris = np.array(d + g, np.float32).reshape(-1, 3, 3)
    pts = [tris.reshape(-1, 3)]
    seg = [np.stack([tris[:, a], tris[:, b]], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))]
    for c, r, _ in spheres:
        c = np.array(c, np.float32)
        poles = np.array([c + np.float32(r) * np.eye(3, dtype=np.float32)[k] * s for k in range(3) for s in (1, -1)],
                         np.float32)
        pts += [c[None], poles]
        pairs = [(a, b) for a in range(6) for b in range(a + 1, 6)]  # diameters and chords: points inside the sphere
        seg.append(np.stack([poles[[a for a, _ in pairs]], poles[[b for _, b in pairs]]], axis=1))
    return np.concatenate(pts).astype(np.float32), np.concatenate(seg).astype(np.float32)


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_fixtures = {}


def fixture(name):
    """The committed corpus of a family and the reference's answers to it
    (tests/golden/geozoo_<name>.f32 / .txt.gz, made by make_golden.py geozoo):
    rays (n, 9) = o, d, occlusion target; prim (n,), -1 for a miss; vals (n, 7)
    = t, p, n as float32; inside, mat and occ (n,).  Read once, never changed."""
    if name not in _fixtures:
        import gzip
        rays = np.fromfile(os.path.join(GOLD, f"geozoo_{name}.f32"), np.float32).reshape(-1, 9)
        n = rays.shape[0]
        fx = {"rays": rays, "prim": np.full(n, -1, np.int32), "vals": np.zeros((n, 7), np.float32),
              "inside": np.zeros(n, np.int32), "mat": np.zeros(n, np.int32), "occ": np.zeros(n, np.uint8)}
        with gzip.open(os.path.join(GOLD, f"geozoo_{name}.txt.gz"), "rt") as f:
            lines = f.read().splitlines()
        assert len(lines) == n, (name, len(lines), n)
        for k, line in enumerate(lines):
            tok = line.split()
            fx["occ"][k] = int(tok[-1])
            if tok[0] != "-1":
                fx["prim"][k] = int(tok[0])
                fx["vals"][k] = [np.float32(float.fromhex(t)) for t in tok[1:8]]
                fx["inside"][k], fx["mat"][k] = int(tok[8]), int(tok[9])
        for a in fx.values():
            a.setflags(write=False)
        _fixtures[name] = fx
    return _fixtures[name]


def compare(label, hits, occ, fx):
    """The GPU tests' comparison with a fixture (test_gpu._check_golden_corpus' on a zoo fixture): primitive,
    t bit for bit, p and n, inside, material, and the occlusion answers."""
    bad = np.nonzero(hits["prim"] != fx["prim"])[0]
    assert bad.size == 0, (label, "prim", int(bad.size), bad[:8].tolist(), hits["prim"][bad[:8]].tolist(),
                           fx["prim"][bad[:8]].tolist())
    hit = fx["prim"] >= 0
    got = np.concatenate([hits["t"][:, None], hits["p"], hits["n"]], axis=1).astype(np.float32)
    bad = np.nonzero(hit & (got[:, 0].view(np.uint32) != fx["vals"][:, 0].view(np.uint32)))[0]
    assert bad.size == 0, (label, "t", int(bad.size), bad[:8].tolist(), got[bad[:4], 0], fx["vals"][bad[:4], 0])
    # p and n: the same bits, but a zero may carry either sign and a NaN any payload (the normal of a
    # zero-area triangle the reference reports is NaN): _check_golden_corpus' equal floats, NaN included
    want = fx["vals"]
    same = (got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0)) | (np.isnan(got) & np.isnan(want))
    bad = np.nonzero(hit & ~same.all(axis=1))[0]
    assert bad.size == 0, (label, "p n", int(bad.size), bad[:8].tolist(), got[bad[:2]], fx["vals"][bad[:2]])
    assert np.array_equal(hits["inside"][hit], fx["inside"][hit]), (label, "inside")
    assert np.array_equal(hits["mat_id"][hit], fx["mat"][hit]), (label, "material")
    bad = np.nonzero(occ != fx["occ"])[0]
    assert bad.size == 0, (label, "occluded", int(bad.size), bad[:8].tolist())


def brute_force_hits(name, rays):
    """t of every primitive along every ray, float64 Moeller-Trumbore and the
    sphere quadratic over all primitives ((n, nprims), inf where there is no hit
    beyond 1e-6), triangles first.  For counting what a corpus exercises only:
    never the truth of a test."""
    tris, sph = primitives(name)
    o = rays[:, 0:3].astype(np.float64)[:, None, :]
    d = rays[:, 3:6].astype(np.float64)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True))[:, None, :]
    p0 = tris[:, 0].astype(np.float64)[None]
    e1 = (tris[:, 1].astype(np.float64) - tris[:, 0])[None]
    e2 = (tris[:, 2].astype(np.float64) - tris[:, 0])[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        pv = np.cross(d, e2)
        det = (e1 * pv).sum(-1)
        tv = o - p0
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1)
        v = (d * qv).sum(-1) / det
        t = (e2 * qv).sum(-1) / det
        area = np.linalg.norm(np.cross(e1, e2), axis=-1)
        tol = 1e-7
        ok = (np.abs(det) > 1e-12 * area) & (area > 0) & (u >= -tol) & (v >= -tol) & (u + v <= 1 + tol) & (t > 1e-6)
    out = [np.where(ok, t, np.inf)]
    if len(sph):
        c, r = sph[:, :3].astype(np.float64)[None], sph[:, 3].astype(np.float64)[None]
        oc = o - c
        b = (oc * d).sum(-1)
        disc = b * b - ((oc * oc).sum(-1) - r * r)
        with np.errstate(invalid="ignore"):
            sq = np.sqrt(disc)
        t0, t1 = -b - sq, -b + sq
        ts = np.where(t0 > 1e-6, t0, np.where(t1 > 1e-6, t1, np.inf))
        out.append(np.where(disc >= 0, ts, np.inf))
    return np.concatenate(out, axis=1)
