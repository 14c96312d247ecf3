"""The geometry zoo on the CPU (tests/_geometry_zoo.py): scenes of
degenerate, coincident, crowded, axis-aligned, needle-thin, wildly scaled and
fanned triangles and of nested / coincident / tangent / tiny spheres, against
the reference's own answers (tests/golden/geozoo_*, golden_geozoo.json, made by
tests/golden/make_golden.py geozoo).

  * the product's loader and KD build give the reference's dump, bit for bit;
  * the oracle's trace equals the reference's on every corpus, bit for bit
    (the film tests of tests/test_gpu_geometry_zoo.py lean on the oracle);
  * the BVH built on these scenes keeps its structure (binary, 4- and 8-wide);
  * the cell filter drops no leaf the KD walk reaches on the corpora's rays;
  * the corpora exercise what they are for: counts from a float64 brute force
    over all primitives (for counting only -- the truth is the reference's).
"""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import _geometry_zoo as gz
import _oracle
import _scenes
import test_bvh_host
import test_cell_filter
from winmad_rt import native, scenes

GOLD = gz.GOLD
META = json.load(open(os.path.join(GOLD, "golden_geozoo.json")))
WINDOW = 3e-3  # the tie window of the BVH mode's proof is 3 EPS
# wrf::build_fast declines a scene holding a triangle with non-zero, nearly parallel edges (wr_bvh.h
# kSliverSin; DESIGN.md 4b, slivers): `degenerate` has the collinear ones
DECLINED = ("degenerate",)


def test_fixture_list_is_the_zoo():
    assert tuple(META) == gz.NAMES
    for name in gz.NAMES:
        n = gz.fixture(name)["rays"].shape[0]
        assert n == (2048 if name in gz.FAR else 1024), (name, n)
        for ext in ("f32", "txt.gz"):
            assert os.path.getsize(os.path.join(GOLD, f"geozoo_{name}.{ext}")) < 100_000, (name, ext)
        tris, sph = gz.primitives(name)
        assert len(tris) + len(sph) == META[name]["nobjs"] <= 1000, name


@pytest.mark.parametrize("name", gz.NAMES)
def test_product_loader_and_kdtree_match_reference(name, tmp_path):
    s = native.Scene(gz.scene(name))
    txt = s.dump(str(tmp_path / "p.txt"))
    m = META[name]
    assert hashlib.sha256(txt.encode()).hexdigest() == m["scene_sha256"]
    info = s.info()
    assert info["nprims"] == m["nobjs"]
    assert info["kd_inner"] == m["inner"] and info["kd_leaves"] == m["leaves"]
    assert info["kd_refs"] == m["refs"] and info["kd_depth_max"] == m["depmax"]
    assert 1 <= info["kd_max_stack"] <= m["depmax"]


@pytest.mark.parametrize("name", gz.NAMES)
def test_oracle_scene_and_trace_bit_exact(name, tmp_path):
    """cr_trace == Scene::intersect + Scene::occluded of the reference on the
    zoo: prim, t, p, n, inside, material and the occlusion answer of every ray."""
    s = _oracle.Scene(gz.scene(name))
    assert hashlib.sha256(s.dump(str(tmp_path / "d.txt")).encode()).hexdigest() == META[name]["scene_sha256"]
    fx = gz.fixture(name)
    oi, of, oc, st = s.trace(fx["rays"])
    assert st.closest_rays == st.shadow_rays == fx["rays"].shape[0]
    bad = np.nonzero(oi[:, 0] != fx["prim"])[0]
    assert bad.size == 0, (name, "prim", bad[:8], oi[bad[:8], 0], fx["prim"][bad[:8]])
    hit = fx["prim"] >= 0
    bad = np.nonzero(hit & (of.view(np.uint32) != fx["vals"].view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, (name, "t p n", bad[:8])
    assert np.array_equal(oi[hit, 1], fx["inside"][hit]) and np.array_equal(oi[hit, 2], fx["mat"][hit])
    bad = np.nonzero(oc != fx["occ"])[0]
    assert bad.size == 0, (name, "occluded", bad[:8])


def test_a_damaged_fixture_is_noticed():
    """One ray's expected primitive changed: the comparison above must see it."""
    name = "duplicates"
    fx = gz.fixture(name)
    oi = _oracle.Scene(gz.scene(name)).trace(fx["rays"])[0]
    prim = fx["prim"].copy()
    k = int(np.nonzero(prim >= 0)[0][17])
    prim[k] += 1
    assert np.array_equal(oi[:, 0], fx["prim"])
    assert np.nonzero(oi[:, 0] != prim)[0].tolist() == [k]


@pytest.mark.parametrize("wide", [None, 4, 8], ids=["binary", "wide4", "wide8"])
@pytest.mark.parametrize("name", gz.NAMES)
def test_bvh_structure(name, wide):
    r = subprocess.run([test_bvh_host.checker(wide), gz.scene(name)], capture_output=True, text=True, timeout=300)
    if name in DECLINED:
        assert r.returncode != 0 and r.stdout.startswith("FAIL build refused: a triangle with nearly collinear vertices"), \
            r.stdout + r.stderr
        return
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    if name == "fan" and wide is None:  # a primitive in more than 16 KD leaves: the scan list, first_leaves_wave
        print(r.stdout.strip())
        assert int(r.stdout.split(" >16: ")[1].split(",")[0]) > 0, r.stdout


@pytest.mark.parametrize("name", gz.NAMES)
def test_cell_filter_drops_no_reached_leaf(name, tmp_path):
    """cell_may_be_reached (wr_fast.h) over the leaves the KD walk reaches on the
    corpus' rays (tests/native/cell_filter_check.cpp, --rays: o, d, tmin, tmax)."""
    rays = gz.fixture(name)["rays"]
    d = rays[:, 3:6].astype(np.float32)
    l = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    r8 = native.rays_from_arrays(rays[:, 0:3], (d / l[:, None]).astype(np.float32))
    p = tmp_path / "rays8.f32"
    r8.tofile(str(p))
    rc, out = test_cell_filter.run(gz.scene(name), "--rays", str(p))
    assert rc == 0, out[-3000:]
    last = out.strip().splitlines()[-1]
    assert last.startswith(f"rays {rays.shape[0]} ") and " dropped 0 " in last, last


@pytest.mark.parametrize("maker", [lambda: _scenes.torus(64, 64), lambda: _scenes.cbox(64, 48), test_bvh_host.small_torus,
                                   lambda: _scenes.spheres(64, 64)],
                         ids=["torus", "cbox_dragon", "synthetic_torus_40k", "spheres"])
def test_standard_scenes_are_still_accepted(maker):
    """The sliver rule declines none of the four standard scenes nor the 40k torus
    (test_bvh_host.test_bvh_structure checks their trees; here: not refused, and
    the thinnest corner of any of their triangles is 300 times the rule's)."""
    r = subprocess.run([test_bvh_host.checker(), maker()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK") and "refused" not in r.stdout, r.stdout + r.stderr


def test_synthetic_1m_torus_has_no_sliver():
    """The 1M-triangle torus (tests/test_gpu_bvh.py searches its 4-wide tree): the
    sine of every triangle's corner at p0, from the generator's own vertices."""
    import io
    p = os.path.join(_scenes._DIR, "torus1m.obj")
    if not os.path.exists(p):
        scenes.synth_torus_obj(p)
    with open(p) as f:
        lines = f.read().splitlines()
    v = np.loadtxt(io.StringIO("\n".join(l[2:] for l in lines if l.startswith("v "))), dtype=np.float32)
    f = np.loadtxt(io.StringIO("\n".join(l[2:] for l in lines if l.startswith("f "))), dtype=np.int64) - 1
    e1 = (v[f[:, 1]] - v[f[:, 0]]).astype(np.float64)
    e2 = (v[f[:, 2]] - v[f[:, 0]]).astype(np.float64)
    sin = np.linalg.norm(np.cross(e1, e2), axis=1) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
    assert len(f) == 1_000_000 and sin.min() > 1e-3, sin.min()


# ------------------------------------------------------------ the corpora are not thin
_counts = {}


def counts(name):
    """What a corpus exercises, by brute force: per ray the smallest hit and
    how many other primitives are hit within WINDOW of it."""
    if name not in _counts:
        fx = gz.fixture(name)
        t = gz.brute_force_hits(name, fx["rays"])
        tmin = t.min(axis=1)
        hit = np.isfinite(tmin)
        with np.errstate(invalid="ignore"):
            others = (np.abs(t - tmin[:, None]) <= WINDOW).sum(axis=1) - 1
        ntri = len(gz.primitives(name)[0])
        first = t.argmin(axis=1)
        with np.errstate(invalid="ignore"):
            sph_near = (np.abs(t[:, ntri:] - tmin[:, None]) <= 1e-6).sum(axis=1)  # zeros where there is no sphere
        _counts[name] = {"tmin": tmin, "hit": hit, "others": np.where(hit, others, 0),
                         "sphere": hit & (first >= ntri), "sph_same": np.where(hit, sph_near, 0)}
    return _counts[name]


@pytest.mark.parametrize("name", gz.NAMES)
def test_corpus_is_not_thin(name):
    c = counts(name)
    fx = gz.fixture(name)
    n = len(c["hit"])
    ref_hit = fx["prim"] >= 0
    line = {"rays": n, "hits": int(c["hit"].sum()), "reference hits": int(ref_hit.sum()),
            "exactly 1 other": int((c["others"] == 1).sum()), "exactly 2 others": int((c["others"] == 2).sum()),
            ">= 9 in window": int((c["others"] + 1 >= 9).sum()), "occluded": int(fx["occ"].sum())}
    # at least 25 % hits and 10 % misses: by the brute force and by the reference itself
    for h in (c["hit"], ref_hit):
        assert h.sum() >= 0.25 * n and (~h).sum() >= 0.10 * n, (name, line)
    assert 0.05 * n <= fx["occ"].sum() <= 0.95 * n, (name, line)  # both occlusion answers
    # the four quarters of each half all contribute hits
    for q in range(n // 256):
        assert ref_hit[256 * q:256 * (q + 1)].sum() >= 16, (name, "quarter", q, line)
    if name == "duplicates":
        assert line["exactly 1 other"] >= 100 and line["exactly 2 others"] >= 50, line
    if name in ("crowd", "fan"):
        assert line[">= 9 in window"] >= 50, line
    if name in gz.FAR:
        far = np.arange(n) >= 1024
        line["far hits t >= 4096"] = int((c["hit"] & far & (c["tmin"] >= 4096)).sum())
        line["far reference hits t >= 4096"] = int((ref_hit & far & (fx["vals"][:, 0] >= 4096)).sum())
        assert line["far hits t >= 4096"] >= 200 and line["far reference hits t >= 4096"] >= 200, line
        o = fx["rays"][far, 0:3].astype(np.float64)
        dist = np.linalg.norm(o, axis=1)
        assert ((dist >= 4990) & (dist <= 20010)).sum() == 512, (name, "far origins")
    if name == "spheremix":
        line["sphere hits"] = int(c["sphere"].sum())
        line["coincident sphere hits"] = int((c["sphere"] & (c["sph_same"] >= 2)).sum())
        assert line["sphere hits"] >= 100 and line["coincident sphere hits"] >= 20, line
    if name == "degenerate":  # the reference never reports a zero-area triangle
        tris, _ = gz.primitives(name)
        area = np.linalg.norm(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]), axis=1)
        line["zero-area triangles"] = int((area == 0).sum())
        assert line["zero-area triangles"] >= 12, line
    if name == "axisgrid":  # rays inside a split plane holding geometry: a zero direction component and o on the plane
        r = fx["rays"][768:]
        inplane = ((r[:, 3:6] == 0) & (r[:, 0:3] == 0)).any(axis=1)
        line["axis rays in a grid plane"] = int(inplane.sum())
        assert line["axis rays in a grid plane"] >= 20, line
    print(name, line)
