"""The geometry zoo on the GPU (tests/_geometry_zoo.py): every
traversal mode must return the reference's (t, primitive) bit for bit on
degenerate, coincident, crowded, axis-aligned, needle-thin, wildly scaled and
fanned triangles and on nested / coincident / tangent / tiny spheres, for rays
from nearby and from 5,000 to 20,000 units away.

No tolerance anywhere but the film gates of tests/_parity.py:
  * the reference's own answers (tests/golden/geozoo_*, CPU-checked by
    tests/test_geometry_zoo_host.py) against the KD walk, its dense variant,
    the verified BVH on the binary and the 4-wide tree, and the wave KD walk,
    through the host calls and the device-array calls;
  * 20,000-ray corpora derived on each scene (tests/test_gpu_bvh.py's extension,
    shadow and plane-grazing rays): the BVH modes and the wave walk against
    the KD walk of the same library;
  * 32 x 32 BDPT / PT / VCM films against the oracle, and one BDPT render per
    tree with every ray verified against the KD walk inside the library.
"""
import numpy as np
import pytest

import _geometry_zoo as gz
import _oracle
from _geometry_zoo import compare as _compare
from _parity import assert_film_parity, assert_ray_counts
from test_gpu import normalize_f32
from test_gpu_bvh import _corpus, _plane_grazing_rays, _same_hits
from winmad_rt import native

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W = H = 32
# mode: (trace mode of the context, environment around its creation)
MODES = {"kd_walk": ("TRACE_REFERENCE", {}),
         "kd_walk_dense": ("TRACE_REFERENCE", {"WR_TRACE_DENSE": "1"}),
         "bvh": ("TRACE_BVH", {}),
         "bvh_wide4": ("TRACE_BVH", {"WR_BVH_WIDE": "4"}),
         "wave_walk": ("TRACE_BVH", {"WR_BVH_DIAG": "256"})}
# build_fast declines a scene with a sliver triangle (wr_bvh.h kSliverSin): its contexts keep
# the KD walk, which must give the fixtures' answers in every "mode"
DECLINED = ("degenerate",)
KNOBS = ("WR_TRACE_DENSE", "WR_BVH_WIDE", "WR_BVH_DIAG", "WR_BVH_VERIFY", "WR_BVH_WIDE_LAT", "WR_TRACE_BVH")


def _context(scene, mode, declined=False):
    trace, env = MODES[mode]
    with pytest.MonkeyPatch.context() as m:  # the knobs are read when the context is created
        for k in KNOBS:
            m.delenv(k, raising=False)
        for k, v in env.items():
            m.setenv(k, v)
        if not (declined and trace == "TRACE_BVH"):
            return native.Context(scene, 0, trace=getattr(native, trace))
        c = native.Context(scene, 0)  # the library default: the KD walk, and asking for the BVH is an error
        with pytest.raises(native.WrError) as e:
            c.set_trace_mode(native.TRACE_BVH)
        assert e.value.code == native.WR_E_SCENE
        return c


@pytest.fixture(scope="module", params=gz.NAMES)
def zoo(request):
    """One family at a time: its scene, a context per mode, the committed
    fixture and the derived rays (made once, on the KD walk's context)."""
    name = request.param
    scene = native.Scene(gz.scene(name))
    z = {"name": name, "scene": scene, "fx": gz.fixture(name),
         "ctx": {mode: _context(scene, mode, name in DECLINED) for mode in MODES}}
    yield z
    for c in z["ctx"].values():
        c.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_fixtures_every_mode(zoo, mode):
    """The reference's answers to the family's corpus (the `far` half included):
    closest hit and occlusion, host calls and device-array calls."""
    fx, c = zoo["fx"], zoo["ctx"][mode]
    rays = fx["rays"]
    r8 = native.rays_from_arrays(rays[:, 0:3], normalize_f32(rays[:, 3:6]))  # Ray's constructor normalises
    o8 = native.rays_from_arrays(rays[:, 0:3], rays[:, 3:6])
    tgt = np.ascontiguousarray(rays[:, 6:9])
    _compare((zoo["name"], mode, "host"), c.trace_closest(r8), c.occluded(o8, tgt), fx)
    f = native.hit_fields(c.trace_closest_t(torch.from_numpy(r8).cuda()).cpu().numpy())
    occ = c.occluded_t(torch.from_numpy(o8).cuda(), torch.from_numpy(tgt).cuda()).cpu().numpy()
    _compare((zoo["name"], mode, "device"), f, occ, fx)


def test_a_damaged_fixture_fails(zoo):
    """One expected primitive changed in a copy of the fixture: _compare sees it."""
    fx = dict(zoo["fx"])
    fx["prim"] = fx["prim"].copy()
    fx["prim"][int(np.nonzero(fx["prim"] >= 0)[0][5])] += 1
    rays = fx["rays"]
    c = zoo["ctx"]["bvh"]
    hits = c.trace_closest(native.rays_from_arrays(rays[:, 0:3], normalize_f32(rays[:, 3:6])))
    occ = c.occluded(native.rays_from_arrays(rays[:, 0:3], rays[:, 3:6]), np.ascontiguousarray(rays[:, 6:9]))
    with pytest.raises(AssertionError):
        _compare("damaged", hits, occ, fx)


@pytest.mark.parametrize("kind", ["spawned", "grazing"])
def test_derived_rays_match_the_kd_walk(zoo, kind):
    """20,000-ray corpora on the family's own surfaces: extension rays EPS off
    them in every direction and shadow rays between hit points (`spawned`), and
    rays along the plane of the surface they leave (`grazing`).  A nearly empty
    scene yields fewer grazing rays than asked for (the floor is most of what a
    random ray meets): at least 2,000 are required, of which a tenth must hit."""
    ref = zoo["ctx"]["kd_walk"]
    n = 20_000
    if kind == "spawned":
        rays, (p, sd, q) = _corpus(ref, n, 4242)
        shadow, targets = native.rays_from_arrays(p, sd), q
    else:
        rays = _plane_grazing_rays(ref, n, 4343)
        shadow = rays
    assert rays.shape[0] >= 2000, (zoo["name"], kind, rays.shape[0])
    a = ref.trace_closest(rays)
    assert (a["prim"] >= 0).sum() >= 0.1 * rays.shape[0], (zoo["name"], kind, int((a["prim"] >= 0).sum()))
    if kind == "grazing":  # targets: the hit point itself, or a point beyond the origin for a miss
        targets = np.where((a["prim"] >= 0)[:, None], a["p"], rays[:, 0:3] + rays[:, 3:6]).astype(np.float32)
    occ = ref.occluded(shadow, targets)
    print(zoo["name"], kind, rays.shape[0], "rays,", int((a["prim"] >= 0).sum()), "hits,", int(occ.sum()), "of",
          occ.size, "occluded")
    for mode in ("bvh", "bvh_wide4", "wave_walk"):
        c = zoo["ctx"][mode]
        b = c.trace_closest(rays)
        ok = _same_hits(a, b)
        assert ok.all(), (zoo["name"], kind, mode, int((~ok).sum()), rays.shape[0], np.nonzero(~ok)[0][:8].tolist())
        for fld in ("p", "n", "inside", "mat_id"):
            assert np.array_equal(a[fld], b[fld]), (zoo["name"], kind, mode, fld)
        bad = np.nonzero(occ != c.occluded(shadow, targets))[0]
        assert bad.size == 0, (zoo["name"], kind, mode, "occluded", int(bad.size), bad[:8].tolist())


@pytest.mark.parametrize("kind", ["bdpt", "pt", "vcm"])
def test_films_match_the_oracle(zoo, kind):
    """32 x 32 renders on the library default against the oracle (itself pinned
    to the reference on these scenes by tests/test_geometry_zoo_host.py): the
    film gates, the ray counts, VCM's query / found / merged counts.  Every
    oracle render traces more than 500 shadow rays, but VCM on `scales`: its
    merge radius follows the 4e5-wide scene, every light vertex is merged at
    every camera vertex and the connections carry less than EPS."""
    name = zoo["name"]
    path = gz.scene(name)
    c = native.Context(zoo["scene"], 0)
    try:
        if kind == "bdpt":
            film, st = c.render_bdpt(W, H, iterations=2, seed=5489, control_length=0)
            ref, rst = _oracle.Scene(path).bdpt(W, H, 2, 5489, mode=1, control_length=0)
        elif kind == "pt":
            film, st = c.render_path(W, H, spp=4, max_depth=7, seed=5489)
            film = film * np.float32(1.0 / 4)  # the oracle (like the reference) scales by 1 / spp
            ref, rst = _oracle.Scene(path).pt(W, H, 4, 7, 5489, mode=1)
        else:
            film, st = c.render_vcm(W, H, iterations=2, seed=3, radius_factor=0.05)
            ref, rst = _oracle.Scene(path).vcm(W, H, 2, 3, mode=1, radius_factor=0.05)
    finally:
        c.close()
    assert rst.closest_rays > 500 and (rst.shadow_rays > 500 or (name, kind) == ("scales", "vcm")), \
        (name, kind, rst.closest_rays, rst.shadow_rays)
    if name in DECLINED:
        assert st.bvh_width == 0, (name, kind, st.bvh_width)
    else:
        assert st.bvh_width in (2, 4), (name, kind, st.bvh_width)  # the verified BVH took the scene
    assert_film_parity(film, ref, case=f"{kind}_geozoo_{name}{W}x{H}")
    assert_ray_counts(st, rst)
    if kind == "vcm":
        assert rst.vm_merged > 100, (name, rst.vm_merged)
        for k in ("vm_queries", "vm_found", "vm_merged"):
            assert getattr(st, k) == getattr(rst, k), (name, k, getattr(st, k), getattr(rst, k))


@pytest.mark.parametrize("tree", ["latency_4wide", "binary"])
def test_every_render_ray_verified(zoo, tree, monkeypatch):
    """One BDPT render with WR_BVH_VERIFY: every ray traced again by the KD walk
    inside the library, (t, primitive) compared bit for bit.  As it comes two
    iterations are latency-bound and search the 4-wide tree; with
    WR_BVH_WIDE_LAT=0 the binary one (test_bvh_tree_of_each_schedule_verified)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("WR_BVH_VERIFY", "1")
    if tree == "binary":
        monkeypatch.setenv("WR_BVH_WIDE_LAT", "0")
    declined = zoo["name"] in DECLINED
    c = native.Context(zoo["scene"], 0, trace=None if declined else native.TRACE_BVH)
    try:
        _, st = c.render_bdpt(W, H, iterations=2, seed=31, control_length=0)
    finally:
        c.close()
    if declined:  # the KD walk rendered it: nothing to verify against
        assert st.bvh_width == 0 and st.verify_mismatches == 0 and st.closest_rays > 0, (zoo["name"], st.bvh_width)
        return
    assert st.verify_rays == st.closest_rays + st.shadow_rays > 0, (zoo["name"], st.verify_rays)
    assert st.verify_mismatches == 0, (zoo["name"], st.verify_mismatches, st.verify_rays)
    assert st.bvh_width == (4 if tree == "latency_4wide" else 2), (zoo["name"], tree, st.bvh_width)
