"""The photon-mapping integrator without a GPU: the CPU mirror
tests/_script_photonmap.py against the reference's own estimate(), its closed
forms against the literal loops they replace, and the library's new symbols."""
import json
import os

import numpy as np
import pytest

import _oracle
import _points_ref
import _scenes
import _script_photonmap as pm
from winmad_rt import native

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW = ["wr_photon_map_build", "wr_photon_map_info_get", "wr_photon_map_read", "wr_photon_map_free",
       "wr_photon_estimate_dev", "wr_render_photon"]


def test_symbols_are_exported_and_the_version_stays():
    L = native.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in native.EXPORTS
    assert L.wr_api_version() == 8


def test_null_context_and_null_map_are_refused_before_any_device_call():
    L = native.lib()
    prm = native.WrPhotonMapParams(16, 16, 5, 100, 0, 0.0, 1)
    assert L.wr_photon_map_build(None, prm, None, None) == native.WR_E_ARG
    assert b"null context" in L.wr_last_error()
    assert L.wr_photon_estimate_dev(None, None, 0, None, None, 0, 50, 0.1, None, None, None) == native.WR_E_ARG
    assert L.wr_render_photon(None, None, None, None, 0, None) == native.WR_E_ARG
    assert L.wr_photon_map_info_get(None, None) == native.WR_E_ARG
    L.wr_photon_map_free(None)  # a no-op


def test_mirror_estimate_matches_the_reference_fixture():
    """tests/golden/pm_estimate_spheres.f32: the reference's estimate()
    (photonMap.cpp:164-231) on a KdTree<Photon> of 400 photons, for 48 camera-ray
    hits on the spheres scene, knn 50, maxSqrDis 0.1.  Every term is
    non-negative and the two sums differ only in the order of at most 64 float
    adds (the reference's is its heap's), so the gate is 2 * 64 * 2^-24
    relative, plus 1e-30.  The fixture's rays were chosen so that the 50th and
    51st nearest photon differ in d2: with a tie there the reference's set is
    its heap's choice, ours the lower index."""
    meta = json.load(open(os.path.join(GOLD, "pm_estimate_spheres.json")))
    a = np.fromfile(os.path.join(GOLD, "pm_estimate_spheres.f32"), F)
    nph, nray, knn, msd = int(a[0]), int(a[1]), int(a[2]), a[3]
    assert (nph, nray, knn) == (meta["photons"], meta["rays"], meta["knn"]) and msd == F(meta["max_sqr_dist"])
    ph = a[4:4 + nph * 9].reshape(nph, 9)
    rays = a[4 + nph * 9:4 + nph * 9 + nray * 6].reshape(nray, 6)
    ref = a[4 + nph * 9 + nray * 6:].reshape(nray, 8)
    be = pm.Backend(_oracle.Scene(_scenes.spheres(64, 64)), 5489)
    d = rays[:, 3:6]
    d = (d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]).astype(F)  # Ray's constructor
    h = be.trace(rays[:, 0:3].copy(), d)
    assert (ref[:, 3] == 1).all() and np.array_equal(h["p"], ref[:, 4:7]) and np.array_equal(h["mat_id"], ref[:, 7])
    d2 = np.sort(_points_ref.sqr_dist(h["p"], ph[:, 0:3]), 1)
    assert (d2[:, knn - 1] != d2[:, knn]).all()  # no tie at the k-th distance
    photons = {"pos": ph[:, 0:3].copy(), "wi": ph[:, 3:6].copy(), "alpha": ph[:, 6:9].copy()}
    rgb, got_msd, found = pm.estimate(be, photons, h, -d, knn, msd)
    want = ref[:, 0:3].astype(np.float64)
    assert (found == knn).all() and len(np.unique(got_msd)) > 1 and (want.any(1)).sum() > nray // 2
    assert (np.abs(rgb - want) <= 2 * 64 * 2.0 ** -24 * np.abs(want) + 1e-30).all(), np.abs(rgb - want).max()


@pytest.mark.parametrize("n,k,msd", [(300, 50, 0.1), (300, 50, 1e-6), (300, 1, 0.01), (20, 50, 0.1), (64, 64, 1e-6),
                                     (0, 50, 0.1)])
def test_closed_form_msd_equals_the_doubling_loop(n, k, msd):
    rng = np.random.default_rng(n * 131 + k)
    pts = rng.uniform(-1, 1, (n, 3)).astype(F)
    pts[: n // 4] = (pts[: n // 4] * F(0.01)).astype(F)  # a dense clump: a few doublings for some, many for others
    q = rng.uniform(-1.2, 1.2, (24, 3)).astype(F)
    idx, sqr, cnt = _points_ref.knn(q, pts, k, F(np.inf)) if n else (np.zeros((24, k), np.int32), None, np.zeros(24, int))
    for j in range(len(q)):
        if n == 0:  # an empty map: nothing found, the estimate is black
            rgb, m, f = pm.estimate(None, {"pos": pts, "wi": pts, "alpha": pts},
                                    {"p": q, "prim": np.zeros(24, np.int32)}, q, k, msd)
            assert not rgb.any() and not m.any() and not f.any()
            break
        k_eff = min(k, n)
        assert cnt[j] == k_eff
        want_msd, want_idx = pm.doubling_loop(q[j], pts, k, msd)
        got = pm.closed_form_msd(sqr[j, k_eff - 1:k_eff], msd)[0]
        assert got == want_msd and np.array_equal(idx[j, :k_eff], want_idx), (j, got, want_msd)
    if msd == 1e-6 and n:
        assert np.log2(float(pm.closed_form_msd(sqr[:, min(k, n) - 1], msd).max()) / 1e-6) > 20  # twenty-odd doublings


def test_photon_pass_first_n_equals_the_serial_loop():
    """The mirror's maps (prefix counts over (shot, bounce)-sorted photons) are
    what buildPhotonMap's serial loop keeps of the same shots, and do not
    depend on the chunk the shots are run in."""
    be = pm.Backend(_oracle.Scene(_scenes.spheres(64, 64)), 5489)
    a = pm.build_maps(be, 24, 200, 5, 4096, chunk=256)
    b = pm.build_maps(be, 24, 200, 5, 4096, chunk=1000)
    rec = a["records"]
    s = pm.serial_select(rec, 24, 200, a["shots_run"])
    assert (s["shots"], s["caustic_paths"], s["indirect_paths"]) == (a["shots"], a["caustic_paths"], a["indirect_paths"])
    assert a["shots"] < 4096 and len(s["caustic"]) == 24 and len(s["indirect"]) == 200
    for name in ("caustic", "indirect"):
        for f in ("pos", "wi", "alpha", "shot"):
            assert np.array_equal(a[name][f], rec[f][s[name]]), (name, f)
            assert np.array_equal(a[name][f], b[name][f]), (name, f)
    assert (rec["nint"] >= 2).all() and (rec["nint"] <= 6).all()
    assert (np.diff(rec["shot"]) >= 0).all()
    # the cap: a scene without caustics stops at max_shots with what it found
    bc = pm.Backend(_oracle.Scene(_scenes.cbox(16, 12)), 5489)
    c = pm.build_maps(bc, 16, 100000, 5, 300, chunk=128)
    assert c["shots"] == 300 and len(c["caustic"]["pos"]) == 0 and c["caustic_paths"] == 300 == c["indirect_paths"]
    sc = pm.serial_select(c["records"], 16, 100000, 300)
    assert sc["shots"] == 300 and len(sc["indirect"]) == len(c["indirect"]["pos"])
