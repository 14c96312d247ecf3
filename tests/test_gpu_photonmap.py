"""The photon-mapping integrator on the GPU (include/winmad_rt.h wr_photon_*,
wr_render_photon) against its CPU mirror, tests/_script_photonmap.py,
which runs the same definitions over the oracle's primitives.

Gates: counts and shot numbers equal; photon and estimate floats within the
per-ray gate of tests/test_gpu_shading.py, 1e-5 |ref| + 1e-30, no photon or
query exempt; msd and found bit-equal; films by tests/_parity.py's film gate.
The mirror's maps and film are computed once per module.
"""
import ctypes as C

import numpy as np
import pytest

import _oracle
import _scenes
import _script_photonmap as pm
from _parity import assert_film_parity
from winmad_rt import native

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
F = np.float32
SEED = 5489
MAPS = dict(n_caustic=256, n_indirect=2048, max_path_length=5, max_shots=65536)
W, H, SPP, KNN, MSD = 32, 24, 4, 16, 0.1

_state = {}


def ctx(name="spheres"):
    if name not in _state:
        path = _scenes.spheres(W, H) if name == "spheres" else _scenes.cbox(16, 12)
        s = native.Scene(path)
        _state[name] = (s, native.Context(s, 0), path)
    return _state[name][1]


def backend(name="spheres"):
    ctx(name)
    key = "be_" + name
    if key not in _state:
        _state[key] = pm.Backend(_oracle.Scene(_state[name][2]), SEED)
    return _state[key]


def mirror_maps():
    if "maps" not in _state:
        _state["maps"] = pm.build_maps(backend(), MAPS["n_caustic"], MAPS["n_indirect"], MAPS["max_path_length"],
                                       MAPS["max_shots"])
    return _state["maps"]


def gpu_map(**over):
    return ctx().photon_map(seed=SEED, **{**MAPS, **over})


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bad = ~(np.abs(got - want) <= 1e-5 * np.abs(want) + 1e-30)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def hit_records(h):
    """wr_hit records (n, 10) int32 of a mirror hit dict."""
    n = len(h["prim"])
    rec = np.zeros((n, 10), np.int32)
    rec[:, 0] = np.asarray(h["t"], F).view(np.int32)
    rec[:, 1:4] = np.asarray(h["p"], F).view(np.int32)
    rec[:, 4:7] = np.asarray(h["n"], F).view(np.int32)
    rec[:, 7] = h["prim"]
    rec[:, 9] = h["mat_id"]
    return rec


def test_maps_match_the_mirror_on_spheres():
    """n_caustic 256, n_indirect 2048, max_shots 65536 on the spheres scene (glass
    and mirror, unit scale): the mirror fills the caustic map at shot 3909 and the
    indirect map at shot 1753, far below the cap, so both first-N cuts are tested.
    Shots, counts, *_paths and the shot column are equal."""
    want = mirror_maps()
    assert want["shots"] < MAPS["max_shots"] and len(want["caustic"]["pos"]) == MAPS["n_caustic"]
    with gpu_map() as m:
        info = m.info()
        for k in ("shots", "caustic_paths", "indirect_paths"):
            assert info[k] == want[k], (k, info[k], want[k])
        for which, name in ((native.PHOTON_CAUSTIC, "caustic"), (native.PHOTON_INDIRECT, "indirect")):
            got = m.photons(which)
            assert info[name + "_count"] == len(want[name]["pos"]) == len(got["pos"])
            assert np.array_equal(got["shot"], want[name]["shot"]), name
            t = m.photons_t(which)
            for f in ("pos", "wi", "alpha", "shot"):
                assert np.array_equal(t[f].cpu().numpy(), got[f]), (name, f)


def test_map_photons_are_within_the_per_ray_gate_of_the_mirror():
    """pos, wi and alpha of every photon of both maps within 1e-5 |ref| + 1e-30
    per value, no photon exempt.  The mirror traces a bounce ray with the
    direction as sampled, like the reference and the kernels (Backend.trace): with
    the oracle's own trace, which normalises every direction, hit points differ
    in their last bits and components near zero miss this gate (25 of the 20,736
    values did).  Measured on the MI355X with the mirror as it is: all 20,736
    values bit-equal."""
    want = mirror_maps()
    bad = []
    with gpu_map() as m:
        for which, name in ((native.PHOTON_CAUSTIC, "caustic"), (native.PHOTON_INDIRECT, "indirect")):
            got = m.photons(which)
            for f in ("pos", "wi", "alpha"):
                g, w = got[f].astype(np.float64), want[name][f].astype(np.float64)
                err = np.abs(g - w)
                off = ~(err <= 1e-5 * np.abs(w) + 1e-30)
                print(name, f, "values off:", int(off.sum()), "of", off.size, "max abs err", err.max(),
                      "bit-equal:", int((got[f].view(np.uint32) == want[name][f].view(np.uint32)).sum()))
                if off.any():
                    bad.append((name, f, int(off.sum()), np.argwhere(off)[:4].tolist(), g[off][:4], w[off][:4]))
    assert not bad, bad


def _bytes(m):
    out = [repr(sorted((k, v) for k, v in m.info().items() if k not in ("device_bytes", "caustic_cell", "indirect_cell")))]
    for which in (native.PHOTON_CAUSTIC, native.PHOTON_INDIRECT):
        p = m.photons(which)
        out += [p[f].tobytes() for f in ("pos", "wi", "alpha", "shot")]
    return out


def test_maps_are_byte_identical_across_batch_cell_and_builds():
    with gpu_map() as m:
        want = _bytes(m)
    for over in ({"shot_batch": 1000}, {"shot_batch": 4096}, {}, {"cell": 0.05}, {"cell": 0.7}):
        with gpu_map(**over) as m:
            assert _bytes(m) == want, over


def _first_hits(c, be, width, height):
    o, d = be.camera_rays(width, height)
    return o, d, be.trace(o, d)


def test_shot_cap_on_the_cornell_box():
    """No specular material: the caustic map never fills, the build stops at
    max_shots with what it found, and a render with that map equals the mirror's."""
    c, be = ctx("cbox"), backend("cbox")
    want = pm.build_maps(be, 16, 512, 5, 3000, chunk=3000)
    with c.photon_map(n_caustic=16, n_indirect=512, max_shots=3000, seed=SEED) as m:
        info = m.info()
        assert info["shots"] == 3000 and info["caustic_count"] == 0
        assert info["caustic_paths"] == 3000 and info["indirect_paths"] == want["indirect_paths"]
        assert info["indirect_count"] == len(want["indirect"]["pos"])
        film, _ = c.render_photon(m, 16, 12, 1, knn=8, max_sqr_dist=MSD, seed=SEED)
    ref = pm.render(be, want, 16, 12, 1, 8, MSD)[0]
    assert np.isfinite(film).all() and film.any()
    assert_film_parity(film, ref, case="pm_cbox16x12_spp1")


def _estimate_case(m, which, photons, h, wo, k, msd):
    be = backend()
    want = pm.estimate(be, photons, h, wo, k, msd)
    rgb, gm, gf = m.estimate_t(which, dev(hit_records(h)), dev(np.asarray(wo, F)), k=k, max_sqr_dist=msd)
    rgb, gm, gf = rgb.cpu().numpy(), gm.cpu().numpy(), gf.cpu().numpy()
    assert np.array_equal(gf, want[2]), np.argwhere(gf != want[2])[:4].ravel()
    assert np.array_equal(gm.view(np.uint32), want[1].view(np.uint32)), np.argwhere(gm != want[1])[:4].ravel()
    close(rgb, want[0], ("rgb", k, msd))
    return want


def _queries():
    """First hits of the camera rays (every material of the scene, an emitter
    if one is in view), the same hits seen from below the surface (the z-flip
    branch), hits far outside the maps' bounding box, a material-0 hit and a miss."""
    if "queries" in _state:
        return _state["queries"]
    be = backend()
    o, d, h = _first_hits(ctx(), be, W, H)
    k = np.nonzero(h["prim"] >= 0)[0][::3]
    h = be.take(h, k)
    wo = -d[k]
    n = len(k)
    parts = [(h, wo), (h, -wo)]
    far = {f: v[:8].copy() for f, v in h.items()}
    far["p"] = far["p"] + np.array([50.0, -80.0, 120.0], F)
    parts.append((far, wo[:8]))
    odd = {f: v[:2].copy() for f, v in h.items()}
    odd["mat_id"][0] = 0
    odd["prim"][1] = -1
    parts.append((odd, wo[:2]))
    hh = {f: np.concatenate([p[0][f] for p in parts]) for f in h}
    _state["queries"] = (hh, np.concatenate([p[1] for p in parts]).astype(F), n)
    return _state["queries"]


@pytest.mark.parametrize("k,msd", [(1, 0.1), (50, 0.1), (64, 0.1), (50, 1e-6)])
def test_estimate_matches_the_mirror(k, msd):
    h, wo, n = _queries()
    with gpu_map() as m:
        for which, name in ((native.PHOTON_INDIRECT, "indirect"), (native.PHOTON_CAUSTIC, "caustic")):
            photons = m.photons(which)  # the map as the device holds it
            want = _estimate_case(m, which, photons, h, wo, k, msd)
            if name == "indirect":
                assert want[0][:n].any()
                # seen from below, nv = -n and every photon that arrived from above takes the z-flip
                # branch; BSDF::f is black there for the scene's one-sided lobes, on both sides alike
                assert (want[2][n:2 * n] > 0).all()
                assert not want[0][-2:].any() and want[2][-1] == 0  # material 0: black; a miss: nothing found
                assert (want[2][2 * n:2 * n + 8] == min(k, len(photons["pos"]))).all()  # far outside: still k_eff


def test_estimate_on_a_map_smaller_than_k():
    h, wo, _ = _queries()
    with gpu_map(n_caustic=0, n_indirect=20) as m:
        assert m.info()["indirect_count"] == 20 and m.info()["caustic_count"] == 0
        want = _estimate_case(m, native.PHOTON_INDIRECT, m.photons(native.PHOTON_INDIRECT), h, wo, 50, 0.1)
        assert want[2].max() == 20
        none = _estimate_case(m, native.PHOTON_CAUSTIC, m.photons(native.PHOTON_CAUSTIC), h, wo, 50, 0.1)
        assert not none[0].any() and not none[2].any()


def _films():
    if "films" not in _state:
        be = backend()
        _state["films"] = pm.render(be, mirror_maps(), W, H, SPP, KNN, MSD)
        _state["films_a"] = pm.render(be, mirror_maps(), W, H, SPP, KNN, MSD, sample_begin=0, sample_count=1)
    return _state["films"]


@pytest.mark.parametrize("direct_target", [0, 1])
def test_render_matches_the_mirror(direct_target):
    ref = _films()
    assert not np.array_equal(ref[0], ref[1])
    with gpu_map() as m:
        film, _ = ctx().render_photon(m, W, H, SPP, knn=KNN, max_sqr_dist=MSD, direct_target=direct_target, seed=SEED)
        other, _ = ctx().render_photon(m, W, H, SPP, knn=KNN, max_sqr_dist=MSD, direct_target=1 - direct_target,
                                       seed=SEED)
    assert_film_parity(film, ref[direct_target], case=f"pm_spheres{W}x{H}_spp{SPP}_t{direct_target}")
    assert not np.array_equal(film, other)  # the flag does something


def test_sample_shards_sum_to_the_whole_render():
    with gpu_map() as m:
        c = ctx()
        kw = dict(knn=KNN, max_sqr_dist=MSD, seed=SEED)
        full, _ = c.render_photon(m, W, H, SPP, **kw)
        a, _ = c.render_photon(m, W, H, SPP, sample_begin=0, sample_count=1, **kw)
        b, _ = c.render_photon(m, W, H, SPP, sample_begin=1, sample_count=3, **kw)
        dfilm = torch.zeros((H, W, 3), dtype=torch.float32, device=DEV)  # a device film accumulates in place
        c.render_photon(m, W, H, SPP, film_ptr=dfilm.data_ptr(), **kw)
    assert_film_parity(a + b, full, case="pm_shards")
    assert_film_parity(dfilm.cpu().numpy(), full, case="pm_device_film")
    _films()
    assert_film_parity(a, _state["films_a"][0], case="pm_shard_a_mirror")


def test_bad_arguments_are_refused_and_a_good_call_still_works():
    L = native.lib()
    c = ctx()
    h, wo, _ = _queries()
    hits, two = dev(hit_records(h)), dev(wo)
    n = hits.shape[0]
    rgb = torch.zeros((n + 1, 3), dtype=torch.float32, device=DEV)
    P = C.c_void_p
    with gpu_map() as m:
        def call(ctx_h=None, map_h=None, which=1, hp=hits.data_ptr(), wp=two.data_ptr(), nn=n, k=50, msd=0.1,
                 out=rgb.data_ptr()):
            return L.wr_photon_estimate_dev(ctx_h or c.h, map_h or m.h, which, P(hp), P(wp), nn, k, msd, P(out), None,
                                            None)
        assert call(k=0) == native.WR_E_ARG and b"k must be" in L.wr_last_error()
        assert call(k=65) == native.WR_E_ARG
        assert call(out=None) == native.WR_E_ARG and b"null rgb" in L.wr_last_error()
        assert call(out=rgb.data_ptr() + 2) == native.WR_E_ARG and b"aligned" in L.wr_last_error()
        assert call(which=2) == native.WR_E_ARG
        assert call(msd=0.0) == native.WR_E_ARG
        assert call(nn=-1) == native.WR_E_ARG
        host_rgb = np.zeros((n, 3), F)
        assert call(out=host_rgb.ctypes.data) == native.WR_E_ARG and b"not device memory" in L.wr_last_error()
        other = native.Context(_state["spheres"][0], 0)
        try:
            assert call(ctx_h=other.h) == native.WR_E_ARG and b"another context" in L.wr_last_error()
        finally:
            other.close()
        assert call(nn=0) == native.WR_OK
        assert call() == native.WR_OK
        _estimate_case(m, native.PHOTON_INDIRECT, m.photons(native.PHOTON_INDIRECT), h, wo, 50, 0.1)
    for bad in (dict(n_caustic=-1), dict(max_path_length=0), dict(max_shots=0), dict(shot_batch=-1),
                dict(cell=float("nan"))):
        with pytest.raises(native.WrError):
            gpu_map(**bad)
