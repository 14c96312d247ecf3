"""The BVH search with the top of its tree in LDS (multi-wave workgroups,
wr_fast.h search_wg_bytes) returns what it returned without:
the node a lane reads is the same 64 (4-wide: 128) bytes from LDS or from
global memory, and everything after the fetch is the same code.

Rays go in through trace_closest_t, so each launch's ray count is exact.  Per
scene the same rays are traced by
  * the library as it comes (its default top set and workgroup),
  * the top set switched on by its knobs (binary and 4-wide tree, WG waves),
  * WR_BVH_TOP=0 (one wave per workgroup, no copy), and
  * the reference's KD walk (TRACE_REFERENCE),
and (t, prim) must be equal bit for bit among all of them: no tolerance.  The
ray counts walk the launch's edges: one wave and one workgroup more or less
(64 w -+ 1 for w = WG waves), the queue reservation (kRayGrab -+ 1), and one
count above 64 x the search waves a device can hold (32 per CU at most), at
which every resident wave takes its rays from the shared cursor.
"""
import numpy as np
import pytest

import _parity
import _scenes
import _tiny_scenes
from winmad_rt import native

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WG = 4          # waves per search workgroup of the `top` contexts below
RAY_GRAB = 128  # wr_traverse.h kRayGrab
TOP_ON = {"WR_BVH_TOP": "127", "WR_BVH_TOP4": "63", "WR_BVH_TOP_WG": str(WG)}
TOP_OFF = {"WR_BVH_TOP": "0"}

SCENES = {
    "torus": (lambda: _scenes.torus(64, 64), {}),           # binary tree, ntop below the node count
    "torus_wide4": (lambda: _scenes.torus(64, 64), {"WR_BVH_WIDE": "4"}),
    "spheres": (lambda: _scenes.spheres(64, 64), {}),       # the SPH variant
    "tri1": (lambda: _tiny_scenes.tiny(1), {}),             # the whole tree in LDS
    "tri3": (lambda: _tiny_scenes.tiny(3), {}),
}
_ctx = {}


def _device_waves_bound():
    return 32 * torch.cuda.get_device_properties(0).multi_processor_count


def contexts(name, monkeypatch):
    """(default, top on, top off, reference) contexts of a scene, made once."""
    if name not in _ctx:
        maker, env = SCENES[name]
        scene = native.Scene(maker())
        made = []
        for knobs in ({}, TOP_ON, TOP_OFF):
            with monkeypatch.context() as m:
                for k in ("WR_BVH_TOP", "WR_BVH_TOP4", "WR_BVH_TOP_WG"):
                    m.delenv(k, raising=False)
                for k, v in {**env, **knobs}.items():
                    m.setenv(k, v)
                made.append(native.Context(scene, 0, trace=native.TRACE_BVH))
        made.append(native.Context(scene, 0, trace=native.TRACE_REFERENCE))
        _ctx[name] = made
    return _ctx[name]


def counts():
    w = WG
    return sorted({1, 63, 64, 65, 64 * w - 1, 64 * w, 64 * w + 1, RAY_GRAB - 1, RAY_GRAB + 1,
                   64 * _device_waves_bound() + 65})


_rays = {}


def rays_of(name, kind, ref):
    """The ray pool of a scene (device tensor, as many as the largest count)."""
    key = (name, kind)
    if key in _rays:
        return _rays[key]
    nmax = counts()[-1]
    side = int(np.ceil(np.sqrt(nmax)))
    cam = ref.camera_rays_t(side, side)[:nmax].clone()
    if kind == "raster":
        r = cam
    elif kind == "permuted":
        g = torch.Generator(device="cpu").manual_seed(20240611)
        r = cam[torch.randperm(nmax, generator=g).to(cam.device)].contiguous()
    elif kind == "miss":  # from far outside the scene, pointing away from it on every axis
        r = cam.clone()
        r[:, 0:3] += 1.0e5
        r[:, 3:6] = r[:, 3:6].abs()
    elif kind == "tmax":  # a finite tmax: before the hit (even rays) and beyond it (odd rays)
        f = native.hit_fields(ref.trace_closest_t(cam))
        t = f["t"].view(torch.float32) if f["t"].dtype != torch.float32 else f["t"]
        hit = f["prim"] >= 0
        even = (torch.arange(nmax, device=cam.device) % 2) == 0
        r = cam.clone()
        r[:, 7] = torch.where(hit, torch.where(even, 0.5 * t, 1.5 * t), r[:, 7])
    else:
        raise KeyError(kind)
    _rays[key] = r
    return r


def _tp(hits):
    """(t bits, prim) columns of wr_hit records."""
    f = native.hit_fields(hits)
    t = f["t"]
    return (t.view(torch.int32) if t.dtype == torch.float32 else t), f["prim"]


@pytest.mark.parametrize("kind", ["raster", "permuted", "miss", "tmax"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_top_in_lds_same_hits_bit_for_bit(name, kind, monkeypatch):
    default, top, notop, ref = contexts(name, monkeypatch)
    rays = rays_of(name, kind, ref)
    want_t, want_p = _tp(ref.trace_closest_t(rays))  # the reference, once: a prefix's answers are its prefix
    nhit = int((want_p >= 0).sum())
    if kind == "miss":
        assert nhit == 0
    elif kind == "tmax":
        assert 0 < nhit < rays.shape[0] * 0.75  # the even rays end before their hit
    else:
        assert nhit > 0
    for n in counts():
        for label, c in (("default", default), ("top", top), ("top=0", notop)):
            t, p = _tp(c.trace_closest_t(rays[:n]))
            bad = (t != want_t[:n]) | (p != want_p[:n])
            assert not bool(bad.any()), (name, kind, label, n, int(bad.sum()), torch.nonzero(bad)[:8, 0].tolist())


@pytest.mark.parametrize("sched", ["latency_4wide", "binary"])
def test_top_in_lds_bdpt_render_verified(sched, monkeypatch):
    """One BDPT render, every ray verified against the KD walk inside the
    library (WR_BVH_VERIFY): as it comes (two iterations are latency-bound:
    the 4-wide tree) and with WR_BVH_WIDE_LAT=0 (the binary tree).  Same ray
    counts as the WR_BVH_TOP=0 render, film equal up to the order of the float
    atomics (tests/_parity.py)."""
    monkeypatch.setenv("WR_BVH_VERIFY", "1")
    if sched == "binary":
        monkeypatch.setenv("WR_BVH_WIDE_LAT", "0")
    scene = native.Scene(_scenes.torus(64, 64))
    out = []
    for knobs in (TOP_ON, TOP_OFF, {}):
        with monkeypatch.context() as m:
            for k in ("WR_BVH_TOP", "WR_BVH_TOP4", "WR_BVH_TOP_WG"):
                m.delenv(k, raising=False)
            for k, v in knobs.items():
                m.setenv(k, v)
            c = native.Context(scene, 0, trace=native.TRACE_BVH)
        out.append(c.render_bdpt(64, 64, iterations=2, seed=5489))
        c.close()
    (f_top, s_top), (f_off, s_off), (f_def, s_def) = out
    for label, f, s in (("top", f_top, s_top), ("default", f_def, s_def)):
        assert s.bvh_width == (4 if sched == "latency_4wide" else 2), (label, s.bvh_width)
        assert s.verify_rays == s.closest_rays + s.shadow_rays > 0
        assert s.verify_mismatches == 0, (label, s.verify_mismatches, s.verify_rays)
        assert (s.closest_rays, s.shadow_rays) == (s_off.closest_rays, s_off.shadow_rays), label
        _parity.assert_film_parity(f, f_off, case=f"bvh_top_{sched}_{label}_torus64x64_i2")
    assert s_off.verify_mismatches == 0
