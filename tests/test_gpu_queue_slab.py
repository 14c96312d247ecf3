"""The slab form of the BDPT traversal launches.

A BDPT pipeline's ray arrays -- o, d, t, prim of every buffer set's shadow /
aux queue and extension queue -- are segments of one slab per parity, and the
search, the resolve and the hard kernels address a ray by its slab entry:
launch index + a per-queue shift held in scalar registers.  WR_QUEUE_SLAB=0
keeps the general form (per-queue pointers selected per lane) over the same
buffers.  Both must trace the same rays to the same answers:

  * equal closest / shadow ray counts,
  * films inside the gates of tests/_parity.py against each other,
  * every ray of the slab form verified against the KD walk (WR_BVH_VERIFY,
    run with count_work: the counting instantiations).

Shapes: the torus at 40 x 24 is 960 paths, a shadow / aux segment of 1,920
entries and an extension segment of 1,920; the queues hold a few hundred rays,
so a wave's 64 launch indices straddle two or three segments with gaps of
unused entries between them, and the late steps have empty queues.  1, 2 and
3 iterations are groups of one buffer set, two, and two then one.  As they
come these renders are latency-bound and search the scene's 4-wide tree;
WR_BVH_WIDE_LAT=0 keeps the binary tree, the benchmark's kernel.
"""
import pytest

import _parity
import _scenes
from winmad_rt import native

pytestmark = pytest.mark.gpu

_scene_cache = {}


def _scene(name, W, H):
    key = (name, W, H)
    if key not in _scene_cache:
        _scene_cache[key] = native.Scene(getattr(_scenes, name)(W, H))
    return _scene_cache[key]


def _render(monkeypatch, env, scene, W, H, iterations, trace=None, **kw):
    """One context made under `env` (the knobs are read at its creation), one render."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        c = native.Context(scene, 0, trace=trace) if trace is not None else native.Context(scene, 0)
        out = c.render_bdpt(W, H, iterations=iterations, seed=77, **kw)
        c.close()
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)
    return out


def _rays(st):
    return (st.closest_rays, st.shadow_rays)


def _check_case(monkeypatch, env, name, W, H, iterations, width=None):
    scene = _scene(name, W, H)
    case = f"slab_{name}{W}x{H}_i{iterations}_" + "_".join(f"{k}={v}" for k, v in sorted(env.items()))
    fs, ss = _render(monkeypatch, env, scene, W, H, iterations)
    fg, sg = _render(monkeypatch, dict(env, WR_QUEUE_SLAB="0"), scene, W, H, iterations)
    fv, sv = _render(monkeypatch, dict(env, WR_BVH_VERIFY="1"), scene, W, H, iterations, count_work=1)
    print(f"{case}: rays slab {_rays(ss)} general {_rays(sg)} verified {sv.verify_rays} "
          f"mismatches {sv.verify_mismatches} width {ss.bvh_width}")
    assert sum(_rays(ss)) > 0
    assert _rays(ss) == _rays(sg) == _rays(sv)
    if width is not None:
        assert ss.bvh_width == sg.bvh_width == sv.bvh_width == width
    _parity.assert_film_parity(fs, fg, case=case)
    _parity.assert_film_parity(fv, fg, case=case + "_verify")
    assert sv.verify_mismatches == 0, (sv.verify_mismatches, sv.verify_rays)
    assert sv.verify_rays == sv.closest_rays + sv.shadow_rays


@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_torus_groups_of_one_two_and_two_then_one(iterations, monkeypatch):
    _check_case(monkeypatch, {}, "torus", 40, 24, iterations)


@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_torus_binary_tree(iterations, monkeypatch):
    """The benchmark's search kernel (the binary tree with the resolve list)."""
    _check_case(monkeypatch, {"WR_BVH_WIDE_LAT": "0"}, "torus", 40, 24, iterations, width=2)


def test_sequential_schedule(monkeypatch):
    """WR_BDPT_OVERLAP=0: extension queues alone in the light pass, then the
    sets' shadow / aux queues followed by their extension queues."""
    _check_case(monkeypatch, {"WR_BDPT_OVERLAP": "0"}, "torus", 40, 24, 2)


def test_sphere_scene(monkeypatch):
    """SPH: the search's sphere instantiation (no resolve list)."""
    _check_case(monkeypatch, {}, "spheres", 32, 32, 2)


def test_four_wide_tree(monkeypatch):
    _check_case(monkeypatch, {"WR_BVH_WIDE": "4"}, "torus", 40, 24, 2, width=4)


def test_shadow_segments_smaller_than_extension_segments(monkeypatch):
    """WR_BDPT_POOL_SCALE=0.05: shadow / aux segments of 704 entries (the
    pools' floor) beside extension segments of 1,920; a step whose queue
    passes its segment is redone with pieces that fit (the clamp)."""
    _check_case(monkeypatch, {"WR_BDPT_POOL_SCALE": "0.05"}, "torus", 40, 24, 2)


def test_reference_walk_on_the_slab_buffers(monkeypatch):
    """TRACE_REFERENCE (k_trace) reads the same segments through the queues'
    general description (plane stride = the slab's entries, count clamped to
    the segment): the same rays and film as BVH mode in slab form."""
    scene = _scene("torus", 40, 24)
    fs, ss = _render(monkeypatch, {}, scene, 40, 24, 2)
    fr, sr = _render(monkeypatch, {}, scene, 40, 24, 2, trace=native.TRACE_REFERENCE)
    print(f"rays slab {_rays(ss)} reference {_rays(sr)}")
    assert _rays(ss) == _rays(sr) and sum(_rays(ss)) > 0
    _parity.assert_film_parity(fs, fr, case="slab_torus40x24_i2_vs_reference")
