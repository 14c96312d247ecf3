"""The search's settle batches (DESIGN.md 4b "The resolve list").

With the resolve list on, k_trace_fast does not run the first membership test
(first_cells_crossed) in the lanes that finish a ray: a finished ray with an
unmarked winner leaves (launch index, p1) in a per-wave LDS buffer, and the
wave runs the test over 64 entries at a time, every lane on -- mid-kernel
whenever the buffer holds 64, and once over the remainder at the kernel's end.
The same rays must be listed and the same rays settled: every answer equal to
the reference mode's, every render ray verified against the KD walk, and the
renders equal to those of the resolve over every ray (WR_RESOLVE_LIST=0).

The shapes: WR_FAST_WAVES_PER_CU=4 with a top set gives 1,024 search waves; a
launch of n <= 65,536 rays reserves 64 at a time, so only the end-of-kernel
batch runs (test 1); a larger launch gives each wave several reservations of
128, so batches fire mid-kernel (tests 2 and 3).

Full 64-ray batches the counting build logged (WR_TRACE_LOG, one run each):
  * test 2 (200,000 rays): 2,103 full batches over 22,257 outer rounds (0.85
    of them with a finishing lane, 10.6 lanes per such round);
  * test 3 (384 x 384, 2 iterations): 7,707 full batches in either tree's
    render (1,228,068 rays; 108,365 rounds in the 4-wide render, 109,351 in the
    binary one), and none in the WR_RESOLVE_LIST=0 renders.
"""
import numpy as np
import pytest

import _scenes
from test_gpu_bvh import _corpus, _film_close, _same_hits
from winmad_rt import native

pytestmark = pytest.mark.gpu

_cache = {}


def _pair(monkeypatch=None, waves=None):
    """(reference-mode context, BVH-mode context) on the torus; `waves` caps
    the search's resident waves per CU (read when the context is made)."""
    if waves not in _cache:
        if waves is not None:
            monkeypatch.setenv("WR_FAST_WAVES_PER_CU", str(waves))
        s = native.Scene(_scenes.torus(256, 256))
        _cache[waves] = (s, native.Context(s, 0, trace=native.TRACE_REFERENCE),
                         native.Context(s, 0, trace=native.TRACE_BVH))
    return _cache[waves][1], _cache[waves][2]


def _shuffled_corpus(ref, n0, seed):
    """test_gpu_bvh's corpus (first rays, extension rays, shadow rays), mixed,
    so that any leading slice of it holds rays of every kind."""
    key = ("corpus", n0, seed)
    if key not in _cache:
        rays, _ = _corpus(ref, n0, seed)
        _cache[key] = rays[np.random.default_rng(seed).permutation(rays.shape[0])]
    return _cache[key]


def _assert_same_answers(ref, fast, rays):
    a = ref.trace_closest(rays)
    b = fast.trace_closest(rays)
    ok = _same_hits(a, b)
    assert ok.all(), (int((~ok).sum()), rays.shape[0], np.nonzero(~ok)[0][:8])
    for fld in ("p", "n", "inside", "mat_id"):
        assert np.array_equal(a[fld], b[fld]), fld
    return a


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 4096])
def test_end_of_kernel_batches_match_reference_mode(n):
    """A launch this small gives each wave one reservation of 64: no buffer
    reaches 64 entries and only the partial batch at the kernel's end runs
    (for n = 1 .. 129 over one to three waves, some with a single entry)."""
    ref, fast = _pair()
    rays = _shuffled_corpus(ref, 4096, 4321)
    assert rays.shape[0] >= 4096
    a = _assert_same_answers(ref, fast, rays[:n])
    if n == 4096:
        assert (a["prim"] >= 0).any() and (a["prim"] < 0).any()  # hits to settle, and misses


def test_mid_kernel_batches_match_reference_mode(monkeypatch):
    """200,000 rays over 1,024 search waves: about 195 rays per wave in
    reservations of 128, so the buffers pass 64 entries and full batches run
    between the rounds, the tail of each buffer moving down behind them."""
    ref, fast = _pair(monkeypatch, waves=4)
    rays = _shuffled_corpus(ref, 200_000, 99)
    assert rays.shape[0] >= 200_000
    _assert_same_answers(ref, fast, rays[:200_000])


def _render(monkeypatch, env, kind, W, H, **kw):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = native.Context(native.Scene(_scenes.torus(W, H)), 0)
    out = (c.render_bdpt if kind == "bdpt" else c.render_vcm)(W, H, iterations=2, **kw)
    c.close()
    for k in env:
        monkeypatch.delenv(k)
    return out


@pytest.mark.parametrize("width", [4, 2])
def test_bdpt_render_verified_and_equal_to_resolve_over_every_ray(width, monkeypatch):
    """Torus BDPT 384 x 384, 2 iterations, 1,024 search waves (the first
    overlapped launch holds 295 K rays: mid-kernel batches).  As is the render
    takes the 4-wide tree; WR_BVH_WIDE_LAT=0 keeps the binary one.  Every ray
    is verified against the KD walk, and the render with the resolve over
    every ray traces the same rays to the same film, with the same replay
    steps and fallback rays (the two counters repeated from run to run on the
    parent commit, three runs: 191,282 replay steps and 2 fallback rays, list
    on and off, in either tree's render)."""
    env = {"WR_FAST_WAVES_PER_CU": "4"}
    if width == 2:
        env["WR_BVH_WIDE_LAT"] = "0"
    fa, sa = _render(monkeypatch, dict(env, WR_BVH_VERIFY="1"), "bdpt", 384, 384, seed=21, count_work=True)
    assert sa.bvh_width == width, sa.bvh_width
    assert sa.verify_mismatches == 0, (sa.verify_mismatches, sa.verify_rays)
    assert sa.verify_rays == sa.closest_rays + sa.shadow_rays > 0
    fb, sb = _render(monkeypatch, dict(env, WR_RESOLVE_LIST="0"), "bdpt", 384, 384, seed=21, count_work=True)
    assert sb.bvh_width == width
    assert (sa.closest_rays, sa.shadow_rays) == (sb.closest_rays, sb.shadow_rays)
    assert _film_close(fa, fb)
    print(f"kd_replay_steps {sa.kd_replay_steps} / {sb.kd_replay_steps}, fallback_rays {sa.fallback_rays} / {sb.fallback_rays}")
    assert (sa.kd_replay_steps, sa.fallback_rays) == (sb.kd_replay_steps, sb.fallback_rays)


def test_vcm_render_equal_to_resolve_over_every_ray(monkeypatch):
    """VCM shares the search: torus 192 x 192, 2 iterations, list on against
    list off -- the same rays, the same merges, the film close."""
    fa, sa = _render(monkeypatch, {}, "vcm", 192, 192, seed=13)
    fb, sb = _render(monkeypatch, {"WR_RESOLVE_LIST": "0"}, "vcm", 192, 192, seed=13)
    assert (sa.closest_rays, sa.shadow_rays) == (sb.closest_rays, sb.shadow_rays)
    assert sa.vm_merged == sb.vm_merged
    assert _film_close(fa, fb)
