"""When a round of the search ends (DESIGN.md 4b "When a round ends").

k_trace_fast's node loop no longer runs until every active lane of the wave
has parked a leaf or finished: it ends once at most K = (active lanes *
kStragglerNum) >> kStragglerShift lanes still lack one, and those lanes keep
descending in the next round, past the leaf phase, the finish test and the
refill (mid-kernel refills and settle batches included).  A wave with fewer
than 16 active lanes gets K = 0, today's rule.  Every answer must stay the
reference mode's, bit for bit, and every render ray verified against the KD
walk, with the film of the resolve over every ray (WR_RESOLVE_LIST=0).

The shapes:
  * n = 1 .. 4,096 corpus rays: a launch this small reserves 64 rays at a time,
    so n <= 15 is one wave that never has 16 active lanes (K = 0: no lane may
    be carried, asserted from the counting build's log), n = 16 / 17 the first
    sizes with K > 0 allowed, 64 / 65 one full wave and a second wave of one ray;
  * a 4,096-ray set whose every 64 consecutive rays -- one wave -- hold 2 long
    rays (the corpus rays of most node visits in the reference walk) among 31
    that point away from the scene box (done after one node) and 31 that go
    down at the floor from all heights (done after 4 to 30 nodes): the wave's
    rounds end with the long rays, and the slowest of the others, mid-descent,
    while 16 or more lanes are still active; carried lanes > 0 is asserted;
  * 200,000 corpus rays over 1,024 search waves (WR_FAST_WAVES_PER_CU=4): about
    195 rays per wave in reservations of 128, so lanes are carried across
    mid-kernel refills and full settle batches;
  * renders with every ray verified (WR_BVH_VERIFY): BDPT 384 x 384 in the
    4-wide and the binary tree, the same in the general queue form
    (WR_QUEUE_SLAB=0), the sphere scene, VCM 192 x 192, each at the default
    number of search waves and at 4 per CU.

The counting build's [wr bvh rounds] line is parsed here (tests/_trace_log.py
reads the launch lines only).  Its figures on the MI355X at the shipped
fraction 1/4 (one run; rounds / node-loop iterations / stepping lanes /
leaf-phase lanes / carried lanes):
  * n = 1: 6 / 36 / 35 / 5 / 0;  n = 15: 8 / 80 / 487 / 56 / 0;
    n = 16: 9 / 79 / 508 / 58 / 4;  n = 17: 9 / 79 / 534 / 61 / 4;
    n = 64: 13 / 82 / 2,098 / 215 / 61;  n = 65: 16 / 121 / 2,137 / 217 / 61;
    n = 4,096: 959 / 6,255 / 136,335 / 14,611 / 4,110;
  * the mixed set: 591 / 3,794 / 27,073 / 3,066 / 1,197 -- 9.2 rounds per wave
    and 2.0 carried lanes per round (the long rays' reference walks visit 406
    to 513 nodes, the corpus median 107);
  * 200,000 rays: 26,232 / 215,411 / 6,743,787 / 726,772 / 232,622 (8.9 carried
    lanes per round), with full settle batches.
At fraction 1/16 the same cases carried 0 / 0 / 1 / 1 / 11 / 11 / 737, 252 and
43,557 lanes.
"""
import ctypes as C
import re

import numpy as np
import pytest

import _oracle
import _scenes
import _trace_log
from test_gpu_bvh import _corpus, _film_close, _same_hits, _unit
from winmad_rt import native

pytestmark = pytest.mark.gpu

_cache = {}

_ROUNDS = re.compile(r"^\[wr bvh rounds\] (\d+) outer rounds, .* (\d+) node-loop iterations \([^)]*\), (\d+) stepping lanes "
                     r"\([^)]*\), (\d+) leaf-phase lanes \([^)]*\), (\d+) lanes carried mid-descent\s*$", re.M)


def _rounds(err):
    """(outer rounds, node-loop iterations, stepping lanes, leaf-phase lanes,
    carried lanes) of the counting launches in the captured stderr text, summed."""
    m = _ROUNDS.findall(err)
    assert m, err
    return tuple(int(v) for v in np.array(m, dtype=np.int64).sum(axis=0))


def _contexts(waves=None):
    """(reference-mode context, BVH-mode context, BVH-mode context of the
    counting kernels with the log on) on the torus; `waves` caps the search's
    resident waves per CU."""
    if waves not in _cache:
        s = native.Scene(_scenes.torus(256, 256))
        env = {} if waves is None else {"WR_FAST_WAVES_PER_CU": waves}
        _cache[waves] = (s, _trace_log.knob_context(s, env, trace=native.TRACE_REFERENCE),
                         _trace_log.knob_context(s, env, trace=native.TRACE_BVH),
                         _trace_log.knob_context(s, dict(env, WR_TRACE_LOG="1"), trace=native.TRACE_BVH))
    return _cache[waves][1:]


def _shuffled_corpus(ref, n0, seed):
    key = ("corpus", n0, seed)
    if key not in _cache:
        rays, _ = _corpus(ref, n0, seed)
        rays = rays[np.random.default_rng(seed).permutation(rays.shape[0])]
        rays.setflags(write=False)
        _cache[key] = rays
    return _cache[key]


def _assert_same_answers(ref, fast, rays, a=None):
    a = ref.trace_closest(rays) if a is None else a
    b = fast.trace_closest(rays)
    ok = _same_hits(a, b)
    assert ok.all(), (int((~ok).sum()), rays.shape[0], np.nonzero(~ok)[0][:8])
    for fld in ("p", "n", "inside", "mat_id"):
        assert np.array_equal(a[fld], b[fld]), fld
    return a


@pytest.mark.parametrize("n", [1, 15, 16, 17, 64, 65, 4096])
def test_small_launches_match_reference_mode(n, capfd):
    """Either side of 16 active lanes, where K leaves 0: the product kernels
    and the counting ones give the reference mode's answers, and a wave of at
    most 15 rays carries no lane over a round's end."""
    ref, fast, logged = _contexts()
    rays = _shuffled_corpus(ref, 4096, 4321)
    assert rays.shape[0] >= 4096
    a = _assert_same_answers(ref, fast, rays[:n])
    capfd.readouterr()
    _assert_same_answers(ref, logged, rays[:n], a)
    rounds, iters, stepped, leafed, carried = _rounds(capfd.readouterr().err)
    print(f"n {n}: {rounds} rounds, {iters} iterations, {stepped} stepping lanes, {leafed} leaf lanes, {carried} carried")
    assert rounds > 0 and iters >= rounds and stepped > 0  # every round runs the node loop at least once
    if n <= 15:
        assert carried == 0, (n, carried)


def _walk_nodes(path, rays):
    """Nodes (inner + leaf) the reference's KD walk visits for each ray: the
    oracle's Scene::intersect, one ray per call."""
    sc = _oracle.Scene(path)
    out = np.zeros(rays.shape[0], np.int64)
    r9 = np.zeros(9, np.float32)
    oi, of = np.zeros(3, np.int32), np.zeros(7, np.float32)
    for k in range(rays.shape[0]):
        r9[0:6] = rays[k, 0:6]
        st = _oracle.Stats()
        sc.L.cr_trace(sc.h, _oracle.fptr(r9), 1, oi.ctypes.data_as(C.POINTER(C.c_int32)), _oracle.fptr(of), None,
                      C.byref(st))
        out[k] = st.inner_visits + st.leaf_visits
    return out


def _mixed_set(ref):
    """4,096 rays, every block of 64 holding 2 long rays among 62 short ones."""
    if "mixed" in _cache:
        return _cache["mixed"]
    rng = np.random.default_rng(77)
    blocks = 64
    pool = np.array(_shuffled_corpus(ref, 4096, 4321)[:4096])
    nodes = _walk_nodes(_scenes.torus(256, 256), pool)
    order = np.argsort(-nodes, kind="stable")
    long_rays = pool[order[:2 * blocks]]
    # the scene's box (the meshes' vertices): x -1131 .. 1008, y -204 (the floor) .. 947, z -1135 .. 989
    n_away = n_down = 31 * blocks
    # short, away: from outside the box, along the line from its middle through the origin
    o = _unit(rng.normal(size=(n_away, 3))) * rng.uniform(4000.0, 9000.0, (n_away, 1)).astype(np.float32)
    away = native.rays_from_arrays(o.astype(np.float32), _unit(o + rng.normal(size=(n_away, 3)).astype(np.float32)))
    # short, down: from every height above the floor, nearly along -y (not an axis ray: those take the KD walk)
    o = np.stack([rng.uniform(-1100.0, 1000.0, n_down), rng.uniform(-190.0, 940.0, n_down),
                  rng.uniform(-1100.0, 980.0, n_down)], axis=1).astype(np.float32)
    d = np.stack([rng.uniform(-0.02, 0.02, n_down), -np.ones(n_down), rng.uniform(-0.02, 0.02, n_down)], axis=1)
    down = native.rays_from_arrays(o, _unit(d.astype(np.float32)))
    # "long" is against the block's other rays: every long ray takes at least four times the nodes of the
    # median ray that goes down at the floor (the rays that point away take one or two)
    short = _walk_nodes(_scenes.torus(256, 256), down)
    print("reference walk, nodes per ray: long rays", int(nodes[order[2 * blocks - 1]]), "..", int(nodes[order[0]]),
          "corpus median", int(np.median(nodes)), "down rays median", int(np.median(short)), "max", int(short.max()))
    assert nodes[order[2 * blocks - 1]] >= 4 * np.median(short)
    rays = np.zeros((64 * blocks, 8), np.float32)
    for b in range(blocks):
        blk = np.concatenate([long_rays[2 * b:2 * b + 2], away[31 * b:31 * b + 31], down[31 * b:31 * b + 31]])
        rays[64 * b:64 * b + 64] = blk[rng.permutation(64)]
    rays.setflags(write=False)
    _cache["mixed"] = rays
    return rays


def test_two_long_rays_per_wave_are_carried_and_match_reference_mode(capfd):
    """One wave per 64-ray block: the rounds end with the block's long rays
    mid-descent, over several rounds while 16 or more of the short rays are
    still active (the logged counts are in the module docstring)."""
    ref, fast, logged = _contexts()
    rays = _mixed_set(ref)
    a = _assert_same_answers(ref, fast, rays)
    assert (a["prim"] >= 0).any() and (a["prim"] < 0).sum() >= 31 * 64
    capfd.readouterr()
    _assert_same_answers(ref, logged, rays, a)
    rounds, iters, stepped, leafed, carried = _rounds(capfd.readouterr().err)
    print(f"mixed set: {rounds} rounds, {iters} iterations, {stepped} stepping lanes, {leafed} leaf lanes, {carried} carried")
    assert carried > 0, (rounds, iters, carried)


def test_lanes_carried_across_refills_and_settle_batches_match_reference_mode(capfd):
    """200,000 rays over 1,024 search waves: reservations of 128, so a carried
    lane sits beside lanes that finish, settle in full batches and refill."""
    ref, fast, logged = _contexts(waves=4)
    rays = _shuffled_corpus(ref, 200_000, 99)
    assert rays.shape[0] >= 200_000
    a = _assert_same_answers(ref, fast, rays[:200_000])
    capfd.readouterr()
    _assert_same_answers(ref, logged, rays[:200_000], a)
    err = capfd.readouterr().err
    rounds, iters, stepped, leafed, carried = _rounds(err)
    print(f"200,000 rays: {rounds} rounds, {iters} iterations, {stepped} stepping lanes, {leafed} leaf lanes, {carried} carried")
    full = int(re.search(r"(\d+) full settle batches", err).group(1))
    assert full > 0, err  # mid-kernel settle batches ran
    assert carried > 0, (rounds, iters, carried)  # ... beside lanes left mid-descent


def _render(scene, env, kind, W, H, **kw):
    """One render in a context made with exactly the knobs of `env` set
    (WR_RESOLVE_LIST is not among _trace_log's)."""
    with pytest.MonkeyPatch.context() as m:
        for k in _trace_log.KNOBS + ("WR_RESOLVE_LIST",):
            m.delenv(k, raising=False)
        for k, v in env.items():
            m.setenv(k, str(v))
        c = native.Context(scene, 0)
        try:
            return (c.render_bdpt if kind == "bdpt" else c.render_vcm)(W, H, iterations=2, **kw)
        finally:
            c.close()


RENDERS = {
    "bdpt_4wide": ("torus", "bdpt", 384, {}, 4),
    "bdpt_binary": ("torus", "bdpt", 384, {"WR_BVH_WIDE_LAT": "0"}, 2),
    "bdpt_4wide_general_form": ("torus", "bdpt", 384, {"WR_QUEUE_SLAB": "0"}, 4),
    "bdpt_spheres": ("spheres", "bdpt", 256, {}, None),
    "vcm": ("torus", "vcm", 192, {}, 2),
}


@pytest.mark.parametrize("waves", [None, 4])
@pytest.mark.parametrize("name", list(RENDERS))
def test_renders_verified_and_equal_to_resolve_over_every_ray(name, waves):
    """Every ray of the render traced again by the KD walk inside the library
    (0 mismatches, every ray checked), and the film close to that of the
    render whose resolve reads every ray -- the same rays traced.  With the
    search's waves per CU as a context has them by default (what the benchmark
    runs), and capped at 4 (1,024 search waves: more rays per wave, so more
    refills and full settle batches beside the carried lanes)."""
    occ = {} if waves is None else {"WR_FAST_WAVES_PER_CU": str(waves)}
    scene_name, kind, side, env, width = RENDERS[name]
    key = ("scene", scene_name, side)
    if key not in _cache:
        _cache[key] = native.Scene((_scenes.torus if scene_name == "torus" else _scenes.spheres)(side, side))
    scene = _cache[key]
    kw = dict(seed=21, count_work=True) if kind == "bdpt" else dict(seed=13)
    fa, sa = _render(scene, dict(env, WR_BVH_VERIFY="1", **occ), kind, side, side, **kw)
    if width is not None:
        assert sa.bvh_width == width, sa.bvh_width
    assert sa.verify_mismatches == 0, (sa.verify_mismatches, sa.verify_rays)
    assert sa.verify_rays == sa.closest_rays + sa.shadow_rays > 0
    fb, sb = _render(scene, dict(env, WR_RESOLVE_LIST="0", **occ), kind, side, side, **kw)
    assert (sa.closest_rays, sa.shadow_rays) == (sb.closest_rays, sb.shadow_rays)
    assert _film_close(fa, fb)
