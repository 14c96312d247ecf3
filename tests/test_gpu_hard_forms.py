"""The hard-ray kernel's other forms, and the "same answers" knobs of
INTEGRATION.md ("Runtime configuration") that reach them.

k_fast_hard settles what the search and the resolve leave over: the tie list
(near-ties, and rays sent straight to the KD walk), the pair list and the scan
list.  A pipeline launch resolves the tie list one ray per wave while it holds
at most WR_TIE_WAVE_MAX (4,096) rays, and one ray per lane above that -- which
no film of the suite reaches, so the lane form's hand-back (kTieDeferred,
hand_walk), the whole wave's replay of the rays handed back (__ballot / __shfl,
the 64-bit pointer shuffles) and its kWalkEntry entries ran through the pair
list only.  The knobs below put every launch there:

  A. pipeline renders (BDPT, VCM) of the tie-heavy zoo families and the torus
     with WR_TIE_WAVE_MAX=0 (the lane form), without the pair record (near-ties
     on the tie list), with the serial KD walk (WR_WALK_WAVE=0), in the general
     queue form (WR_QUEUE_SLAB=0) and with one scan wave (WR_SCAN_WAVES=1: one
     wave settles every scan ray of a launch in turn), on the 4-wide and on the
     binary tree: the oracle's film, ray counts and merges, and every ray
     verified against the KD walk inside the library (WR_BVH_VERIFY);
  B. the zoo's committed corpora, bit for bit, through the host and the
     device-array calls of contexts made under each remaining traversal knob;
     and a 20,000-ray launch whose tie list is longer than the API form's 2,048
     waves (the wave form's second round);
  D. BDPT torus 384 x 256 and PT cbox 96 x 64 under the grid, cut, pipeline
     and issue-thread knobs.

Every configuration of A renders twice: in a context with WR_TRACE_LOG=1,
whose lines (tests/_trace_log.py) show what the launches held, and in one
without it (the log synchronises after every launch) that verifies every ray.

Counts read from the log on the MI355X (one run; the same on either tree).
Largest tie list T and scan list S of one launch, BDPT / VCM:
  * duplicates 64 x 64: T 772 / 457 (and 410 on the pair list) with the pair
    record, 772 / 867 without it (cases 2, 4); S 0;
  * crowd 64 x 64: T 462, S 0;
  * fan: T 43, S 18 at 64 x 64; case 2 at 128 x 128: T 224, S 82;
  * torus: T 31 / 14, S 14 / 8 at 64 x 64 (case 5: 31 scan rays over the BDPT
    render's launches, 14 in one, all settled by the one scan wave); case 2 at
    128 x 128: T 126 / 73, S 44 / 24;
  so every scene ran the lane form on more than one wave (T > 64), `fan` and
  the torus in case 2's larger film only.
  * case 3 with count_work: fallback_rays 634 on crowd, 0 on duplicates and fan;
  * duplicates 256 x 256 without the pair record: T 12,132 in one launch (of
    549,814 rays in 11 launches) -- 190 waves of the lane form, but short of
    the 16,384 that would give a wave of it a second round: that round stays
    unreached by the suite (it takes T > 64 * min(256, ceil(max_rays / 64)),
    which no launch of fewer than 16,384 rays can give either);
  * the API path on duplicates: the 36,456 spawned rays leave T 5,475 (and 952
    pairs), their 8,228 shadow rays T 4,698: two to three rounds of the wave
    form's 2,048 waves.
"""
import numpy as np
import pytest

import _geometry_zoo as gz
import _oracle
import _scenes
import _trace_log
from _parity import assert_film_parity, assert_ray_counts, assert_vcm_parity
from test_gpu import normalize_f32
from test_gpu_bvh import _corpus, _same_hits
from winmad_rt import native

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

_context = _trace_log.knob_context


# ---------------------------------------------------------------- A: pipeline renders through the lane forms

CASES = {
    1: {"WR_TIE_WAVE_MAX": "0"},
    2: {"WR_TIE_WAVE_MAX": "0", "WR_PAIR_RECORD": "0"},
    3: {"WR_TIE_WAVE_MAX": "0", "WR_WALK_WAVE": "0"},
    4: {"WR_TIE_WAVE_MAX": "0", "WR_PAIR_RECORD": "0", "WR_QUEUE_SLAB": "0"},  # the general-form listed_ray
    5: {"WR_SCAN_WAVES": "1"},
    6: {"WR_SCAN_WAVES": "1", "WR_TIE_WAVE_MAX": "0", "WR_WALK_WAVE": "0", "WR_FAST_WAVES_PER_CU": "1"},
}
# (the tree of the BDPT renders: two iterations are latency-bound and search the 4-wide tree unless
# WR_BVH_WIDE_LAT=0; VCM searches the binary tree of these scenes either way)
TREES = {"latency_4wide": ({}, 4), "binary": ({"WR_BVH_WIDE_LAT": "0"}, 2)}
ZOO = ("duplicates", "crowd", "fan")
NAMES = ZOO + ("torus",)
VCM_NAMES = ("duplicates", "torus")
# the film of a (scene, case): 64 x 64 unless that does not reach the case's condition on the GPU
# (at 64 x 64 `fan` lists at most 43 and the torus at most 31 ties in one launch)
FILM = {("fan", 2): 128, ("torus", 2): 128}

_scene_cache = {}
_oracle_cache = {}
_logged = {}


def _side(name, case):
    return FILM.get((name, case), 64)


def _scene(name, side):
    """(path, native.Scene) of a scene at a film size: built once per module."""
    key = (name, side)
    if key not in _scene_cache:
        path = _scenes.torus(side, side) if name == "torus" else gz.scene(name, side, side)
        _scene_cache[key] = (path, native.Scene(path))
    return _scene_cache[key]


def _oracle_film(name, side, kind):
    key = (name, side, kind)
    if key not in _oracle_cache:
        o = _oracle.Scene(_scene(name, side)[0])
        if kind == "bdpt":
            film, st = o.bdpt(side, side, 2, 5489, mode=1, control_length=0)
        else:
            film, st = o.vcm(side, side, 2, 3, mode=1, radius_factor=0.05)
        film.setflags(write=False)
        _oracle_cache[key] = (film, st)
    return _oracle_cache[key]


def _render(c, side, kind, **kw):
    if kind == "bdpt":
        return c.render_bdpt(side, side, iterations=2, seed=5489, control_length=0, **kw)
    return c.render_vcm(side, side, iterations=2, seed=3, radius_factor=0.05, **kw)


def _kinds(name):
    return ("bdpt", "vcm") if name in VCM_NAMES else ("bdpt",)


def _check(film, st, name, side, kind, label):
    ref, rst = _oracle_film(name, side, kind)
    # (VCM at 128 x 128 traces no shadow ray, in the oracle as on the GPU: with 16,384 light paths and this merge
    # radius every connection carries less than EPS and is dropped before its visibility test)
    assert rst.closest_rays > 500 and (kind == "vcm" or rst.shadow_rays > 500), (label, rst.closest_rays, rst.shadow_rays)
    if kind == "bdpt":
        assert_film_parity(film, ref, case=f"bdpt_hard_forms_{label}")
    else:
        assert_vcm_parity(film, ref, case=f"vcm_hard_forms_{label}")
        for k in ("vm_queries", "vm_found", "vm_merged"):
            assert getattr(st, k) == getattr(rst, k), (label, k, getattr(st, k), getattr(rst, k))
    assert_ray_counts(st, rst)


def _logged_renders(capfd, name, case, tree):
    """The case's renders in a context that logs its launches: {kind: (film,
    stats, launches)}.  Rendered once, whichever test asks first."""
    key = (name, case, tree)
    if key not in _logged:
        side = _side(name, case)
        c = _context(_scene(name, side)[1], dict(CASES[case], **TREES[tree][0], WR_TRACE_LOG="1"), trace=native.TRACE_BVH)
        out = {}
        try:
            for kind in _kinds(name):
                capfd.readouterr()
                film, st = _render(c, side, kind)
                out[kind] = (film, st, _trace_log.bvh_launches(capfd.readouterr().err))
        finally:
            c.close()
        _logged[key] = out
    return _logged[key]


@pytest.mark.parametrize("tree", list(TREES))
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", NAMES)
def test_pipeline_renders_through_the_lane_forms(name, case, tree, capfd):
    side = _side(name, case)
    label = f"{name}{side}_case{case}_{tree}"
    width = TREES[tree][1]
    for kind, (film, st, launches) in _logged_renders(capfd, name, case, tree).items():
        assert launches, (label, kind, "no [wr bvh] line: the log was not read")
        print(label, kind, "launches", len(launches), "rays", sum(x.rays for x in launches), "of",
              st.closest_rays + st.shadow_rays, "largest T", _trace_log.largest(launches, "ties"), "P",
              _trace_log.largest(launches, "pairs"), "S", _trace_log.largest(launches, "scans"), "sum T",
              sum(x.ties for x in launches), "sum S", sum(x.scans for x in launches))
        assert st.bvh_width == (width if kind == "bdpt" else 2), (label, kind, st.bvh_width)
        _check(film, st, name, side, kind, label + "_logged")
    # the same configuration without the log, every ray traced again by the KD walk inside the library
    c = _context(_scene(name, side)[1], dict(CASES[case], **TREES[tree][0], WR_BVH_VERIFY="1"), trace=native.TRACE_BVH)
    try:
        for kind in _kinds(name):
            film, st = _render(c, side, kind)
            _check(film, st, name, side, kind, label)
            assert st.bvh_width == (width if kind == "bdpt" else 2), (label, kind, st.bvh_width)
            assert st.verify_mismatches == 0, (label, kind, st.verify_mismatches, st.verify_rays)
            assert st.verify_rays == st.closest_rays + st.shadow_rays > 0, (label, kind, st.verify_rays)
    finally:
        c.close()


@pytest.mark.parametrize("name", NAMES)
def test_the_lane_form_ran_on_more_than_one_wave(name, capfd):
    """At least one of cases 1-4 shows a launch whose tie list holds more than
    64 rays: with WR_TIE_WAVE_MAX=0 that is more than one wave of the lane form."""
    seen = {}
    for case in (1, 2, 3, 4):
        for tree in TREES:
            runs = _logged_renders(capfd, name, case, tree)
            seen[(case, tree)] = max(_trace_log.largest(r[2], "ties") for r in runs.values())
    print(name, "largest tie list of one launch:", seen)
    assert max(seen.values()) > 64, (name, seen)


def test_one_scan_wave_settles_several_rays_in_turn(capfd):
    """Torus, WR_SCAN_WAVES=1: a launch with two or more scan rays, which the
    one scan wave settles one after the other."""
    seen = {}
    for tree in TREES:
        runs = _logged_renders(capfd, "torus", 5, tree)
        seen[tree] = max(_trace_log.largest(r[2], "scans") for r in runs.values())
    print("torus largest scan list of one launch:", seen)
    assert max(seen.values()) >= 2, seen


def test_the_serial_walk_is_the_fallback_without_the_wave_walk():
    """Case 3 with count_work (the counting kernels): the oracle's films, and
    fallback_rays > 0 on at least one zoo family -- settle_ray's serial kd_walk
    really ran, in lanes (the lane form never hands a walk back with
    WR_WALK_WAVE=0) and in whole waves (the scan list)."""
    fallback = {}
    for name in ZOO:
        side = _side(name, 3)
        c = _context(_scene(name, side)[1], CASES[3], trace=native.TRACE_BVH)
        try:
            film, st = _render(c, side, "bdpt", count_work=True)
        finally:
            c.close()
        _check(film, st, name, side, "bdpt", f"{name}{side}_case3_counted")
        fallback[name] = st.fallback_rays
    print("fallback_rays with WR_WALK_WAVE=0:", fallback)
    assert max(fallback.values()) > 0, fallback


# longer than the default WR_TIE_WAVE_MAX: a tie list that production settles in the lane form too.  (A second round
# of the lane loop would take more than 16,384; the film gives 12,132.)
LONG_TIE_LIST = 4096


def test_the_lane_loop_on_a_long_tie_list(capfd):
    """`duplicates` at 256 x 256 without the pair record: the longest tie
    lists a film of the suite gives the lane form, 12,132 rays in one launch.
    A second round of its loop needs more than 64 * lgrid = 16,384: not
    reached, so this is a parity case over 190 waves of the form."""
    side = 256
    path, scene = _scene("duplicates", side)
    c = _context(scene, {"WR_TIE_WAVE_MAX": "0", "WR_PAIR_RECORD": "0", "WR_TRACE_LOG": "1"}, trace=native.TRACE_BVH)
    try:
        capfd.readouterr()
        film, st = _render(c, side, "bdpt")
        launches = _trace_log.bvh_launches(capfd.readouterr().err)
    finally:
        c.close()
    ref, rst = _oracle.Scene(path).bdpt(side, side, 2, 5489, mode=1, control_length=0)
    assert_film_parity(film, ref, case="bdpt_hard_forms_duplicates256_long_tie_list")
    assert_ray_counts(st, rst)
    big = _trace_log.largest(launches, "ties")
    print("duplicates 256 x 256: largest tie list of one launch", big, "of", len(launches), "launches")
    assert big > LONG_TIE_LIST, (big, LONG_TIE_LIST)


# ---------------------------------------------------------------- B: the API forms, corpus answers bit for bit

API_SETTINGS = [
    ("TRACE_BVH", {"WR_WALK_WAVE": "0"}),
    ("TRACE_BVH", {"WR_SCAN_WAVES": "1"}),
    ("TRACE_BVH", {"WR_FAST_WAVES_PER_CU": "1"}),
    ("TRACE_BVH", {"WR_RESOLVE_GRID": "1"}),
    ("TRACE_BVH", {"WR_TRACE_NO_CUT": "1"}),
    ("TRACE_BVH", {"WR_PAIR_RECORD": "0"}),
    ("TRACE_BVH", {"WR_BVH_TOP_WG": "1"}),
    ("TRACE_BVH", {"WR_BVH_TOP_WG": "16"}),
    # the build's measurement knobs: another tree (4 SAH bins, exact sweeps below 8 triangles, a dearer node), built
    # without helper threads
    ("TRACE_BVH", {"WR_BVH_BINS": "4", "WR_BVH_SWEEP": "8", "WR_BVH_CT": "2", "WR_BVH_SERIAL": "1"}),
    ("TRACE_REFERENCE", {"WR_TRACE_WAVES_PER_CU": "1"}),
    ("TRACE_REFERENCE", {"WR_TRACE_WAVES_PER_CU": "1", "WR_TRACE_DENSE": "1"}),
    ("TRACE_REFERENCE", {"WR_TRACE_NO_CUT": "1"}),
]
DECLINED = ("degenerate",)  # build_fast declines the sliver scene: its contexts keep the KD walk (test_gpu_geometry_zoo.py)


def _setting_id(s):
    return (s[0] or "TRACE_default")[6:].lower() + "-" + "-".join(f"{k[3:]}={v}" for k, v in s[1].items())


@pytest.fixture(scope="module", params=gz.NAMES)
def family(request):
    name = request.param
    return name, native.Scene(gz.scene(name)), gz.fixture(name)


@pytest.mark.parametrize("setting", API_SETTINGS, ids=_setting_id)
def test_corpus_answers_under_every_setting(family, setting):
    """The reference's answers to the family's committed corpus, closest hit
    and occlusion, through the host calls and the device-array calls."""
    name, scene, fx = family
    trace, env = setting
    if name in DECLINED and trace == "TRACE_BVH":
        c = _context(scene, env)  # the library default: the KD walk, and asking for the BVH is an error
        with pytest.raises(native.WrError) as e:
            c.set_trace_mode(native.TRACE_BVH)
        assert e.value.code == native.WR_E_SCENE
    else:
        c = _context(scene, env, trace=getattr(native, trace))
    try:
        rays = fx["rays"]
        r8 = native.rays_from_arrays(rays[:, 0:3], normalize_f32(rays[:, 3:6]))  # Ray's constructor normalises
        o8 = native.rays_from_arrays(rays[:, 0:3], rays[:, 3:6])
        tgt = np.ascontiguousarray(rays[:, 6:9])
        gz.compare((name, _setting_id(setting), "host"), c.trace_closest(r8), c.occluded(o8, tgt), fx)
        f = native.hit_fields(c.trace_closest_t(torch.from_numpy(r8).cuda()).cpu().numpy())
        occ = c.occluded_t(torch.from_numpy(o8).cuda(), torch.from_numpy(tgt).cuda()).cpu().numpy()
        gz.compare((name, _setting_id(setting), "device"), f, occ, fx)
    finally:
        c.close()


API_TIE_SCENE = "duplicates"


def test_the_wave_form_takes_a_second_round_on_the_api_path(capfd):
    """The API calls' hard launch is one tie per wave on min(2048, n) waves.
    The 20,000 spawned rays of test_gpu_geometry_zoo's derived corpus leave
    more than 2,048 ties in one launch: every wave takes a second listed ray,
    with the LDS stack columns, the wave walk's region and the counters as the
    first left them.  Answers as the KD walk's, bit for bit."""
    scene = native.Scene(gz.scene(API_TIE_SCENE))
    ref = _context(scene, {}, trace=native.TRACE_REFERENCE)
    fast = _context(scene, {"WR_TRACE_LOG": "1"}, trace=native.TRACE_BVH)
    try:
        rays, (p, sd, q) = _corpus(ref, 20_000, 4242)
        a = ref.trace_closest(rays)
        capfd.readouterr()
        b = fast.trace_closest(rays)
        launches = _trace_log.bvh_launches(capfd.readouterr().err)
        ok = _same_hits(a, b)
        assert ok.all(), (int((~ok).sum()), rays.shape[0], np.nonzero(~ok)[0][:8].tolist())
        for fld in ("p", "n", "inside", "mat_id"):
            assert np.array_equal(a[fld], b[fld]), fld
        shadow = native.rays_from_arrays(p, sd)
        occ = fast.occluded(shadow, q)
        launches += _trace_log.bvh_launches(capfd.readouterr().err)
        bad = np.nonzero(ref.occluded(shadow, q) != occ)[0]
        assert bad.size == 0, ("occluded", int(bad.size), bad[:8].tolist())
    finally:
        ref.close()
        fast.close()
    print(API_TIE_SCENE, rays.shape[0], "rays:", [(x.rays, x.ties, x.pairs, x.scans) for x in launches])
    assert _trace_log.largest(launches, "ties") > 2048, launches


# ---------------------------------------------------------------- D: the remaining render knobs

RENDER_SETTINGS = [
    (None, {"WR_SHADE_GRID": "2"}),
    (None, {"WR_SHADE_GRID": "64"}),
    (None, {"WR_RESOLVE_GRID": "1"}),
    (None, {"WR_TRACE_NO_CUT": "1"}),
    # four pipelines that really get pieces: 98,304 paths in pieces of at most 4,096
    (None, {"WR_PIPES": "4", "WR_ISSUE_THREADS": "4", "WR_PIECE_MIN": "64", "WR_PIECE_CAP": "4096"}),
    ("TRACE_REFERENCE", {"WR_TRACE_WAVES_PER_CU": "1"}),
]
_render_refs = {}


def _render_ref(kind):
    """Scenes and oracle films of part D: made once."""
    if kind not in _render_refs:
        if kind == "bdpt":
            path = _scenes.torus(384, 256)
            ref, rst = _oracle.Scene(path).bdpt(384, 256, 2, 5489, mode=1)
        else:
            path = _scenes.cbox(96, 64)
            ref, rst = _oracle.Scene(path).pt(96, 64, 4, 7, 5489, mode=1)
        ref.setflags(write=False)
        _render_refs[kind] = (native.Scene(path), ref, rst)
    return _render_refs[kind]


@pytest.mark.parametrize("kind", ["bdpt", "pt"])
@pytest.mark.parametrize("setting", RENDER_SETTINGS, ids=_setting_id)
def test_renders_under_the_grid_cut_and_pipeline_knobs(setting, kind):
    """BDPT torus 384 x 256, 2 iterations (98,304 paths: the vertex kernels'
    grid-stride loops take a second, partial round on the default 256 blocks)
    and PT cbox 96 x 64, 4 spp, against the oracle: film gates and ray counts."""
    trace, env = setting
    scene, ref, rst = _render_ref(kind)
    c = _context(scene, env, trace=getattr(native, trace) if trace else None)
    try:
        if kind == "bdpt":
            film, st = c.render_bdpt(384, 256, iterations=2, seed=5489)
        else:
            film, st = c.render_path(96, 64, spp=4, max_depth=7, seed=5489)
            film = film * np.float32(1.0 / 4)  # the oracle (like the reference) scales by 1 / spp
    finally:
        c.close()
    label = "_".join(f"{k[3:].lower()}{v}" for k, v in env.items())
    assert_film_parity(film, ref, case=f"{kind}_knobs_{label}")
    assert_ray_counts(st, rst)
    print(kind, label, "pipelines", st.pipelines)
    if "WR_PIPES" in env and kind == "bdpt":
        assert st.pipelines == 4, st.pipelines
