"""Contexts made under runtime knobs, and the library's WR_TRACE_LOG=1 lines on
stderr, parsed (test infrastructure of test_gpu_hard_forms.py and
test_gpu_vcm_grid.py).

A context made with WR_TRACE_LOG=1 prints one line per traversal launch
(wr_render.hip, trace_launch):

    [wr bvh] N rays  .. us (search .., resolve .., hard ..: T + P pair + S scan rays)  grid G
    [wr trace] Q queues, N rays  .. us  grid G

T, P and S are the launch's tie list, pair list and scan list (what
k_fast_hard found to do), G the search's workgroups / the KD walk's blocks.
Tests read them to show that the path they are about really ran.
"""
import collections
import re

import pytest

from winmad_rt import native

# every knob those files make a context under: all cleared first, so that nothing leaks from case to case
KNOBS = ("WR_TIE_WAVE_MAX", "WR_PAIR_RECORD", "WR_WALK_WAVE", "WR_QUEUE_SLAB", "WR_SCAN_WAVES", "WR_FAST_WAVES_PER_CU",
         "WR_BVH_WIDE_LAT", "WR_BVH_VERIFY", "WR_TRACE_LOG", "WR_RESOLVE_GRID", "WR_TRACE_NO_CUT", "WR_BVH_TOP_WG",
         "WR_BVH_BINS", "WR_BVH_SWEEP", "WR_BVH_CT", "WR_BVH_SERIAL", "WR_TRACE_WAVES_PER_CU", "WR_TRACE_DENSE",
         "WR_SHADE_GRID", "WR_PIPES", "WR_ISSUE_THREADS", "WR_PIECE_MIN", "WR_PIECE_CAP", "WR_VCM_CELL")


def knob_context(scene, env, trace=None):
    """A context on device 0 made with exactly the knobs of `env` set (they
    are read when the context is created); trace as native.Context's."""
    assert set(env) <= set(KNOBS), sorted(set(env) - set(KNOBS))
    with pytest.MonkeyPatch.context() as m:
        for k in KNOBS:
            m.delenv(k, raising=False)
        for k, v in env.items():
            m.setenv(k, str(v))
        return native.Context(scene, 0, trace=trace)


Launch = collections.namedtuple("Launch", "rays ties pairs scans grid")
Walk = collections.namedtuple("Walk", "queues rays grid")

_BVH = re.compile(r"^\[wr bvh\] (\d+) rays .*hard [^:]*: (\d+) \+ (\d+) pair \+ (\d+) scan rays\)\s+grid (\d+)\s*$", re.M)
_WALK = re.compile(r"^\[wr trace\] (\d+) queues, (\d+) rays .* grid (\d+)\s*$", re.M)


def bvh_launches(err):
    """Every BVH-mode launch of the captured stderr text, in order."""
    return [Launch(*map(int, m.groups())) for m in _BVH.finditer(err)]


def walk_launches(err):
    """Every KD-walk launch (the reference mode's) of the captured stderr text."""
    return [Walk(*map(int, m.groups())) for m in _WALK.finditer(err)]


def largest(launches, field):
    return max((getattr(x, field) for x in launches), default=0)
