"""The VCM merge grid away from the 441 cells of the other VCM tests.

A grid row (cy, cz) is a run of kRowW = 1,024 buckets addressed by cx & 1023
(wr_vcm.h, vcm_row / vcm_bucket), so a query's cells [x0, x1] of a row are one
bucket range -- or two, where cx wraps inside the query (`a > bx` in
vcm_merge) -- and a bucket is shared by the cells cx, cx + 1024, ...: the
`vx < x0 || vx > x1` filter keeps a vertex of another lap out (one that is
1,024 cells off also fails the distance test before it: a scratch build
without the filter passed these cases, so they pin the ranges and the shared
buckets, not that filter).  All of that only matters once the scene spans more than 1,024 cells on x.  The torus scene
is 2,138.7 units wide with sceneRadius 1,613.1: 441 cells at the reference's
radius (factor 0.003, cell edge of one radius, iteration 0), and no other VCM
test has more.  Production does: the radius shrinks by (it + 1)^-0.125, so the
same scene passes 1,024 cells at about iteration 838, and WR_VCM_CELL=0.25
(1,766 cells at iteration 0) wraps at once.  A wrong answer there is a missed
or a doubled merge.

Every case is compared with the oracle's restatement of vertexcm.cpp (the
reference's KD-tree range search, no grid): the film gates of tests/_parity.py
and equal ray, query, found and merged counts.  The wrapping cases recompute
their cells on x from the scene's bounding box and the radius schedule
(wr_render.hip, wr_render_vcm) and require more than 1,024 in every iteration.

Queries that took the two-range branch, counted once by a scratch build of the
library (a counter in vcm_merge, not committed), and the light vertices those
queries found (film, factor, cell: queries, two-range queries, vertices found
by them), each at iterations 4,000 and 4,001:
  * 256 x 256, 0.003, 1:    113,206 queries, none two-range (a query spans 3
    cells; the case has the shared buckets and the filter, not the branch);
  * 192 x 192, 0.01, 0.25:   63,761 queries, 51 two-range, 25 vertices;
  * 192 x 192, 0.003, 0.25:  63,761 queries, 88 two-range, 30 vertices;
  (256 x 256, 0.01, 0.25 would give 92 and 90: not needed, two cases have 50.)
A scratch build that never reads the second range fails both quarter-cell
wrapping cases, every cell-edge case and the spheres case (cells -1 and 0
wrap too) on their found counts.
"""
import os

import numpy as np
import pytest

import _geometry_zoo as gz
import _oracle
import _scenes
import _trace_log
from _parity import assert_vcm_parity
from winmad_rt import native, scenes

pytestmark = pytest.mark.gpu

ROW_W = 1024  # wr_vcm.h kRowW
_scene_cache = {}


def _scene(maker):
    """(path, native.Scene): built once per module."""
    path = maker()
    if path not in _scene_cache:
        _scene_cache[path] = native.Scene(path)
    return path, _scene_cache[path]


def _context(scene, cell):
    return _trace_log.knob_context(scene, {} if cell is None else {"WR_VCM_CELL": cell})


def _torus_box():
    """Bounding box of the torus scene: the vertices of its four .obj files."""
    v = []
    for f in ("torus_torus.obj", "torus_glass.obj", "torus_floor.obj", "torus_light.obj"):
        with open(os.path.join(scenes.ASSETS, f)) as fh:
            v += [[np.float32(t) for t in ln.split()[1:4]] for ln in fh if ln.startswith("v ")]
    v = np.array(v, np.float32)
    return v.min(axis=0), v.max(axis=0)


def cells_on_x(it, radius_factor, cell, alpha=0.75):
    """Grid cells the torus scene spans on x in iteration `it`: the library's
    float arithmetic (wr_scene.cpp's scene sphere, wr_render_vcm's radius
    schedule, rq = r (1 + 2^-10), cell edge = WR_VCM_CELL x rq)."""
    f = np.float32
    lo, hi = _torus_box()
    d = hi - lo
    scene_radius = f(np.sqrt(f(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])) * f(0.5)
    radius = f(f(radius_factor) * scene_radius) / f(np.power(f(it + 1), f(0.5) * (f(1) - f(alpha))))
    return float(d[0] / (f(cell) * f(radius * f(1.0009765625))))


def _check(film, st, ref, rst, label):
    assert rst.vm_merged > 1000, (label, rst.vm_merged)
    print(label, "queries", st.vm_queries, "found", st.vm_found, "merged", st.vm_merged, "oracle",
          rst.vm_queries, rst.vm_found, rst.vm_merged)
    for k in ("closest_rays", "shadow_rays", "vm_queries", "vm_found", "vm_merged"):
        assert getattr(st, k) == getattr(rst, k), (label, k, getattr(st, k), getattr(rst, k))
    assert_vcm_parity(film, ref, case=f"vcm_grid_{label}")


def test_the_torus_box_is_the_one_the_docstring_counts_with():
    """2,138.7 units on x, 441 cells at the reference's radius: the numbers the
    wrapping cases' arithmetic starts from."""
    lo, hi = _torus_box()
    assert abs(float(hi[0] - lo[0]) - 2138.7) < 0.1, (lo, hi)
    assert 440 < cells_on_x(0, 0.003, 1.0) < 443
    assert 1760 < cells_on_x(0, 0.003, 0.25) < 1770


@pytest.mark.parametrize("side,radius_factor,cell", [
    (256, 0.003, None),   # the reference's radius 4,000 iterations on: about 1,245 cells, one wrap
    (192, 0.01, 0.25),    # about 1,494 cells, a query spans 9 of them: the two-range branch
    (192, 0.003, 0.25),   # about 4,980 cells: four wraps, a bucket shared by five cells of a row
])
def test_wrapped_rows_merge_what_the_reference_merges(side, radius_factor, cell):
    it0, n = 4000, 2
    for it in range(it0, it0 + n):
        cx = cells_on_x(it, radius_factor, 1.0 if cell is None else cell)
        print(f"torus {side} factor {radius_factor} cell {cell} iteration {it}: {cx:.1f} cells on x")
        assert cx > ROW_W, (it, cx)
    path, scene = _scene(lambda: _scenes.torus(side, side))
    c = _context(scene, cell)
    try:
        film, st = c.render_vcm(side, side, iterations=n, seed=5, iter_begin=it0, radius_factor=radius_factor)
    finally:
        c.close()
    ref, rst = _oracle.Scene(path).vcm(side, side, n, 5, mode=1, iter_begin=it0, radius_factor=radius_factor)
    _check(film, st, ref, rst, f"torus{side}_it{it0}_rf{radius_factor}_cell{cell}")


_clamp_ref = {}


@pytest.mark.parametrize("cell", [0.25, 0.5, 1.7, 4, 8])
def test_cell_edges_other_than_one_radius(cell):
    """Torus 64 x 64 at factor 0.05 (26 cells on x at cell 1): cells of a
    quarter and of half a radius give a query 9 and 5 cells per axis, cells of
    1.7, 4 and 8 radii one or two."""
    path, scene = _scene(lambda: _scenes.torus(64, 64))
    if "torus" not in _clamp_ref:
        _clamp_ref["torus"] = _oracle.Scene(path).vcm(64, 64, 2, 11, mode=1, radius_factor=0.05)
    ref, rst = _clamp_ref["torus"]
    c = _context(scene, cell)
    try:
        film, st = c.render_vcm(64, 64, iterations=2, seed=11, radius_factor=0.05)
    finally:
        c.close()
    _check(film, st, ref, rst, f"torus64_rf0.05_cell{cell}")


def test_quarter_radius_cells_with_delta_vertices():
    """The spheres scene (glass and mirror: vertices that are never merged)."""
    path, scene = _scene(lambda: _scenes.spheres(64, 64))
    c = _context(scene, 0.25)
    try:
        film, st = c.render_vcm(64, 64, iterations=2, seed=11, radius_factor=0.1)
    finally:
        c.close()
    ref, rst = _oracle.Scene(path).vcm(64, 64, 2, 11, mode=1, radius_factor=0.1)
    _check(film, st, ref, rst, "spheres64_rf0.1_cell0.25")


@pytest.mark.parametrize("cell", [0.25, 8])
def test_query_spans_at_the_cell_clamp(cell):
    """The zoo's `scales` family: the merge radius follows the 4e5-wide scene
    and every light vertex lies within it of every camera vertex, so a query's
    span is the whole occupied grid, and the far vertices' coordinates run
    against vcm_cell's +-2^30 clamp."""
    path, scene = _scene(lambda: gz.scene("scales", 32, 32))
    if "scales" not in _clamp_ref:
        _clamp_ref["scales"] = _oracle.Scene(path).vcm(32, 32, 2, 3, mode=1, radius_factor=0.05)
    ref, rst = _clamp_ref["scales"]
    c = _context(scene, cell)
    try:
        film, st = c.render_vcm(32, 32, iterations=2, seed=3, radius_factor=0.05)
    finally:
        c.close()
    _check(film, st, ref, rst, f"scales32_rf0.05_cell{cell}")
