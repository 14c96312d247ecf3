"""CPU checks of the BVH's top-first node order (wrf::build_fast's top / top4
budgets, wr_bvh.h): the first ntop nodes are a parent-closed set with the root
at 0, every inner link is in range and reached exactly once, and the tree is
the build-order tree under another numbering -- the same leaf links, every
node's boxes equal to its old self's bit for bit -- for the binary and the
4-wide tree (tests/native/bvh_top_check.cpp, compiled here from the product's
own sources).  The scenes of 1 to 3 triangles cover the root that holds a leaf
(at most kMaxLeaf triangles) and trees smaller than the budget."""
import os
import subprocess
import tempfile

import pytest

import _scenes
import _tiny_scenes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "winmad-s-raytracer-v1.0_amd", "csrc")
_bin = []


def checker():
    if not _bin:
        out = os.path.join(tempfile.mkdtemp(prefix="wr_bvhtop_"), "bvh_top_check")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-I", os.path.join(REPO, "include"),
                        os.path.join(REPO, "tests", "native", "bvh_top_check.cpp"), os.path.join(CSRC, "wr_scene.cpp"),
                        os.path.join(CSRC, "wr_bvh.cpp"), "-o", out, "-lpthread"], check=True)
        _bin.append(out)
    return _bin[0]


SCENES = {"torus": lambda: _scenes.torus(64, 64), "cbox_dragon": lambda: _scenes.cbox(64, 48),
          "spheres": lambda: _scenes.spheres(64, 64), "tri1": lambda: _tiny_scenes.tiny(1),
          "tri2": lambda: _tiny_scenes.tiny(2), "tri3": lambda: _tiny_scenes.tiny(3)}


@pytest.mark.parametrize("top,top4", [(127, 63), (63, 127), (255, 1), (1, 255)])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_top_first_order_is_the_same_tree(name, top, top4):
    r = subprocess.run([checker(), SCENES[name](), str(top), str(top4)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    f = r.stdout.split()
    nodes, ntop, nodes4, ntop4 = int(f[2]), int(f[4]), int(f[6]), int(f[8])
    assert ntop == min(top, nodes) and ntop4 == min(top4, nodes4), r.stdout
    if name.startswith("tri"):  # at most two nodes: a budget of 63 or more takes the whole tree
        assert nodes <= 2 and nodes4 == 1, r.stdout
        assert (ntop == nodes or top < nodes) and ntop4 == nodes4, r.stdout
