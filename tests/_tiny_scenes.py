"""Scenes of a few triangles (tests of the BVH's small-tree paths): the root
that is a leaf holder (at most wrf::kMaxLeaf triangles) and trees smaller than
any top set."""
import os

import _scenes
from winmad_rt import scenes

# (vertices, faces): triangles in front of the torus scene's camera axis
_V = [(-50, 0, -50), (50, 0, -50), (0, 0, 50), (-40, 30, -40), (40, 30, -40), (0, 30, 40), (-30, 60, -30), (30, 60, -30),
      (0, 60, 30)]


def tiny(ntri, W=32, H=32):
    """A scene of `ntri` (1..3) stacked triangles seen from above."""
    obj = os.path.join(_scenes._DIR, f"tiny{ntri}.obj")
    if not os.path.exists(obj):
        with open(obj, "w") as f:
            for v in _V[:3 * ntri]:
                f.write("v %g %g %g\n" % v)
            for t in range(ntri):
                f.write("f %d %d %d\n" % (3 * t + 1, 3 * t + 2, 3 * t + 3))
    text = "<scene>\n"
    text += scenes._camera((3, 300, 5), (0, -1, 0), (0, 0, -1), H, W, 40)
    text += scenes._mat()
    text += scenes._mat(d=("0.7", "0.7", "0.7"))
    text += scenes._obj(obj, 1)
    text += "</scene>\n"
    return _scenes.path(f"tiny{ntri}_{W}x{H}.scene", text)
