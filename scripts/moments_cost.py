"""What second-moment films cost: torus 1920x1080 BDPT, 20
iterations into device films, rendered three ways with one library --
  (a) plain:    one wr_render_bdpt call (the sum only),
  (b) moments:  one wr_render_bdpt_moments call (sum and sum of squares),
  (c) folded:   twenty one-iteration wr_render_bdpt calls, each into a scratch
                film that torch adds to the sum and, squared, to the sum of
                squares: what a caller had to do before (b) existed.
The three alternate, --repeats times, after one warm-up of each; the line
printed is JSON: per way the wall seconds of every repeat, the median and its
Mrays/s, the ratios b/a and c/b, and the kernel-time columns of wr_stats
(time_kernels = 1, a run of its own after the timed ones) of (a) and (b).

    python scripts/moments_cost.py [--iterations 20] [--repeats 3] [--width 1920 --height 1080]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "winmad-s-raytracer-v1.0_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import _scenes  # noqa: E402
from winmad_rt import native  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iterations", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--seed", type=int, default=5489)
args = ap.parse_args()
W, H, K = args.width, args.height, args.iterations

native.lib()  # asks for 16 hardware queues before HIP initialises
import torch  # noqa: E402

ctx = native.Context(native.Scene(_scenes.torus(W, H)), 0, trace=native.TRACE_BVH)
film, film_sq, one = (torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0") for _ in range(3))


def plain(**kw):
    return ctx.render_bdpt(W, H, iterations=K, seed=args.seed, film_ptr=film.data_ptr(), **kw)[1]


def moments(**kw):
    return ctx.render_bdpt_moments(W, H, iterations=K, seed=args.seed, film_ptr=film.data_ptr(),
                                   film_sq_ptr=film_sq.data_ptr(), **kw)[2]


def folded(**kw):
    rays = 0
    for i in range(K):
        one.zero_()
        st = ctx.render_bdpt(W, H, iterations=1, seed=args.seed, iter_begin=i, film_ptr=one.data_ptr(), **kw)[1]
        film.add_(one)
        film_sq.addcmul_(one, one)
        rays += st.closest_rays + st.shadow_rays
    return rays


def timed(fn):
    film.zero_()
    film_sq.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, (r if isinstance(r, int) else r.closest_rays + r.shadow_rays), r


ways = {"plain": plain, "moments": moments, "folded": folded}
for fn in ways.values():  # warm-up: allocations, caches
    timed(fn)
secs = {k: [] for k in ways}
rays = {}
pipes = {}
for _ in range(args.repeats):
    for k, fn in ways.items():
        dt, n, r = timed(fn)
        secs[k].append(round(dt, 5))
        rays[k] = n
        if not isinstance(r, int):
            pipes[k] = int(r.pipelines)
med = {k: statistics.median(v) for k, v in secs.items()}
out = {"scene": f"torus {W}x{H} BDPT", "iterations": K, "repeats": args.repeats, "lib_sha": native.library_sha16(),
       "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "seconds": secs, "median_s": med, "rays": rays,
       "pipelines": pipes, "mrays_per_s": {k: round(rays[k] / med[k] / 1e6, 1) for k in ways},
       "moments_over_plain": round(med["moments"] / med["plain"], 4),
       "folded_over_moments": round(med["folded"] / med["moments"], 4)}
names = ["trace", "shade", "resolve", "gen", "other"]
for k, fn in (("plain", plain), ("moments", moments)):  # where the time goes: summed launch durations per category
    _, _, st = timed(lambda: fn(time_kernels=1))
    out[f"kernel_ms_{k}"] = {n: round(st.kernel_ms[i], 3) for i, n in enumerate(names)}
    out[f"kernel_launches_{k}"] = {n: int(st.kernel_launches[i]) for i, n in enumerate(names)}
    out[f"trace_wall_ms_{k}"] = round(st.trace_wall_ms, 3)
print(json.dumps(out))
assert rays["plain"] == rays["moments"] == rays["folded"], rays
assert med["moments"] < med["folded"], "a moments render must beat folding one-iteration renders"
