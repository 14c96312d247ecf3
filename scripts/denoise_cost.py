"""What the feature films and the denoiser cost: torus
1920x1080, a BDPT moments render of a few iterations into device films, then
wr_render_features and wr_film_denoise on device films, default parameters --
warmed up, then --calls calls each between device events; the line printed is
JSON with the medians.  The denoise is also timed with levels = 1 .. 5: the
differences are the single levels' launches (level t has step 2^t).

Next to the denoise time: (a) its traffic floor -- the bytes the definition
must move (counted below from the film size) over the HBM peak -- and (b) one
1080p BDPT iteration (2.73 ms, BENCH_r06).

    python scripts/denoise_cost.py [--calls 20] [--iterations 4] [--width 1920 --height 1080]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "winmad-s-raytracer-v1.0_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import _scenes  # noqa: E402
from winmad_rt import native  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--iterations", type=int, default=4)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
args = ap.parse_args()
W, H, K = args.width, args.height, args.iterations
HBM_PEAK = 8.0e12       # bytes / s, MI355X HBM3E
BDPT_ITERATION_MS = 2.73  # one 1080p BDPT iteration, BENCH_r06

native.lib()  # asks for 16 hardware queues before HIP initialises
import torch  # noqa: E402

ctx = native.Context(native.Scene(_scenes.torus(W, H)), 0, trace=native.TRACE_BVH)
film, film_sq, nrm, pos, alb, out = (torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0") for _ in range(6))
dep = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()
ctx.render_bdpt_moments(W, H, iterations=K, film_ptr=film.data_ptr(), film_sq_ptr=film_sq.data_ptr())


def features():
    ctx.render_features(W, H, native.FILM_BDPT, normal_ptr=nrm.data_ptr(), albedo_ptr=alb.data_ptr(),
                        position_ptr=pos.data_ptr(), depth_ptr=dep.data_ptr())


def denoise(levels=5, guides=True):
    g = dict(normal_ptr=nrm.data_ptr(), position_ptr=pos.data_ptr(), albedo_ptr=alb.data_ptr()) if guides else {}
    ctx.film_denoise(film.data_ptr(), film_sq.data_ptr(), W, H, K, out.data_ptr(), levels=levels, **g)


def median_ms(fn, calls=args.calls):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()  # ordered after the null stream's work, returns when done
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)


res = {"scene": f"torus {W}x{H}", "passes": K, "calls": args.calls, "lib_sha": native.library_sha16()}
res["features_ms"] = median_ms(features)
by_levels = {n: median_ms(lambda n=n: denoise(n)) for n in range(1, 6)}
res["denoise_ms_by_levels"] = by_levels
res["denoise_ms"] = by_levels[5]
res["denoise_no_guides_ms"] = median_ms(lambda: denoise(5, False))
# levels = 1 is prepare + level 0; each further level adds one launch
res["level_ms"] = {"prepare+step1": by_levels[1][0],
                   **{f"step{1 << (n - 1)}": round(by_levels[n][0] - by_levels[n - 1][0], 4) for n in range(2, 6)}}
res["longest_level"] = max(res["level_ms"], key=res["level_ms"].get)
# the bytes the definition must move: prepare reads S, Q and three guides and
# writes (c, v) and the 10 guide floats; a level reads (c, v) and the guides of
# every pixel once and writes (c, v) (the last level 3 floats)
npix = W * H
prep = npix * (24 + 36 + 16 + 40)
level = npix * (16 + 40 + 16)
floor_bytes = prep + 4 * level + npix * (16 + 40 + 12)
res["floor_bytes"] = floor_bytes
res["floor_ms_at_hbm_peak"] = round(floor_bytes / HBM_PEAK * 1e3, 4)
res["floor_share_of_denoise"] = round(res["floor_ms_at_hbm_peak"] / res["denoise_ms"][0], 4)
res["bdpt_iteration_ms"] = BDPT_ITERATION_MS
res["denoise_over_bdpt_iteration"] = round(res["denoise_ms"][0] / BDPT_ITERATION_MS, 3)
res["features_over_bdpt_iteration"] = round(res["features_ms"][0] / BDPT_ITERATION_MS, 3)
print(json.dumps(res))
