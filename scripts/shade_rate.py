"""The rate of the shading calls on device arrays: torus, the
hits of the 2^22 camera rays of a 2048x2048 FILM_PT film, one call per step --
bsdf_eval_t, bsdf_sample_t, light_illuminate_t, light_emit_t, light_radiance_t,
rng_uniform_t (3 draws, counters kept) -- each into preallocated outputs.
3 warm-up calls, then the median / minimum / maximum of --calls calls on the
host clock (every call returns when its records are written).

The yardstick of a step is a plain copy of the same bytes in the same process:
torch's copy_ of an int32 buffer that reads half and writes half of what the
call moves per record, timed the same way (copy_, then synchronize).

Every call is a step of its own: a fresh process under its own `timeout`, one
after the other; the first step that fails ends the run.  The result goes to
profiles/r15/shading/rates.json (--out).

    python scripts/shade_rate.py [--calls 20] [--width 2048 --height 2048]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "winmad-s-raytracer-v1.0_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

# bytes read + written per record: hits 40, a direction or sample 12, a light id 4, and the record written
BYTES = {"bsdf_eval_t": 40 + 12 + 12 + 36 + 32, "bsdf_sample_t": 40 + 12 + 12 + 36 + 36,
         "light_illuminate_t": 4 + 12 + 12 + 40, "light_emit_t": 4 + 12 + 12 + 48, "light_radiance_t": 40 + 12 + 20,
         "rng_uniform_t": 4 + 4 + 12}
HBM_PEAK = 8.0e12  # bytes / s, the MI355X's specified peak
STEP_TIMEOUT_S = 240

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--width", type=int, default=2048)
ap.add_argument("--height", type=int, default=2048)
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "r15", "shading", "rates.json"))
ap.add_argument("--step", default=None, help="internal: CALL, run that step here and print its JSON line")
args = ap.parse_args()
W, H = args.width, args.height
N = W * H


def timed(fn, calls):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()  # returns when the answer is written
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def run_step(call):
    import _scenes
    from winmad_rt import native
    native.lib()  # asks for 16 hardware queues before HIP initialises
    import torch

    ctx = native.Context(native.Scene(_scenes.torus(W, H)), 0)
    dev = f"cuda:{ctx.devices()[0]}"
    rays = ctx.camera_rays_t(W, H, native.FILM_PT)
    hits = ctx.trace_closest_t(rays)
    d = rays[:, 3:6].contiguous()
    wi = -d
    u = ctx.rng_uniform_t(N, 6, 5489, 0, 2)
    a, b = u[:, 0:3].contiguous(), u[:, 3:6].contiguous()
    pos = native.hit_fields(hits)["p"].contiguous()
    light = torch.zeros((N,), dtype=torch.int32, device=dev)
    out = lambda words: torch.empty((N, words), dtype=torch.int32, device=dev)
    info, o8, o9, o10, o12, o5 = out(9), out(8), out(9), out(10), out(12), out(5)
    ctr = torch.zeros((N,), dtype=torch.int32, device=dev)
    r3 = torch.empty((N, 3), dtype=torch.float32, device=dev)
    fn = {"bsdf_eval_t": lambda: ctx.bsdf_eval_t(hits, wi, a, info=info, out=o8),
          "bsdf_sample_t": lambda: ctx.bsdf_sample_t(hits, wi, a, info=info, out=o9),
          "light_illuminate_t": lambda: ctx.light_illuminate_t(light, pos, a, out=o10),
          "light_emit_t": lambda: ctx.light_emit_t(light, a, b, out=o12),
          "light_radiance_t": lambda: ctx.light_radiance_t(hits, d, out=o5),
          "rng_uniform_t": lambda: ctx.rng_uniform_t(N, 3, 5489, 0, 2, ctr=ctr, out=r3)}[call]
    torch.cuda.synchronize()
    med, lo, hi = timed(fn, args.calls)
    half = N * BYTES[call] // 8  # int32 words: the copy reads half of the call's bytes and writes half
    src = torch.zeros((half,), dtype=torch.int32, device=dev)
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)
        torch.cuda.synchronize()

    cmed, clo, chi = timed(copy, args.calls)
    gbs = N * BYTES[call] / med / 1e6
    cgbs = 2 * half * 4 / cmed / 1e6
    return {"call": call, "records": N, "bytes_per_record": BYTES[call], "median_ms": round(med, 4),
            "min_ms": round(lo, 4), "max_ms": round(hi, 4), "mrecords_per_s": round(N / med / 1e3, 1),
            "gb_per_s": round(gbs, 1), "hbm_peak_fraction": round(gbs * 1e9 / HBM_PEAK, 4),
            "copy_median_ms": round(cmed, 4), "copy_min_ms": round(clo, 4), "copy_max_ms": round(chi, 4),
            "copy_gb_per_s": round(cgbs, 1), "call_over_copy_bandwidth": round(gbs / cgbs, 3),
            "lib_sha": native.library_sha16()}


if args.step:
    print(json.dumps(run_step(args.step)))
    sys.exit(0)

res = {"scene": f"torus {W}x{H}", "records": N, "calls": args.calls, "hbm_peak_bytes_per_s": HBM_PEAK, "steps": []}
for call in BYTES:
    cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", call,
           "--calls", str(args.calls), "--width", str(W), "--height", str(H)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:  # nothing more on the GPU after a step that failed
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"step {call} ended with status {r.returncode}")
    step = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(step), flush=True)
    res["steps"].append(step)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
