"""The rate of the ray-batch API, host arrays against device arrays (DESIGN.md
12): torus, the 2^22 camera rays of a 2048x2048 FILM_PT film, in raster order
and in one fixed torch.randperm order.  Timed: trace_closest (numpy in, numpy
out) against trace_closest_t (tensors in HBM), and path_radiance against
path_radiance_t -- 3 warm-up calls, then the median / minimum / maximum of
--calls calls on the host clock (every call returns when its answer is
written; the host calls' time includes their copies, which is the point).

Every (order, call) pair is a step of its own: a fresh process under its own
`timeout`, one after the other; the first step that fails ends the run.  The
result goes to profiles/r13/device_rays/rate.json (--out).

    python scripts/device_rays_rate.py [--calls 20] [--width 2048 --height 2048]
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

ORDERS = ("raster", "shuffled")
CALLS = ("trace_closest", "trace_closest_t", "path_radiance", "path_radiance_t")
STEP_TIMEOUT_S = 240

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--width", type=int, default=2048)
ap.add_argument("--height", type=int, default=2048)
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "r13", "device_rays", "rate.json"))
ap.add_argument("--step", default=None, help="internal: ORDER:CALL, run that step here and print its JSON line")
args = ap.parse_args()
W, H = args.width, args.height
N = W * H


def run_step(order, call):
    import _scenes
    from winmad_rt import native
    native.lib()  # asks for 16 hardware queues before HIP initialises
    import torch

    ctx = native.Context(native.Scene(_scenes.torus(W, H)), 0)
    rays = ctx.camera_rays_t(W, H, native.FILM_PT)
    if order == "shuffled":
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(0))
        rays = rays[perm.to(rays.device)].contiguous()
    torch.cuda.synchronize()
    host = rays.cpu().numpy()
    hits = torch.empty((N, 10), dtype=torch.int32, device=rays.device)
    rgb = torch.zeros((N, 3), dtype=torch.float32, device=rays.device)
    torch.cuda.synchronize()
    fn = {"trace_closest": lambda: ctx.trace_closest(host),
          "trace_closest_t": lambda: ctx.trace_closest_t(rays, out=hits),
          "path_radiance": lambda: ctx.path_radiance(host),
          "path_radiance_t": lambda: ctx.path_radiance_t(rays, rgb=rgb)}[call]
    for _ in range(3):
        fn()
    ms = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        fn()  # returns when the answer is written
        ms.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(ms)
    return {"order": order, "call": call, "rays": N, "median_ms": round(med, 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "mrays_per_s": round(N / med / 1e3, 1), "lib_sha": native.library_sha16()}


if args.step:
    print(json.dumps(run_step(*args.step.split(":"))))
    sys.exit(0)

res = {"scene": f"torus {W}x{H}", "rays": N, "calls": args.calls, "steps": []}
for order in ORDERS:
    for call in CALLS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step",
               f"{order}:{call}", "--calls", str(args.calls), "--width", str(W), "--height", str(H)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:  # nothing more on the GPU after a step that failed
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"step {order}:{call} ended with status {r.returncode}")
        step = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        print(json.dumps(step), flush=True)
        res["steps"].append(step)
by = {(s["order"], s["call"]): s["median_ms"] for s in res["steps"]}
res["host_over_device"] = {f"{o}:{c}": round(by[(o, c)] / by[(o, c + "_t")], 3)
                           for o in ORDERS for c in ("trace_closest", "path_radiance")}
res["raster_over_shuffled"] = {c: round(by[("raster", c)] / by[("shuffled", c)], 3) for c in CALLS}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps({k: res[k] for k in ("host_over_device", "raster_over_shuffled")}))
