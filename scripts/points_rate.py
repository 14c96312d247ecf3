"""The rate of the point-set calls on device arrays on a
surface-distributed workload, like photons: torus, the points are the hit
positions of the 2^21 camera rays of a 2048x1024 FILM_PT film, the queries the
hit positions of those rays' first scattered directions (bsdf_sample_t), the
radius VCM's 0.003 x sceneRadius with cell = radius; k = 50 and 8 with
max_sqr_dist = (4 radius)^2.  Per call -- the build, count_t, the fill
(fill_t into preallocated offsets and indices), knn_t at both k -- 3 warm-up
calls, then the median / minimum / maximum of --calls calls on the host clock
(every call returns when its outputs are written).

Two yardsticks, timed the same way: a plain device copy (torch's copy_, then
synchronize) of the bytes the call must at least read and write, and, in the
step `small`, the chunked torch.cdist + topk brute force at 2^15 points x 2^15
queries (an even subset of each), where it still fits, beside the index at that
same size.

Every step is a fresh process under its own `timeout`, one after the other;
the first step that fails ends the run.  The result goes to
profiles/r18/points/rates.json (--out).

    python scripts/points_rate.py [--calls 20] [--width 2048 --height 1024]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "winmad-s-raytracer-v1.0_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

STEPS = ("build", "count", "fill", "knn50", "knn8", "small")
STEP_TIMEOUT_S = 300

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--width", type=int, default=2048)
ap.add_argument("--height", type=int, default=1024)
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "r18", "points", "rates.json"))
ap.add_argument("--steps", default=",".join(STEPS), help="the steps to run, comma-separated")
ap.add_argument("--step", default=None, help="internal: run that step here and print its JSON line")
args = ap.parse_args()
W, H = args.width, args.height


def timed(fn, calls):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()  # returns when the answer is written
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def scene_radius(scene):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "scene.txt")
        scene.dump(path)
        for line in open(path):
            if line.startswith("sphere"):
                return float.fromhex(line.split()[4])
    raise SystemExit("no sphere line in the scene dump")


def run_step(step):
    import _scenes
    from winmad_rt import native
    native.lib()
    import torch

    scene = native.Scene(_scenes.torus(W, H))
    ctx = native.Context(scene, 0)
    dev = f"cuda:{ctx.devices()[0]}"
    rays = ctx.camera_rays_t(W, H, native.FILM_PT)
    hits = ctx.trace_closest_t(rays)
    hf = native.hit_fields(hits)
    hit = hf["prim"] >= 0
    pts = hf["p"][hit].contiguous()
    u = ctx.rng_uniform_t(rays.shape[0], 3, 5489, 0, 2)
    _, smp = ctx.bsdf_sample_t(hits, (-rays[:, 3:6]).contiguous(), u)
    sf = native.bsdf_sample_fields(smp)
    go = hit & (sf["pdf"] > 0)
    wo = sf["wo"][go]
    r2 = torch.zeros((wo.shape[0], 8), dtype=torch.float32, device=dev)
    r2[:, 0:3] = hf["p"][go] + wo * 1e-3
    r2[:, 3:6] = wo
    r2[:, 7] = 1e7
    h2 = native.hit_fields(ctx.trace_closest_t(r2))
    q = h2["p"][h2["prim"] >= 0].contiguous()
    radius = 0.003 * scene_radius(scene)
    m2 = (4 * radius) ** 2
    n, nq = pts.shape[0], q.shape[0]
    res = {"step": step, "points": n, "queries": nq, "radius": radius, "lib_sha": native.library_sha16()}

    def copy_yardstick(nbytes):
        half = max(1, nbytes // 8)
        src = torch.zeros((half,), dtype=torch.int32, device=dev)
        dst = torch.empty_like(src)

        def copy():
            dst.copy_(src)
            torch.cuda.synchronize()

        t = timed(copy, args.calls)
        return {"copy_bytes": 8 * half, **{"copy_" + k: v for k, v in t.items()}}

    if step == "small":
        sp = pts[::max(1, n >> 15)][:1 << 15].contiguous()  # 2^15 of each, spread over the whole set
        sq = q[::max(1, nq >> 15)][:1 << 15].contiguous()
        res.update(points=sp.shape[0], queries=sq.shape[0])
        k = min(50, sp.shape[0])

        def brute():
            for a in range(0, sq.shape[0], 4096):  # 4,096 x 2^15 distances at a time
                d = torch.cdist(sq[a:a + 4096], sp)
                d.topk(k, dim=1, largest=False)
                (d < radius).sum(1)
            torch.cuda.synchronize()

        res["brute_cdist_topk_count"] = timed(brute, args.calls)
        idx = ctx.points_index_t(sp, radius)

        def index():
            idx.knn_t(sq, k, m2)
            idx.count_t(sq, radius=radius)

        res["index_knn50_count"] = timed(index, args.calls)
        res["index_build"] = timed(lambda: ctx.points_index_t(sp, radius).close(), args.calls)
        return res
    if step == "build":
        idx = ctx.points_index_t(pts, radius)
        res["info"] = idx.info()
        idx.close()
        res.update(timed(lambda: ctx.points_index_t(pts, radius).close(), args.calls))
        res.update(copy_yardstick(12 * n + res["info"]["device_bytes"]))
        res["mpoints_per_s"] = round(n / res["median_ms"] / 1e3, 1)
        return res
    idx = ctx.points_index_t(pts, radius)
    if step == "count":
        out = torch.empty((nq,), dtype=torch.int32, device=dev)
        res.update(timed(lambda: idx.count_t(q, radius=radius, out=out), args.calls))
        res["found_per_query"] = round(float(out.sum()) / nq, 2)
        res.update(copy_yardstick(16 * nq + 16 * n))
    elif step == "fill":
        offset, index = idx.in_radius_t(q, radius=radius)
        res.update(timed(lambda: idx.fill_t(q, offset, index, radius=radius), args.calls))
        res["found_per_query"] = round(index.shape[0] / nq, 2)
        res.update(copy_yardstick(20 * nq + 16 * n + 4 * index.shape[0]))
    else:
        k = int(step[3:])
        res.update(timed(lambda: idx.knn_t(q, k, m2), args.calls))  # (allocates its three outputs per call)
        cnt = idx.knn_t(q, k, m2)[2]
        res["found_per_query"] = round(float(cnt.sum()) / nq, 2)
        res.update(copy_yardstick(12 * nq + 16 * n + nq * (8 * k + 4)))
    res["mqueries_per_s"] = round(nq / res["median_ms"] / 1e3, 2)
    return res


if args.step:
    print(json.dumps(run_step(args.step)))
    sys.exit(0)

res = {"scene": f"torus {W}x{H}", "calls": args.calls, "steps": []}
for step in args.steps.split(","):
    cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", step,
           "--calls", str(args.calls), "--width", str(W), "--height", str(H)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:  # nothing more on the GPU after a step that failed
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"step {step} ended with status {r.returncode}")
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(out), flush=True)
    res["steps"].append(out)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
