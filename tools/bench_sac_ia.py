"""SAC-IA timing (dlg_sac_ia_align): source and target are tools/bench_icp.py's two independently
sampled copies of the C5 cloud, the target moved by a small rigid motion, at 1M and 10M points each.
The descriptors are RANDOM finite rows (uniform in [0, 100)): they cost what real FPFH rows cost to
search, and the hypotheses they produce are as wrong as most of a real run's are, which is all the
timing needs.  max_correspondence_distance = 0.01 (PCL compares it with the squared distance), so the
nearest-point search runs; 1000 iterations (PCL's default); warm calls with profiling on.

Per size: knn_ms (the batched descriptor search, HIP events) against its VALU floor -- n_queries x
n_rows x 99 lane-operations at 78.6 T non-FMA lane-ops/s -- score_ms in all
and per scored hypothesis (HIP events around every batch), the one-off hierarchy build (host clock,
its read-backs included) and the wall time per call.  As the scorer's yardstick from the same
process: one dlg_icp_align iteration on the same clouds (device ms per iteration, as
tools/bench_icp.py reports it).

  python tools/bench_sac_ia.py [--sizes 1000000,10000000] [--reps 2] [--iterations 1000]
                               [--out profiles/r13_sac_ia.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dialog_amd as D  # noqa: E402
from bench_icp import clouds, spread  # noqa: E402

VALU_NON_FMA_LANE_OPS = 78.6e12
MAX_DIST = 0.01


def bench_size(ctx, n, reps, iterations):
    src, tgt = clouds(n)
    rng = np.random.default_rng(n)
    fs = (rng.random((n, 33), dtype=np.float32) * np.float32(100.0))
    ft = (rng.random((n, 33), dtype=np.float32) * np.float32(100.0))
    kw = dict(max_correspondence_distance=MAX_DIST, ctx=ctx, return_stats=True)
    D.sac_ia_align(src, fs, tgt, ft, max_iterations=min(iterations, 20), **kw)  # warm
    knn, score, build, wall = [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        final, aligned, st = D.sac_ia_align(src, fs, tgt, ft, max_iterations=iterations, **kw)
        wall.append((time.perf_counter() - t0) * 1e3)
        knn.append(st["knn_ms"])
        score.append(st["score_ms"])
        build.append(st["build_ms"])
    scored = st["n_valid"]
    floor_ms = st["n_queries"] * n * 99 / VALU_NON_FMA_LANE_OPS * 1e3
    row = dict(n_source=n, n_target=n, iterations=st["iterations"], hypotheses_scored=scored,
               n_queries=st["n_queries"], batches=st["batches"], levels=st["levels"],
               best_iteration=st["best_iteration"], error=st["error"], host_syncs=st["host_syncs"],
               knn_ms=spread(knn), knn_valu_floor_ms=round(floor_ms, 3),
               knn_over_valu_floor=round(float(np.median(knn)) / floor_ms, 3),
               score_ms=spread(score),
               score_ms_per_hypothesis=round(float(np.median(score)) / max(scored, 1), 4),
               hierarchy_build_ms=spread(build), wall_ms_per_align=spread(wall))
    print(json.dumps(row), flush=True)
    # the yardstick: one iteration of the registration on the same clouds
    D.icp_align(src, tgt, ctx=ctx)
    dev, its = [], []
    for _ in range(reps):
        _, _, ist = D.icp_align(src, tgt, ctx=ctx, return_stats=True)
        dev.append(ist["device_ms"])
        its.append(ist["iterations"])
    per_it = float(np.median(dev)) / its[-1]
    row["icp_device_ms_per_iteration"] = round(per_it, 3)
    row["score_per_hypothesis_over_icp_iteration"] = round(row["score_ms_per_hypothesis"] / per_it, 3)
    print(json.dumps({k: row[k] for k in ("icp_device_ms_per_iteration",
                                          "score_per_hypothesis_over_icp_iteration")}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = D.Context(0)
    ctx.set_profiling(True)
    res = dict(tool="tools/bench_sac_ia.py", cloud="two independent samples of C5 at each size, the "
               "target moved by 1 degree about z and (0.02, -0.01, 0.015); random finite descriptor "
               "rows (uniform in [0, 100)), for timing only",
               max_correspondence_distance=MAX_DIST, results=[])
    for n in [int(v) for v in a.sizes.split(",") if v]:
        res["results"].append(bench_size(ctx, n, a.reps, a.iterations))
        if a.out:  # (kept after every size: a long run that is cut short still leaves its rows)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    ctx.close()
    print(json.dumps({"done": True, "out": a.out}))


if __name__ == "__main__":
    main()
