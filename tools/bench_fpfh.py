"""FPFH timing (dlg_cloud_fpfh): the C5 cloud generated at 1M and 10M points, uploaded once, radius
0.1 normals attached on the device, then the descriptors at radius 0.1, warm calls with profiling
on.

Per size: device ms per call over --reps calls (median, min, max: HIP events from before the grid
build to the end of the weighting kernel, host copies excluded) and its split into grid build / SPFH
pass / weighting pass, wall ms per call (it ends with the copy of n x 132 bytes to pageable host
memory), the bytes of the n x 33 SPFH table, the call's counts and the neighbour-count
distribution.  As the yardstick from the same process: the radius-0.1 normals on the same cloud
(dlg_cloud_estimate_normals, wall ms per call ending in a synchronise: it reports no event time),
which runs the same scan plus a sort.  The ratio in the output names the two clocks it divides.

  python tools/bench_fpfh.py [--sizes 1000000,10000000] [--reps 5] [--out profiles/r12_fpfh.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dialog_amd as D  # noqa: E402
from dialog_amd.synth import config_cloud  # noqa: E402

RADIUS = 0.1
COUNTS = ("n_finite", "n_nan_rows", "n_zero_rows", "max_neighbours", "n_lds_overflow", "n_pairs",
          "n_pairs_failed", "n_sum_literal")


def spread(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3),
                max=round(float(max(v)), 3), calls=len(v))


def bench_cloud(ctx, p, reps):
    n = p.shape[0]
    cl = D.Cloud(ctx, p)
    cl.estimate_normals(radius=RADIUS)  # warm: allocations, code objects, hipcub's choices
    ctx.synchronize()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        cl.estimate_normals(radius=RADIUS)
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    nrm = dict(n=n, radius=RADIUS, wall_ms=spread(wall))
    print(json.dumps(dict(normals_radius=nrm)), flush=True)
    D.cloud_fpfh(cl, RADIUS)  # warm
    t = {k: [] for k in ("device_ms", "build_ms", "spfh_ms", "weight_ms", "wall_ms")}
    for _ in range(reps):
        t0 = time.perf_counter()
        hist, nb, st = D.cloud_fpfh(cl, RADIUS, return_stats=True)
        t["wall_ms"].append((time.perf_counter() - t0) * 1e3)
        for k in ("device_ms", "build_ms", "spfh_ms", "weight_ms"):
            t[k].append(st[k])
    cl.close()
    fin = nb[nb >= 0]
    sums = hist[:: max(1, n // 4096)].astype(np.float64).reshape(-1, 3, 11).sum(2)
    row = dict(n=n, radius=RADIUS, spfh_table_bytes=int(n) * 33 * 4,
               **{k: spread(v) for k, v in t.items()}, **{k: int(st[k]) for k in COUNTS},
               neighbours=dict(median=float(np.median(fin)), mean=round(float(fin.mean()), 2),
                               p99=float(np.percentile(fin, 99)), max=int(fin.max())),
               sampled_histogram_sums=dict(min=round(float(np.nanmin(sums)), 4),
                                           max=round(float(np.nanmax(sums)), 4)))
    print(json.dumps(row), flush=True)
    return dict(n=n, fpfh=row, normals_radius=nrm,
                fpfh_device_over_normals_wall=round(
                    row["device_ms"]["median"] / nrm["wall_ms"]["median"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = D.Context(0)
    ctx.set_profiling(True)
    res = dict(tool="tools/bench_fpfh.py", cloud="C5 generated at each size (the same extents: "
               "the 1M cloud is ten times sparser)", results=[])
    for n in [int(v) for v in a.sizes.split(",") if v]:
        p, _, _ = config_cloud(5, n_points=n)
        res["results"].append(bench_cloud(ctx, np.ascontiguousarray(p[:, :3], np.float32), a.reps))
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({"done": True, "out": a.out}))


if __name__ == "__main__":
    main()
