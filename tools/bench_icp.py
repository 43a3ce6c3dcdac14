"""Rigid-registration timing (dlg_icp_align): source and target are two independently sampled copies
of the C5 cloud, the target moved by a small rigid motion, at 1M and 10M points each; the defaults
(10 iterations), warm calls with profiling on.

Per size: device ms per align over --reps calls (median, min, max: HIP events from after the target
hierarchy's build to the last kernel, host copies excluded) and per iteration, the one-off
hierarchy build (host clock around it, its read-backs included), wall ms per call, and the stream
synchronisations inside the loop per iteration as the driver counted them.  As the yardstick from
the same process: dlg_orient_normals_nn with the same query and target sizes (a 1-NN search of the
same shape that rebuilds its grid and reads back per level on every call), wall ms per call ending
in a synchronise (it reports no event time, and its clock includes its uploads: a correspondence-
only call of the registration, dlg_icp_correspondences, is timed on that same clock beside it).
The ratios in the output name the two clocks they divide.

  python tools/bench_icp.py [--sizes 1000000,10000000] [--reps 3] [--out profiles/r11_icp.json]
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
from dialog_amd.synth import CONFIGS, SEED_BASE, plane_cloud  # noqa: E402


def spread(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3),
                max=round(float(max(v)), 3), calls=len(v))


def motion():
    th = np.radians(1.0)
    T = np.eye(4, dtype=np.float32)
    T[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    T[:3, 3] = [0.02, -0.01, 0.015]
    return T


def clouds(n):
    c = CONFIGS[5]
    src = plane_cloud(n, c["n_planes"], shares=c["shares"], seed=SEED_BASE + 5, shard=0)[0]
    tgt = plane_cloud(n, c["n_planes"], shares=c["shares"], seed=SEED_BASE + 5, shard=1)[0]
    T = motion()
    tgt = (tgt @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt)


def bench_size(ctx, n, reps):
    src, tgt = clouds(n)
    D.icp_align(src, tgt, ctx=ctx)  # warm: allocations, code objects, hipcub's choices
    dev, wall, build, syncs, its = [], [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        final, aligned, st = D.icp_align(src, tgt, ctx=ctx, return_stats=True)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(st["device_ms"])
        build.append(st["build_ms"])
        syncs.append(st["host_syncs"])
        its.append(st["iterations"])
    row = dict(n_source=n, n_target=n, iterations=its[-1], state=st["state_name"],
               levels=st["levels"], n_corr=st["n_corr"], mse=st["mse"],
               device_ms_per_align=spread(dev), wall_ms_per_align=spread(wall),
               hierarchy_build_ms=spread(build),
               device_ms_per_iteration=round(float(np.median(dev)) / its[-1], 3),
               host_syncs_per_iteration=round(float(np.median(syncs)) / its[-1], 3))
    print(json.dumps(row), flush=True)
    # the yardstick, and the correspondence-only call on its clock
    nrm = np.zeros((n, 4), np.float32)
    nrm[:, 2] = 1.0
    D.orient_normals_nn(src, nrm, tgt, nrm, ctx=ctx)
    ctx.synchronize()
    nn_wall, corr_wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        D.orient_normals_nn(src, nrm, tgt, nrm, ctx=ctx)
        ctx.synchronize()
        nn_wall.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        D.icp_correspondences(src, tgt, ctx=ctx)
        ctx.synchronize()
        corr_wall.append((time.perf_counter() - t0) * 1e3)
    y = dict(orient_normals_nn_wall_ms=spread(nn_wall), icp_correspondences_wall_ms=spread(corr_wall))
    print(json.dumps(y), flush=True)
    nnw = float(np.median(nn_wall))
    row.update(y)
    row["icp_device_per_iteration_over_nn_wall"] = round(row["device_ms_per_iteration"] / nnw, 3)
    row["icp_wall_per_align_over_iterations_over_nn_wall"] = round(
        float(np.median(wall)) / its[-1] / nnw, 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = D.Context(0)
    ctx.set_profiling(True)
    res = dict(tool="tools/bench_icp.py", cloud="two independent samples of C5 at each size, the "
               "target moved by 1 degree about z and (0.02, -0.01, 0.015)", results=[])
    for n in [int(v) for v in a.sizes.split(",") if v]:
        res["results"].append(bench_size(ctx, n, a.reps))
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({"done": True, "out": a.out}))


if __name__ == "__main__":
    main()
