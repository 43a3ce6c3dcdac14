"""Gaussian-sphere plane seeds timing (dlg_cloud_gs_segment): the C5 cloud generated at 1M and 10M
points, uploaded once, k = 20 normals attached on the device (in place of the reference's radius-0.5
normals), then the seed segmentation with the config.txt parameters, warm calls with profiling on.

Per size: the three device phases per call over --reps calls (median, min, max: HIP events around
the vote, the filter, and the labels / connected components / ordering; the grid build of the
points and the read-backs are outside them), the host phases (gradient field and sink
rectification: host clock), wall ms per call, the first call's parameter-space build, and the
call's counts.  As the yardstick from the same process: the k = 20 normals on the same cloud
(dlg_cloud_estimate_normals, wall ms per call ending in a synchronise).

  python tools/bench_gauss_sphere.py [--sizes 1000000,10000000] [--reps 5] [--out FILE.json]
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

K_NN = 20
PHASES = ("vote_ms", "filter_ms", "segment_ms", "device_ms", "host_ms")
COUNTS = ("n_cells", "n_occupied", "n_voters", "n_fallback_votes", "n_filter_pairs", "n_sinks",
          "n_planes", "n_plane_points")


def spread(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3),
                max=round(float(max(v)), 3), calls=len(v))


def bench_cloud(ctx, p, reps):
    n = p.shape[0]
    cl = D.Cloud(ctx, p)
    cl.estimate_normals(k=K_NN)  # warm: allocations, code objects, hipcub's choices
    ctx.synchronize()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        cl.estimate_normals(k=K_NN)
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    nrm = dict(n=n, k=K_NN, wall_ms=spread(wall))
    print(json.dumps(dict(normals_knn=nrm)), flush=True)
    prm = D.gauss_sphere_params()
    t0 = time.perf_counter()
    first = D.cloud_gauss_sphere_segment(cl, prm, return_stats=True)  # warm; builds the space
    first_wall = (time.perf_counter() - t0) * 1e3
    t = {k: [] for k in PHASES + ("wall_ms",)}
    for _ in range(reps):
        t0 = time.perf_counter()
        got = D.cloud_gauss_sphere_segment(cl, prm, return_stats=True)
        t["wall_ms"].append((time.perf_counter() - t0) * 1e3)
        for k in PHASES:
            t[k].append(got["stats"][k])
    cl.close()
    st = got["stats"]
    sizes = np.diff(got["plane_offsets"])
    row = dict(n=n, first_call=dict(wall_ms=round(first_wall, 1),
                                    space_ms=round(first["stats"]["space_ms"], 1)),
               **{k: spread(v) for k, v in t.items()}, **{k: int(st[k]) for k in COUNTS},
               sink_votes=[int(v) for v in got["sink_votes"][:16]],
               plane_sizes=[int(v) for v in sizes[:16]])
    print(json.dumps(row), flush=True)
    return dict(n=n, gauss_sphere=row, normals_knn=nrm,
                device_over_normals_wall=round(row["device_ms"]["median"] /
                                               nrm["wall_ms"]["median"], 3),
                host_share_of_wall=round(row["host_ms"]["median"] / row["wall_ms"]["median"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = D.Context(0)
    ctx.set_profiling(True)
    res = dict(tool="tools/bench_gauss_sphere.py", cloud="C5 generated at each size (the same "
               "extents: the 1M cloud is ten times sparser)", results=[])
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
