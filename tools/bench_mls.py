"""Moving-least-squares timing (dlg_moving_least_squares, dlg_moving_least_squares_cloud): the C5
cloud generated at 1M and 10M points, radius 0.1, polynomial orders 2 and 3, warm calls with profiling on.

Per (size, order): device ms per call over --reps calls of the host-output entry and of the _cloud
entry (median, min, max: HIP events from after the grid build to the last kernel, host copies
excluded), wall ms per call, the branch counts, and the neighbour-count distribution (median, max,
share of queries past the on-chip buffer).  As the yardstick from the same process: the radius-0.1
normals on the same cloud (dlg_cloud_estimate_normals on a device-resident copy, wall ms per call
ending in a synchronise: it reports no event time), which runs the same scan plus a sort, in
float.  The ratios in the output name the two clocks they divide.

  python tools/bench_mls.py [--sizes 1000000,10000000] [--reps 5] [--out profiles/r10_mls.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dialog_amd as D  # noqa: E402
from dialog_amd import _lib  # noqa: E402
from dialog_amd.sac import _f32p, _i32p  # noqa: E402
from dialog_amd.synth import config_cloud  # noqa: E402

RADIUS = 0.1
ORDERS = (2, 3)


class Runner:
    """both entries on one cloud with the host buffers allocated once"""

    def __init__(self, ctx, p):
        self.ctx, self.p, self.n = ctx, p, p.shape[0]
        self.pts = _lib.Points(_f32p(p), self.n, 12)
        self.xyz = np.empty((self.n, 3), np.float32)
        self.nrm = np.empty((self.n, 4), np.float32)
        self.src = np.empty(self.n, np.int32)
        self.nb = np.empty(self.n, np.int32)
        self.L = _lib.load()

    def host(self, order):
        prm = _lib.MlsParams(RADIUS, 1, order, 1, 0.0)
        k = C.c_int64()
        st = _lib.MlsStats()
        t0 = time.perf_counter()
        self.ctx.check(self.L.dlg_moving_least_squares(
            self.ctx.h, C.byref(self.pts), None, 0, C.byref(prm), _f32p(self.xyz), 12,
            _f32p(self.nrm), self.n, C.byref(k), _i32p(self.src), _i32p(self.nb), C.byref(st)))
        return st, (time.perf_counter() - t0) * 1e3

    def cloud(self, order):
        prm = _lib.MlsParams(RADIUS, 1, order, 1, 0.0)
        k = C.c_int64()
        h = C.c_void_p()
        st = _lib.MlsStats()
        t0 = time.perf_counter()
        self.ctx.check(self.L.dlg_moving_least_squares_cloud(
            self.ctx.h, C.byref(self.pts), None, 0, C.byref(prm), 0, C.byref(h), C.byref(k), None,
            C.byref(st)))
        w = (time.perf_counter() - t0) * 1e3
        D.Cloud._from_handle(self.ctx, h, k.value).close()
        return st, w


def spread(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3),
                max=round(float(max(v)), 3), calls=len(v))


def bench_cloud(ctx, p, reps):
    n = p.shape[0]
    r = Runner(ctx, p)
    rows = []
    for order in ORDERS:
        row = dict(n=n, radius=RADIUS, order=order)
        for name, fn in (("host", r.host), ("cloud", r.cloud)):
            fn(order)  # warm: allocations, code objects, hipcub's choices
            dev, wall = [], []
            for _ in range(reps):
                st, w = fn(order)
                dev.append(st.device_ms)
                wall.append(w)
            row[name + "_device_ms"] = spread(dev)
            row[name + "_wall_ms"] = spread(wall)
        nb = r.nb[r.nb >= 0]
        row.update(n_out=int(st.n_out), n_too_few=int(st.n_too_few),
                   n_plane_only=int(st.n_plane_only), n_fit_nonfinite=int(st.n_fit_nonfinite),
                   neighbours=dict(median=float(np.median(nb)), mean=round(float(nb.mean()), 2),
                                   p99=float(np.percentile(nb, 99)), max=int(nb.max()),
                                   reread_share=round(float(st.n_lds_overflow) / max(len(nb), 1),
                                                      6)))
        print(json.dumps(row), flush=True)
        rows.append(row)
    cl = D.Cloud(ctx, p)
    cl.estimate_normals(radius=RADIUS)
    ctx.synchronize()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        cl.estimate_normals(radius=RADIUS)
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    cl.close()
    nrm = dict(n=n, radius=RADIUS, wall_ms=spread(wall))
    print(json.dumps(dict(normals_radius=nrm)), flush=True)
    d2 = rows[0]["host_device_ms"]["median"]
    return dict(n=n, mls=rows, normals_radius=nrm,
                mls_o2_device_over_normals_wall=round(d2 / nrm["wall_ms"]["median"], 3),
                mls_o3_device_over_o2_device=round(rows[1]["host_device_ms"]["median"] / d2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = D.Context(0)
    ctx.set_profiling(True)
    res = dict(tool="tools/bench_mls.py", cloud="C5 generated at each size (the same extents: "
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
