"""Statistical outlier filter timing (dlg_statistical_outlier_removal): the C3 cloud with 5 % of
its points replaced by uniform outliers over its bounding box, at 1M and 10M points, mean_k 20, 50
and 150, warm calls with profiling on.

Per (size, mean_k): device ms per call over --reps calls (median, min, max: HIP events from the
first kernel to the last, host copies excluded, the small read-backs between included), wall ms per
call (host buffers in and out, as the C ABI takes them), points removed, literal_queries and
exact_sums.  As a yardstick from the same run: the existing k = 20 normals on the same cloud
(dlg_cloud_estimate_normals on a device-resident copy, wall ms per call ending in a synchronise:
it has no host copies and reports no event time), which walks the same hierarchy with a lane per
query.  The ratios in the output say which two clocks they divide.

  python tools/bench_sor.py [--sizes 1000000,10000000] [--reps 5] [--out profiles/r09_sor.json]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sor.py --trace   (one 1M sequence
      for the per-kernel split; --kernel-stats CSV folds the split into the JSON)
"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dialog_amd as D  # noqa: E402
from dialog_amd import _lib  # noqa: E402
from dialog_amd.sac import _f32p, _i32p  # noqa: E402
from dialog_amd.synth import config_cloud  # noqa: E402

MEAN_KS = (20, 50, 150)


def outlier_cloud(base, n, frac=0.05, seed=9):
    """the first n points of `base`, the last frac of them replaced by uniform points over the
    bounding box"""
    p = np.ascontiguousarray(base[:n, :3], np.float32).copy()
    k = int(n * frac)
    rng = np.random.default_rng(seed)
    lo, hi = p.min(0), p.max(0)
    p[n - k:] = (lo + (hi - lo) * rng.random((k, 3), dtype=np.float32)).astype(np.float32)
    return p


class Runner:
    """dlg_statistical_outlier_removal on one cloud with buffers allocated once"""

    def __init__(self, ctx, p):
        self.ctx, self.p, self.n = ctx, p, p.shape[0]
        self.pts = _lib.Points(_f32p(p), self.n, 12)
        self.kept = np.empty(self.n, np.int32)
        self.L = _lib.load()

    def call(self, mean_k, mul=1.0):
        prm = _lib.SorParams(mean_k, 0, mul)
        nk, nr = C.c_int64(), C.c_int64()
        st = _lib.SorStats()
        t0 = time.perf_counter()
        self.ctx.check(self.L.dlg_statistical_outlier_removal(
            self.ctx.h, C.byref(self.pts), None, 0, C.byref(prm), _i32p(self.kept), self.n,
            C.byref(nk), None, 0, C.byref(nr), None, C.byref(st)))
        return nr.value, st, (time.perf_counter() - t0) * 1e3


def spread(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3),
                max=round(float(max(v)), 3), calls=len(v))


def bench_cloud(ctx, p, reps):
    n = p.shape[0]
    r = Runner(ctx, p)
    rows = []
    for mean_k in MEAN_KS:
        r.call(mean_k)  # warm: allocations, code objects, hipcub's choices
        dev, wall = [], []
        for _ in range(reps):
            removed, st, w = r.call(mean_k)
            dev.append(st.device_ms)
            wall.append(w)
        row = dict(n=n, mean_k=mean_k, removed=int(removed), device_ms=spread(dev),
                   wall_ms=spread(wall), literal_queries=int(st.literal_queries),
                   exact_sums=int(st.exact_sums), n_valid=int(st.n_valid),
                   threshold=st.threshold)
        print(json.dumps(row), flush=True)
        rows.append(row)
    cl = D.Cloud(ctx, p)
    cl.estimate_normals(k=20)
    ctx.synchronize()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        cl.estimate_normals(k=20)
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    cl.close()
    nrm = dict(n=n, k=20, wall_ms=spread(wall))
    print(json.dumps(dict(normals_k20=nrm)), flush=True)
    d20 = rows[0]["device_ms"]["median"]
    # the normals call reports no event time: the two ratios name the clocks they divide (the
    # SOR wall time carries the host copies in and out, the normals' wall time has none)
    return dict(n=n, sor=rows, normals_k20=nrm,
                sor20_device_over_normals20_wall=round(d20 / nrm["wall_ms"]["median"], 3),
                sor20_wall_over_normals20_wall=round(
                    rows[0]["wall_ms"]["median"] / nrm["wall_ms"]["median"], 3),
                growth_20_to_150_device=round(rows[-1]["device_ms"]["median"] / d20, 3))


def kernel_kind(name):
    m = re.search(r"dlg::\(anonymous namespace\)::(k_\w+)", name)
    if m:
        return m.group(1)
    for needle, kind in (("histogram", "rocprim radix sort: histogram"),
                         ("onesweep", "rocprim radix sort: onesweep pass"),
                         ("partition", "rocprim partition (DeviceSelect)"),
                         ("scan", "rocprim scan"), ("init_", "rocprim state init"),
                         ("transform", "rocprim transform"), ("fillBuffer", "runtime fill (memset)"),
                         ("copyBuffer", "runtime copy")):
        if needle in name:
            return kind
    return name[:60]


def kernel_split(path):
    """rocprofv3's kernel_stats.csv of a --trace run, kernels of the same kind summed"""
    agg = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            a = agg.setdefault(kernel_kind(r["Name"]), [0, 0.0])
            a[0] += int(r["Calls"])
            a[1] += float(r["TotalDurationNs"]) / 1e6
    tot = sum(a[1] for a in agg.values())
    kernels = [dict(kernel=k, calls=a[0], total_ms=round(a[1], 3), pct=round(100 * a[1] / tot, 2))
               for k, a in sorted(agg.items(), key=lambda kv: -kv[1][1])]
    return dict(note="one rocprofv3 --kernel-trace --stats run of its own (--trace): 1M points, "
                     "two calls each at mean_k 20 and 150; kernels of a kind summed",
                total_kernel_ms=round(tot, 3), kernels=kernels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="one 1M sequence (run under rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv to fold in")
    a = ap.parse_args()
    base, _, _ = config_cloud(3)
    ctx = D.Context(0)
    ctx.set_profiling(True)
    if a.trace:
        r = Runner(ctx, outlier_cloud(base, 1_000_000))
        for mean_k in (20, 150):
            for _ in range(2):
                r.call(mean_k)
        ctx.close()
        return
    res = dict(tool="tools/bench_sor.py", cloud="C3 prefix, the last 5 % replaced by uniform "
               "outliers over the bounding box", results=[])
    for n in [int(v) for v in a.sizes.split(",") if v]:
        res["results"].append(bench_cloud(ctx, outlier_cloud(base, n), a.reps))
    if a.kernel_stats:
        res["kernel_split_1M"] = kernel_split(a.kernel_stats)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({"done": True, "out": a.out}))


if __name__ == "__main__":
    main()
