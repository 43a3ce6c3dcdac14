"""Voxel-grid filter timing (dlg_voxel_grid): the C3 (10M points) and C4 (100M) clouds at leaf 0.02,
0.05 and 0.2, warm calls with profiling on.

Per (cloud, leaf): device ms per call over --reps calls (median, min, max: HIP events from the
first kernel to the last, host copies excluded), wall ms per call (host buffers in and out, as the
C ABI takes them), the algorithmic bytes against the measured HBM peak, the time of a plain
single-threaded C++ loop on this host (tools/voxel_host_loop.cpp: a restatement, not PCL), and
whether the device's output bits equal that loop's.  Also: the DLG_OPT_VOXEL_LONG_RUN cross-over
on the C3 cloud at leaf 0.2 and 1.0, and the worst case (10M points in one voxel).

  python tools/bench_voxel.py [--clouds 3,4] [--reps 10] [--out profiles/r08_voxel.json]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_voxel.py --trace   (one C3 call
      sequence for the per-kernel split; --kernel-stats CSV folds the split into the JSON;
      --extra FILE copies figures the tool does not measure in under 'recorded_by_hand')
"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dialog_amd as D  # noqa: E402
from dialog_amd import _lib  # noqa: E402
from dialog_amd.sac import _f32p, _i32p  # noqa: E402
from dialog_amd.synth import config_cloud  # noqa: E402

HBM_PEAK = 6.29e12  # B/s, measured float4 copy (8.0e12 spec)
LEAVES = (0.02, 0.05, 0.2)
INT32_MAX = 2**31 - 1


def host_loop_lib():
    so = os.path.join(ROOT, "tools", "libvoxel_host_loop.so")
    src = os.path.join(ROOT, "tools", "voxel_host_loop.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src,
                        "-o", so], check=True)
    L = C.CDLL(so)
    L.voxel_host_loop.restype = C.c_int64
    L.voxel_host_loop.argtypes = [C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_float),
                                  C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    return L


class Runner:
    """dlg_voxel_grid on one cloud with buffers allocated once"""

    def __init__(self, ctx, p):
        self.ctx, self.p, self.n = ctx, p, p.shape[0]
        self.pts = _lib.Points(_f32p(p), self.n, 12)
        self.out = np.empty((self.n, 3), np.float32)
        self.cnt = np.empty(self.n, np.int32)
        self.L = _lib.load()

    def call(self, leaf):
        prm = _lib.VoxelParams((C.c_float * 3)(leaf, leaf, leaf), 0)
        k = C.c_int64()
        st = _lib.VoxelStats()
        t0 = time.perf_counter()
        self.ctx.check(self.L.dlg_voxel_grid(self.ctx.h, C.byref(self.pts), None, 0, C.byref(prm),
                                             _f32p(self.out), 12, self.n, C.byref(k),
                                             _i32p(self.cnt), None, C.byref(st)))
        return k.value, st, (time.perf_counter() - t0) * 1e3


def spread(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3),
                max=round(float(max(v)), 3), calls=len(v))


def bench_cloud(ctx, host, name, p, leaves, reps, check):
    r = Runner(ctx, p)
    n = r.n
    rows = []
    for leaf in leaves:
        r.call(leaf)  # warm: allocations, code objects, hipcub's choices
        dev, wall = [], []
        for _ in range(reps):
            k, st, w = r.call(leaf)
            dev.append(st.device_ms)
            wall.append(w)
        bits = 1
        total = int(st.div[0]) * int(st.div[1]) * int(st.div[2])
        while bits < 32 and (1 << bits) < total:
            bits += 1
        passes = (bits + 7) // 8
        # 12 B per point in, the (key, position) pairs read and written once per 8-bit radix
        # pass, 12 B per voxel out
        alg_bytes = 12 * n + 16 * st.n_finite * passes + 12 * k
        row = dict(cloud=name, n=n, leaf=leaf, voxels=int(k), div=list(st.div), key_bits=bits,
                   device_ms=spread(dev), wall_ms=spread(wall), algorithmic_bytes=int(alg_bytes),
                   hbm_floor_ms=round(alg_bytes / HBM_PEAK * 1e3, 3),
                   share_of_hbm_peak=round(alg_bytes / HBM_PEAK * 1e3 / float(np.median(dev)), 4))
        if check:
            ho = np.empty((n, 3), np.float32)
            hc = np.empty(n, np.int32)
            lf = (C.c_float * 3)(leaf, leaf, leaf)
            t0 = time.perf_counter()
            hk = host.voxel_host_loop(_f32p(p), n, lf, _f32p(ho), _i32p(hc))
            row["host_loop_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["bits_equal_host_loop"] = bool(
                hk == k and np.array_equal(ho[:k].view(np.uint32), r.out[:k].view(np.uint32))
                and np.array_equal(hc[:k], r.cnt[:k]))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def crossover(ctx, p, reps):
    r = Runner(ctx, p)
    default = ctx.get_option(D.DLG_OPT_VOXEL_LONG_RUN)
    rows = []
    for leaf in (0.2, 1.0):
        ref = None
        for lr in (1, 8, 16, 32, 64, 128, 256, 1024, 4096, INT32_MAX):
            ctx.set_option(D.DLG_OPT_VOXEL_LONG_RUN, lr)
            r.call(leaf)
            dev = []
            for _ in range(reps):
                k, st, _ = r.call(leaf)
                dev.append(st.device_ms)
            sig = (k, r.out[:k].view(np.uint32).sum(dtype=np.uint64), r.cnt[:k].sum())
            ref = ref or sig
            row = dict(leaf=leaf, long_run=lr, voxels=int(k), max_count=int(r.cnt[:k].max()),
                       device_ms=spread(dev), same_bits=bool(sig == ref))
            print(json.dumps(row), flush=True)
            rows.append(row)
    ctx.set_option(D.DLG_OPT_VOXEL_LONG_RUN, default)
    return rows


def worst_case(ctx, host, n, reps):
    rng = np.random.default_rng(9)
    p = (rng.random((n, 3), dtype=np.float32) + np.float32(1)).astype(np.float32)
    rows = bench_cloud(ctx, host, "one_voxel", p, (100.0,), reps, True)
    assert rows[0]["voxels"] == 1
    return rows[0]


def kernel_kind(name):
    """a rocprofv3 kernel name -> this library's kernel, or the kind of library kernel it is"""
    m = re.search(r"dlg::\(anonymous namespace\)::(k_\w+)\(", name)
    if m:
        return m.group(1)
    for needle, kind in (("histogram", "rocprim radix sort: histogram"),
                         ("onesweep", "rocprim radix sort: onesweep pass"),
                         ("partition", "rocprim partition (DeviceSelect)"),
                         ("wrapped_scan", "rocprim scan (DeviceScan)"),
                         ("init_lookback", "rocprim state init"),
                         ("init_offset", "rocprim state init"),
                         ("transform", "rocprim transform"),
                         ("fillBuffer", "runtime fill (memset)"),
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
    return dict(note="one rocprofv3 --kernel-trace --stats run of its own (--trace): 9 calls on "
                     "the C3 cloud, 3 each at leaf 0.02, 0.05, 0.2; kernels of a kind summed",
                total_kernel_ms=round(tot, 3), kernels=kernels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", default="3,4")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="one C3 sequence (run under rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv to fold in")
    ap.add_argument("--no-host-loop", action="store_true")
    ap.add_argument("--extra", default=None,
                    help="JSON file of figures this tool does not measure (other runs, estimates); "
                         "copied into the output under 'recorded_by_hand'")
    a = ap.parse_args()
    ctx = D.Context(0)
    ctx.set_profiling(True)
    if a.trace:
        p, _, _ = config_cloud(3)
        r = Runner(ctx, p)
        for leaf in LEAVES:
            for _ in range(3):
                r.call(leaf)
        ctx.close()
        return
    host = None if a.no_host_loop else host_loop_lib()
    res = dict(tool="tools/bench_voxel.py", hbm_peak_bytes_per_s=HBM_PEAK,
               default_long_run=ctx.get_option(D.DLG_OPT_VOXEL_LONG_RUN), results=[])
    for cid in [int(v) for v in a.clouds.split(",") if v]:
        p, _, _ = config_cloud(cid)
        p = np.ascontiguousarray(p[:, :3], np.float32)
        res["results"] += bench_cloud(ctx, host, f"C{cid}", p, LEAVES, a.reps, host is not None)
        if cid == 3:
            res["long_run_crossover_C3"] = crossover(ctx, p, max(3, a.reps // 2))
        del p
    if host is not None:
        res["worst_case_one_voxel_10M"] = worst_case(ctx, host, 10_000_000, 3)
    if a.kernel_stats:
        res["kernel_split_C3"] = kernel_split(a.kernel_stats)
    if a.extra:
        with open(a.extra) as f:
            res["recorded_by_hand"] = json.load(f)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({"done": True, "out": a.out}))


if __name__ == "__main__":
    main()
