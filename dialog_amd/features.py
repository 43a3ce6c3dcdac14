"""pcl::FPFHEstimation<PointXYZ, Normal, FPFHSignature33> on the GPU (Dialog/PCLViewer.cpp:524-543,
the descriptors SampleConsensusInitialAlignment consumes).  Runs in libdialog_amd.so
(dlg_fpfh_estimate, dlg_cloud_fpfh); no CPU path."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .sac import Cloud, Context, _f32p, _i32p, _points, default_context

FPFH_DIM = 33


def _stats(st):
    return {k: getattr(st, k) for k, _ in _lib.FpfhStats._fields_}


def fpfh_estimation(points, normals, radius: float, indices=None, ctx: Context | None = None,
                    return_counts: bool = False, return_stats: bool = False):
    """FPFHEstimation::compute with setRadiusSearch(radius), the search surface being `points`
    itself.  normals: float32 [N,3], [N,4] or [N,8] (nx, ny, nz first), one per point.  indices:
    setIndices (any order, duplicates allowed); the neighbours and their SPFHs come from the whole
    cloud either way.  -> (hist float32 [n,33]: one descriptor per list entry, NaN for a non-finite
    entry, zeros for an entry with no neighbour but itself; neighbours int32 [n]: each entry's
    neighbour count, itself included, -1 for a non-finite entry) [, spfh_counts int32 [N,33]: the
    integer bin counts of every finite point's SPFH] [, stats dict]."""
    ctx = ctx or default_context()
    a, pts = _points(points)
    nr = np.ascontiguousarray(normals, dtype=np.float32)
    if nr.ndim != 2 or nr.shape[1] < 3 or nr.shape[0] != a.shape[0]:
        raise ValueError("normals must be float32 [N,3+], one row per point")
    idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.int32)
    n = a.shape[0] if idx is None else idx.shape[0]
    hist = np.empty((max(n, 1), FPFH_DIM), np.float32)
    nb = np.empty(max(n, 1), np.int32)
    counts = np.zeros((max(a.shape[0], 1), FPFH_DIM), np.int32) if return_counts else None
    prm = _lib.FpfhParams(float(radius))
    st = _lib.FpfhStats()
    ctx.check(_lib.load().dlg_fpfh_estimate(
        ctx.h, C.byref(pts), _f32p(nr), 4 * nr.shape[1], None if idx is None else _i32p(idx),
        n if idx is not None else 0, C.byref(prm), _f32p(hist), 4 * FPFH_DIM, _i32p(nb),
        _i32p(counts) if return_counts else None, C.byref(st)))
    res = (hist[:n].copy(), nb[:n].copy())
    if return_counts:
        res += (counts[:a.shape[0]].copy(),)
    return res + (_stats(st),) if return_stats else res


def cloud_fpfh(cloud: Cloud, radius: float, return_stats: bool = False):
    """fpfh_estimation of every point of a device-resident cloud with its attached normals
    (Cloud.set_normals / estimate_normals / regulate_normals): upload -> normals -> FPFH with no host
    round trip on the input side (dlg_cloud_fpfh).  -> (hist float32 [n,33], neighbours int32 [n])
    [, stats dict]."""
    ctx = cloud.ctx
    n = cloud.n
    hist = np.empty((max(n, 1), FPFH_DIM), np.float32)
    nb = np.empty(max(n, 1), np.int32)
    prm = _lib.FpfhParams(float(radius))
    st = _lib.FpfhStats()
    ctx.check(_lib.load().dlg_cloud_fpfh(ctx.h, cloud.h, C.byref(prm), _f32p(hist), 4 * FPFH_DIM,
                                         _i32p(nb), C.byref(st)))
    res = (hist[:n].copy(), nb[:n].copy())
    return res + (_stats(st),) if return_stats else res
