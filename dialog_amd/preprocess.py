"""preProcess() / removeRedundantPoints on the GPU (Dialog/PlaneDetect.h:448-512,
PCLViewer.cpp:781-805): NaN removal, translation to the centroid, redundancy removal with the
radius min_dist_between_points.  Runs in libdialog_amd.so (dlg_preprocess); no CPU path."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .sac import Cloud, Context, _f32p, _i32p, _points, default_context


def preprocess(points, min_dist: float, translate: bool = True, ctx: Context | None = None):
    """-> (kept float32 [k,3] (translated when `translate`), input indices int32 [k],
    translation float32 [3])."""
    ctx = ctx or default_context()
    a, pts = _points(points)
    n = a.shape[0]
    out = np.empty((max(n, 1), 3), np.float32)
    idx = np.empty(max(n, 1), np.int32)
    tr = np.zeros(3, np.float32)
    k = C.c_int64(0)
    ctx.check(_lib.load().dlg_preprocess(ctx.h, C.byref(pts), int(bool(translate)),
                                         float(min_dist), _f32p(out), 12, _i32p(idx), n,
                                         C.byref(k), _f32p(tr)))
    return out[:k.value].copy(), idx[:k.value].copy(), tr


def _voxel_args(points, leaf, indices, min_points):
    a, pts = _points(points)
    lf = np.broadcast_to(np.asarray(leaf, np.float32), (3,))
    prm = _lib.VoxelParams((C.c_float * 3)(*[float(v) for v in lf]), int(min_points))
    idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.int32)
    n = a.shape[0] if idx is None else idx.shape[0]
    return a, pts, prm, idx, n


def _voxel_stats(st):
    return dict(n_finite=st.n_finite, n_voxels=st.n_voxels, div=np.array(st.div[:], np.int32),
                min_b=np.array(st.min_b[:], np.int32), device_ms=st.device_ms)


def voxel_grid(points, leaf, indices=None, min_points: int = 0, ctx: Context | None = None,
               return_stats: bool = False):
    """pcl::VoxelGrid<PointXYZ>::filter on the GPU (dlg_voxel_grid; PCLViewer.cpp:313-332): one
    centroid per occupied voxel of edge lengths `leaf` (a scalar or 3 values), in key order.
    indices: setIndices (any order, duplicates allowed); min_points:
    setMinimumPointsNumberPerVoxel.  -> (xyz float32 [k,3], counts int32 [k], voxel_of_entry
    int32 [n]: the output row of each list entry, -1 for a non-finite entry or a dropped voxel)
    [, stats dict].  A leaf too small for 32-bit voxel indices raises DialogError (status 1)."""
    ctx = ctx or default_context()
    a, pts, prm, idx, n = _voxel_args(points, leaf, indices, min_points)
    out = np.empty((max(n, 1), 3), np.float32)
    cnt = np.empty(max(n, 1), np.int32)
    voe = np.empty(max(n, 1), np.int32)
    k = C.c_int64(0)
    st = _lib.VoxelStats()
    ctx.check(_lib.load().dlg_voxel_grid(ctx.h, C.byref(pts), None if idx is None else _i32p(idx),
                                         n if idx is not None else 0, C.byref(prm), _f32p(out), 12,
                                         n, C.byref(k), _i32p(cnt), _i32p(voe), C.byref(st)))
    res = (out[:k.value].copy(), cnt[:k.value].copy(), voe[:n].copy())
    return res + (_voxel_stats(st),) if return_stats else res


def voxel_grid_cloud(points, leaf, indices=None, min_points: int = 0, id_base: int = 0,
                     ctx: Context | None = None, return_stats: bool = False):
    """voxel_grid with the result left on the device (dlg_voxel_grid_cloud): -> (Cloud,
    voxel_of_entry int32 [n]) [, stats dict].  The Cloud equals Cloud(ctx, xyz, id_base=id_base) of
    the points voxel_grid returns, so normals and planes run on it with no host round trip."""
    ctx = ctx or default_context()
    a, pts, prm, idx, n = _voxel_args(points, leaf, indices, min_points)
    voe = np.empty(max(n, 1), np.int32)
    k = C.c_int64(0)
    h = C.c_void_p()
    st = _lib.VoxelStats()
    ctx.check(_lib.load().dlg_voxel_grid_cloud(ctx.h, C.byref(pts),
                                               None if idx is None else _i32p(idx),
                                               n if idx is not None else 0, C.byref(prm),
                                               int(id_base), C.byref(h), C.byref(k), _i32p(voe),
                                               C.byref(st)))
    res = (Cloud._from_handle(ctx, h, k.value), voe[:n].copy())
    return res + (_voxel_stats(st),) if return_stats else res


def _sor_args(points, mean_k, stddev_mul, indices, negative):
    a, pts = _points(points)
    prm = _lib.SorParams(int(mean_k), int(bool(negative)), float(stddev_mul))
    idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.int32)
    n = a.shape[0] if idx is None else idx.shape[0]
    return a, pts, prm, idx, n


def _sor_stats(st):
    return {k: getattr(st, k) for k, _ in _lib.SorStats._fields_}


def statistical_outlier_removal(points, mean_k: int, stddev_mul: float, indices=None,
                                negative: bool = False, ctx: Context | None = None,
                                return_stats: bool = False):
    """pcl::StatisticalOutlierRemoval<PointXYZ>::filter on the GPU
    (dlg_statistical_outlier_removal; PCLViewer.cpp:334-358): an entry is removed when the mean
    distance to its mean_k nearest neighbours exceeds mean + stddev_mul * stddev of those means
    (negative: when it does not).  indices: setIndices (any order, duplicates allowed); the
    neighbours come from the whole cloud either way.  -> (kept int32 [k], removed int32 [r]: index
    values in list order, distances float32 [n]: one per list entry) [, stats dict].  Fewer than
    mean_k + 1 finite points raise DialogError (status 1)."""
    ctx = ctx or default_context()
    a, pts, prm, idx, n = _sor_args(points, mean_k, stddev_mul, indices, negative)
    kept = np.empty(max(n, 1), np.int32)
    rem = np.empty(max(n, 1), np.int32)
    dist = np.empty(max(n, 1), np.float32)
    nk, nr = C.c_int64(0), C.c_int64(0)
    st = _lib.SorStats()
    ctx.check(_lib.load().dlg_statistical_outlier_removal(
        ctx.h, C.byref(pts), None if idx is None else _i32p(idx), n if idx is not None else 0,
        C.byref(prm), _i32p(kept), n, C.byref(nk), _i32p(rem), n, C.byref(nr), _f32p(dist),
        C.byref(st)))
    res = (kept[:nk.value].copy(), rem[:nr.value].copy(), dist[:n].copy())
    return res + (_sor_stats(st),) if return_stats else res


def statistical_outlier_removal_cloud(points, mean_k: int, stddev_mul: float, indices=None,
                                      negative: bool = False, id_base: int = 0,
                                      ctx: Context | None = None, return_stats: bool = False):
    """statistical_outlier_removal with the kept points left on the device
    (dlg_statistical_outlier_removal_cloud): -> (Cloud, kept int32 [k]) [, stats dict].  The Cloud
    equals Cloud(ctx, points[kept], id_base=id_base)."""
    ctx = ctx or default_context()
    a, pts, prm, idx, n = _sor_args(points, mean_k, stddev_mul, indices, negative)
    kept = np.empty(max(n, 1), np.int32)
    k = C.c_int64(0)
    h = C.c_void_p()
    st = _lib.SorStats()
    ctx.check(_lib.load().dlg_statistical_outlier_removal_cloud(
        ctx.h, C.byref(pts), None if idx is None else _i32p(idx), n if idx is not None else 0,
        C.byref(prm), int(id_base), C.byref(h), C.byref(k), _i32p(kept), C.byref(st)))
    res = (Cloud._from_handle(ctx, h, k.value), kept[:k.value].copy())
    return res + (_sor_stats(st),) if return_stats else res


def _mls_args(points, radius, order, polynomial_fit, compute_normals, sqr_gauss_param, indices):
    a, pts = _points(points)
    prm = _lib.MlsParams(float(radius), int(bool(polynomial_fit)), int(order),
                         int(bool(compute_normals)), float(sqr_gauss_param))
    idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.int32)
    n = a.shape[0] if idx is None else idx.shape[0]
    return a, pts, prm, idx, n


def _mls_stats(st):
    return {k: getattr(st, k) for k, _ in _lib.MlsStats._fields_}


def moving_least_squares(points, radius: float, order: int = 2, polynomial_fit: bool = True,
                         compute_normals: bool = True, sqr_gauss_param: float = 0.0, indices=None,
                         ctx: Context | None = None, return_stats: bool = False):
    """pcl::MovingLeastSquares<PointXYZ, PointNormal>::process on the GPU (dlg_moving_least_squares;
    PCLViewer.cpp:387-423, "rebuild plane"): every list entry projected onto the polynomial surface
    of degree `order` fitted to its neighbours within `radius` (polynomial_fit off, or fewer
    neighbours than coefficients: onto their plane).  indices: setIndices (any order, duplicates
    allowed); the neighbours come from the whole cloud either way.  sqr_gauss_param <= 0: radius^2.
    -> (xyz float32 [k,3], normals float32 [k,4]: nx, ny, nz (not normalised, as PCL 1.8) and
    curvature, zeros when compute_normals is off, src_index int32 [k]: each row's index value,
    neighbours int32 [n]: one per list entry, -1 for a non-finite entry) [, stats dict].  Entries
    that are not finite or have fewer than 3 neighbours give no row."""
    ctx = ctx or default_context()
    a, pts, prm, idx, n = _mls_args(points, radius, order, polynomial_fit, compute_normals,
                                    sqr_gauss_param, indices)
    out = np.empty((max(n, 1), 3), np.float32)
    nrm = np.empty((max(n, 1), 4), np.float32)
    src = np.empty(max(n, 1), np.int32)
    nb = np.empty(max(n, 1), np.int32)
    k = C.c_int64(0)
    st = _lib.MlsStats()
    ctx.check(_lib.load().dlg_moving_least_squares(
        ctx.h, C.byref(pts), None if idx is None else _i32p(idx), n if idx is not None else 0,
        C.byref(prm), _f32p(out), 12, _f32p(nrm), n, C.byref(k), _i32p(src), _i32p(nb),
        C.byref(st)))
    res = (out[:k.value].copy(), nrm[:k.value].copy(), src[:k.value].copy(), nb[:n].copy())
    return res + (_mls_stats(st),) if return_stats else res


def moving_least_squares_cloud(points, radius: float, order: int = 2, polynomial_fit: bool = True,
                               compute_normals: bool = True, sqr_gauss_param: float = 0.0,
                               indices=None, id_base: int = 0, ctx: Context | None = None,
                               return_stats: bool = False):
    """moving_least_squares with the smoothed points left on the device
    (dlg_moving_least_squares_cloud): -> (Cloud, src_index int32 [k]) [, stats dict].  The Cloud
    equals Cloud(ctx, xyz, id_base=id_base) of the rows moving_least_squares returns, with their
    normals attached when compute_normals is on, so planes run on it with no host round trip."""
    ctx = ctx or default_context()
    a, pts, prm, idx, n = _mls_args(points, radius, order, polynomial_fit, compute_normals,
                                    sqr_gauss_param, indices)
    src = np.empty(max(n, 1), np.int32)
    k = C.c_int64(0)
    h = C.c_void_p()
    st = _lib.MlsStats()
    ctx.check(_lib.load().dlg_moving_least_squares_cloud(
        ctx.h, C.byref(pts), None if idx is None else _i32p(idx), n if idx is not None else 0,
        C.byref(prm), int(id_base), C.byref(h), C.byref(k), _i32p(src), C.byref(st)))
    res = (Cloud._from_handle(ctx, h, k.value), src[:k.value].copy())
    return res + (_mls_stats(st),) if return_stats else res


def remove_redundant_points(points, min_dist: float, ctx: Context | None = None):
    """on_removeRedundantPointsAction_triggered (PCLViewer.cpp:781-805): -> kept indices."""
    _, idx, _ = preprocess(points, min_dist, translate=False, ctx=ctx)
    return idx
