"""Gaussian-sphere (normal-space Hough) plane seeds (Dialog/PlaneDetect.h:667-1015): the reference's
createPS -> voteForPS -> filtPS -> createGradientField -> rectifySinkFields -> segmentPlanes.  Runs in
libdialog_amd.so (dlg_gs_space, dlg_gs_vote, dlg_gs_segment, dlg_cloud_gs_segment); no CPU path for
the vote, the filter and the seed planes."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .sac import Cloud, Context, _f32p, _i32p, _points, default_context

_i64p = C.POINTER(C.c_int64)


def gauss_sphere_params(**kw) -> _lib.GsParams:
    """dlg_gs_params with the reference's config.txt values, fields overridden by keyword."""
    p = _lib.GsParams()
    _lib.load().dlg_gs_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(_lib.GsParams._fields_):
            raise TypeError(f"unknown parameter {k}")
        setattr(p, k, v)
    return p


def _params(params) -> _lib.GsParams:
    if isinstance(params, _lib.GsParams):
        return params
    return gauss_sphere_params(**(params or {}))


def _stats(st) -> dict:
    return {k: getattr(st, k) for k, _ in _lib.GsStats._fields_}


def gauss_sphere_space(params=None, corners: bool = True):
    """createPS on the host: -> the PS cells' min corners float32 [cells,3] in PS order (or their
    number with corners=False)."""
    prm = _params(params)
    L = _lib.load()
    n = C.c_int64(0)
    _lib.check(L.dlg_gs_space(C.byref(prm), None, 0, C.byref(n)))
    if not corners:
        return int(n.value)
    out = np.empty((max(n.value, 1), 3), np.float32)
    _lib.check(L.dlg_gs_space(C.byref(prm), _f32p(out), n.value, C.byref(n)))
    return out[:n.value].copy()


def _normals(normals, n=None):
    a = np.ascontiguousarray(normals, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("normals must be float32 [N,>=3]")
    if n is not None and a.shape[0] != n:
        raise ValueError("one normal per point")
    return a


def gauss_sphere_vote(normals, params=None, ctx: Context | None = None,
                      return_stats: bool = False):
    """voteForPS (dlg_gs_vote): -> (cell_of_point int32 [n]: the PS cell of each normal, -1 for a
    non-finite one; votes int32 [cells]) [, stats dict]."""
    ctx = ctx or default_context()
    prm = _params(params)
    a = _normals(normals)
    n = a.shape[0]
    L = _lib.load()
    cell = np.empty(max(n, 1), np.int32)
    st = _lib.GsStats()
    votes = np.empty(1, np.int32)
    while True:
        s = L.dlg_gs_vote(ctx.h, _f32p(a), n, 4 * a.shape[1], C.byref(prm), _i32p(cell),
                          _i32p(votes), votes.size, C.byref(st))
        if s == _lib.DLG_ERR_CAPACITY and st.n_cells > votes.size:
            votes = np.empty(st.n_cells, np.int32)
            continue
        ctx.check(s)
        break
    res = (cell[:n].copy(), votes[:st.n_cells].copy())
    return res + (_stats(st),) if return_stats else res


def _segment(call, n, debug, return_stats):
    """runs call(result, stats) with buffers grown to the sizes it reports"""
    off = np.empty(max(n, 1) + 1, np.int64)
    ids = np.empty(max(n, 1), np.int32)
    cell = np.empty(max(n, 1), np.int32)
    cap_s, cap_c = 64, 0
    st = _lib.GsStats()
    while True:
        sc = np.empty(cap_s, np.int32)
        sv = np.empty(cap_s, np.int64)
        dbg = [np.empty(max(cap_c, 1), np.int32) for _ in range(4)] if debug else None
        r = _lib.GsResult()
        r.plane_offsets = off.ctypes.data_as(_i64p)
        r.planes_cap = off.size - 1
        r.plane_ids = _i32p(ids)
        r.ids_cap = ids.size
        r.sink_cells = _i32p(sc)
        r.sink_votes = sv.ctypes.data_as(_i64p)
        r.sinks_cap = cap_s
        r.cell_of_point = _i32p(cell)
        if debug:
            r.raw_vote, r.filtered_vote, r.sink_init, r.sink = (_i32p(d) for d in dbg)
            r.cells_cap = cap_c
        s = call(r, st)
        if s == _lib.DLG_ERR_CAPACITY and (r.n_cells > cap_c and debug or r.n_sinks > cap_s):
            cap_c = max(cap_c, r.n_cells) if debug else 0
            cap_s = max(cap_s, r.n_sinks)
            continue
        break
    out = dict(status=s)
    if s == _lib.DLG_OK:
        k = r.n_planes
        out.update(plane_offsets=off[:k + 1].copy(), plane_ids=ids[:r.n_ids].copy(),
                   sink_cells=sc[:r.n_sinks].copy(), sink_votes=sv[:r.n_sinks].copy(),
                   cell_of_point=cell[:n].copy(), n_cells=int(r.n_cells))
        if debug:
            for name, d in zip(("raw_vote", "filtered_vote", "sink_init", "sink"), dbg):
                out[name] = d[:r.n_cells].copy()
        if return_stats:
            out["stats"] = _stats(st)
    return out


def planes_of(result) -> list:
    """the planes of a segmentation result as a list of int32 index arrays"""
    off, ids = result["plane_offsets"], result["plane_ids"]
    return [ids[off[k]:off[k + 1]] for k in range(len(off) - 1)]


def gauss_sphere_segment(points, normals, params=None, ctx: Context | None = None,
                         debug: bool = False, return_stats: bool = False) -> dict:
    """The seed planes of a cloud with normals (dlg_gs_segment).  -> dict: plane_offsets int64
    [planes+1] and plane_ids int32 (plane k = plane_ids[offsets[k]:offsets[k+1]], distinct cloud
    indices in the reference's order), sink_cells int32 / sink_votes int64 (the kept sinks),
    cell_of_point int32 [n], n_cells; debug=True adds the per-cell raw_vote, filtered_vote,
    sink_init and sink; return_stats=True adds stats."""
    ctx = ctx or default_context()
    prm = _params(params)
    a, pts = _points(points)
    nr = _normals(normals, a.shape[0])
    L = _lib.load()

    def call(r, st):
        return L.dlg_gs_segment(ctx.h, C.byref(pts), _f32p(nr), 4 * nr.shape[1], C.byref(prm),
                                C.byref(r), C.byref(st))

    out = _segment(call, a.shape[0], debug, return_stats)
    ctx.check(out.pop("status"))
    return out


def cloud_gauss_sphere_segment(cloud: Cloud, params=None, debug: bool = False,
                               return_stats: bool = False) -> dict:
    """gauss_sphere_segment of every point of a device-resident cloud with its attached normals
    (Cloud.set_normals / estimate_normals / regulate_normals): normals -> RegulateNormal -> seeds
    with no host round trip on the input side (dlg_cloud_gs_segment)."""
    ctx = cloud.ctx
    prm = _params(params)
    L = _lib.load()

    def call(r, st):
        return L.dlg_cloud_gs_segment(ctx.h, cloud.h, C.byref(prm), C.byref(r), C.byref(st))

    out = _segment(call, cloud.n, debug, return_stats)
    ctx.check(out.pop("status"))
    return out
