"""Rigid registration (Dialog/PCLViewer.cpp:581-636, on_registrationICPAction_triggered):
pcl::IterativeClosestPoint<PointXYZ, PointXYZ> on the GPU, and the SAC-IA initial alignment before it
(Dialog/PCLViewer.cpp:546-558): pcl::SampleConsensusInitialAlignment over FPFH descriptors.  Runs
in libdialog_amd.so (dlg_icp_align, dlg_icp_correspondences, dlg_sac_ia_align, dlg_sac_ia_score,
dlg_fpfh_knn); no CPU path."""
from __future__ import annotations

import ctypes as C
import math
import sys

import numpy as np

from . import _lib
from .sac import Context, _f32p, _i32p, _points, default_context

DBL_MAX = sys.float_info.max
ICP_STATES = ("NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES")


def _mat(m):
    if m is None:
        return None
    a = np.ascontiguousarray(m, dtype=np.float32)
    if a.size != 16:
        raise ValueError("a transformation is a 4x4 matrix")
    return a.reshape(16)


def _index(indices):
    return None if indices is None else np.ascontiguousarray(indices, dtype=np.int32)


def icp_align(source, target, guess=None, indices=None, max_iterations: int = 10,
              max_correspondence_distance: float = math.sqrt(DBL_MAX),
              transformation_epsilon: float = 0.0, euclidean_fitness_epsilon: float = -DBL_MAX,
              fitness_max_range: float | None = None, ctx: Context | None = None,
              return_history: bool = False, return_stats: bool = False):
    """IterativeClosestPoint::align(output, guess) (dlg_icp_align): the listed source points
    (indices: setIndices, any order, duplicates allowed) registered to the target.
    -> (final float32 [4,4], aligned float32 [m,3]) [, history: a list of dict(n_corr, mse, e, e2,
    T float32 [4,4]), one per iteration] [, stats dict].  fitness_max_range not None:
    stats["fitness"] = getFitnessScore(fitness_max_range)."""
    ctx = ctx or default_context()
    a, src = _points(source)
    b, tgt = _points(target)
    idx = _index(indices)
    n = a.shape[0] if idx is None else idx.shape[0]
    prm = _lib.IcpParams(int(max_iterations), int(fitness_max_range is not None),
                         float(max_correspondence_distance), float(transformation_epsilon),
                         float(euclidean_fitness_epsilon),
                         DBL_MAX if fitness_max_range is None else float(fitness_max_range))
    g = _mat(guess)
    final = np.empty(16, np.float32)
    out = np.empty((max(n, 1), 3), np.float32)
    cap = max(int(max_iterations), 1) if return_history else 0
    hist = (_lib.IcpIteration * max(cap, 1))()
    st = _lib.IcpStats()
    ctx.check(_lib.load().dlg_icp_align(
        ctx.h, C.byref(src), None if idx is None else _i32p(idx), n if idx is not None else 0,
        C.byref(tgt), C.byref(prm), None if g is None else _f32p(g), _f32p(final), _f32p(out), 12,
        hist if return_history else None, cap, C.byref(st)))
    res = (final.reshape(4, 4), out[:n].copy())
    if return_history:
        res += ([dict(n_corr=h.n_corr, mse=h.mse, e=h.e, e2=h.e2,
                      T=np.array(h.T, np.float32).reshape(4, 4))
                 for h in hist[:min(st.iterations, cap)]],)
    if return_stats:
        d = {k: getattr(st, k) for k, _ in _lib.IcpStats._fields_}
        d["state_name"] = ICP_STATES[st.state]
        res += (d,)
    return res


def icp_correspondences(source, target, transform=None, indices=None,
                        max_dist: float = math.sqrt(DBL_MAX), ctx: Context | None = None):
    """CorrespondenceEstimation::determineCorrespondences (dlg_icp_correspondences), by the kernel
    the iteration runs: -> (nn int32 [m]: the target index, -1 for a dropped or non-finite entry,
    d2 float32 [m]: the squared distance, 0 where nn is -1)."""
    ctx = ctx or default_context()
    a, src = _points(source)
    b, tgt = _points(target)
    idx = _index(indices)
    n = a.shape[0] if idx is None else idx.shape[0]
    t = _mat(transform)
    nn = np.empty(max(n, 1), np.int32)
    d2 = np.empty(max(n, 1), np.float32)
    k = C.c_int64(0)
    ctx.check(_lib.load().dlg_icp_correspondences(
        ctx.h, C.byref(src), None if idx is None else _i32p(idx), n if idx is not None else 0,
        C.byref(tgt), None if t is None else _f32p(t), float(max_dist), _i32p(nn), _f32p(d2),
        C.byref(k)))
    return nn[:n].copy(), d2[:n].copy()


# ---- SAC-IA -----------------------------------------------------------------------------------
RNG_GLIBC, RNG_MSVC = 0, 1
_HYP_INT = ("valid", "relaxations", "draws", "err_hi", "err_lo", "n_far", "n_used")


def _rows(features, what):
    a = np.ascontiguousarray(features, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 33:
        raise ValueError(f"{what}: one row of 33 floats per point")
    return a


def _hypothesis(h):
    d = {k: int(getattr(h, k)) for k in _HYP_INT}
    d["sample"] = np.array(h.sample, np.int32)
    d["match"] = np.array(h.match, np.int32)
    d["rank"] = np.array(h.rank, np.int32)
    d["T"] = np.array(h.T, np.float32).reshape(4, 4)
    d["E"] = (d["err_hi"] << 24) + d["err_lo"]
    return d


def fpfh_knn(queries, rows, k: int, ctx: Context | None = None):
    """KdTreeFLANN<FPFHSignature33>::nearestKSearch (dlg_fpfh_knn): the k nearest rows with 33
    finite values of every query, in (d, index) order -> (idx int32 [nq, k], d float32 [nq, k]);
    -1 and 0 for a query with a non-finite value."""
    ctx = ctx or default_context()
    q, r = _rows(queries, "queries"), _rows(rows, "rows")
    nq = q.shape[0]
    idx = np.empty((max(nq, 1), k), np.int32)
    d = np.empty((max(nq, 1), k), np.float32)
    ctx.check(_lib.load().dlg_fpfh_knn(ctx.h, _f32p(q), q.strides[0], nq, _f32p(r), r.strides[0],
                                       r.shape[0], int(k), _i32p(idx), _f32p(d)))
    return idx[:nq].copy(), d[:nq].copy()


def sac_ia_score(source, target, transforms, max_correspondence_distance: float = math.sqrt(DBL_MAX),
                 batch: int = 0, max_blocks: int = 0, ctx: Context | None = None):
    """computeErrorMetric of the given transformations (dlg_sac_ia_score) -> a list of dict(T, E (a
    Python integer: the sum of trunc(term 2^48)), err_hi, err_lo, n_far, n_used, ...)."""
    ctx = ctx or default_context()
    a, src = _points(source)
    b, tgt = _points(target)
    t = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 16)
    hyp = (_lib.SacIaHypothesis * max(len(t), 1))()
    ctx.check(_lib.load().dlg_sac_ia_score(ctx.h, C.byref(src), C.byref(tgt), _f32p(t), len(t),
                                           float(max_correspondence_distance), int(batch),
                                           int(max_blocks), hyp))
    return [_hypothesis(h) for h in hyp[:len(t)]]


def sac_ia_align(source, source_features, target, target_features, guess=None,
                 max_iterations: int = 1000, nr_samples: int = 3, k_correspondences: int = 10,
                 min_sample_distance: float = 0.0,
                 max_correspondence_distance: float = math.sqrt(DBL_MAX), rng: int = RNG_GLIBC,
                 seed: int = 1, fitness_max_range: float | None = None, batch: int = 0,
                 max_blocks: int = 0, ctx: Context | None = None, return_hypotheses: bool = False,
                 return_stats: bool = False):
    """SampleConsensusInitialAlignment::align(output, guess) (dlg_sac_ia_align) over FPFH rows
    (fpfh_estimation's output).  -> (final float32 [4,4], aligned float32 [n,3]) [, hypotheses: a
    list of dict, one per iteration] [, stats dict].  fitness_max_range not None:
    stats["fitness"] = getFitnessScore(fitness_max_range)."""
    ctx = ctx or default_context()
    a, src = _points(source)
    b, tgt = _points(target)
    fa, fb = _rows(source_features, "source_features"), _rows(target_features, "target_features")
    if fa.shape[0] != a.shape[0] or fb.shape[0] != b.shape[0]:
        raise ValueError("one descriptor row per point")
    n = a.shape[0]
    prm = _lib.SacIaParams(int(max_iterations), int(nr_samples), int(k_correspondences), int(rng),
                           int(seed), int(fitness_max_range is not None), int(batch),
                           int(max_blocks), float(min_sample_distance),
                           float(max_correspondence_distance),
                           DBL_MAX if fitness_max_range is None else float(fitness_max_range))
    g = _mat(guess)
    final = np.empty(16, np.float32)
    out = np.empty((max(n, 1), 3), np.float32)
    cap = max(int(max_iterations), 1) if return_hypotheses else 0
    hyp = (_lib.SacIaHypothesis * max(cap, 1))()
    st = _lib.SacIaStats()
    ctx.check(_lib.load().dlg_sac_ia_align(
        ctx.h, C.byref(src), _f32p(fa), fa.strides[0], C.byref(tgt), _f32p(fb), fb.strides[0],
        C.byref(prm), None if g is None else _f32p(g), _f32p(final), _f32p(out), 12,
        hyp if return_hypotheses else None, cap, C.byref(st)))
    res = (final.reshape(4, 4), out[:n].copy())
    if return_hypotheses:
        res += ([_hypothesis(h) for h in hyp[:min(st.iterations, cap)]],)
    if return_stats:
        res += ({k: getattr(st, k) for k, _ in _lib.SacIaStats._fields_ if k != "reserved"},)
    return res
