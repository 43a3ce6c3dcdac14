"""Float64 restatement of the normals path and the exact FLANN neighbour sets it runs on, shared
by tests/test_normals.py and tests/test_knn_normals_gpu.py: independent of the oracle and of the
library (numpy and scipy only)."""
import numpy as np
from scipy.spatial import cKDTree


def flann_radius_sets(p, r):
    """exact KdTreeFLANN radius sets: float d2 = ((0 + dx^2) + dy^2) + dz^2 < float(r*r)."""
    r2 = np.float32(float(r) * float(r))
    tree = cKDTree(p.astype(np.float64))
    cand = tree.query_ball_point(p.astype(np.float64), r * 1.001)
    out = []
    for i, c in enumerate(cand):
        c = np.asarray(c, np.int64)
        d = p[i][None, :] - p[c]
        d2 = ((np.float32(0) + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        out.append(np.sort(c[d2 < r2]))
    return out


def knn_sets(p, k):
    """FLANN kNN sets: the k smallest (float d2, index) among the points (query included)."""
    tree = cKDTree(p.astype(np.float64))
    _, cand = tree.query(p.astype(np.float64), k=min(k + 8, len(p)))
    out = []
    for i, c in enumerate(cand):
        d = p[i][None, :] - p[c]
        d2 = ((np.float32(0) + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        o = np.lexsort((c, d2))[:k]
        out.append(np.sort(c[o]))
    return out


def f64_normals(p, sets, vp=(0.0, 0.0, 0.0)):
    """float64 restatement: covariance, eigh, curvature, viewpoint flip; + eigen-gap quality."""
    n = p.shape[0]
    out = np.full((n, 4), np.nan)
    gap = np.zeros(n)
    P = p.astype(np.float64)
    for i, s in enumerate(sets):
        if len(s) < 3:
            continue
        q = P[s]
        c = np.cov(q.T, bias=True)
        w, v = np.linalg.eigh(c)
        nv = v[:, 0]
        if np.dot(np.asarray(vp) - P[i], nv) < 0:
            nv = -nv
        tr = w.sum()
        out[i, :3] = nv
        out[i, 3] = abs(w[0] / tr) if tr != 0 else 0.0
        gap[i] = (w[1] - w[0]) / max(w[2], 1e-300)
    return out, gap


def angle(a, b):
    """unsigned angle between the lines of two normal sets, robust near 0 (float32 unit vectors
    are only unit to ~6e-8, which arccos of the dot product would turn into ~3e-4 rad)."""
    a = a[:, :3].astype(np.float64)
    b = b[:, :3].astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs(np.sum(a * b, axis=1)))


def same_bits(a, b):
    """bit-equal where b is finite, NaN exactly where b is NaN (a NaN's payload is not pinned)"""
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(b)
    return np.array_equal(a.view(np.uint32)[ok], b.view(np.uint32)[ok])
