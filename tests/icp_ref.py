"""numpy restatement of dlg_icp_align / dlg_icp_correspondences (include/dialog_ransac.h, the
"rigid registration" section; dialog_amd/csrc/icp_model.hpp is the C++ it is compared with).

Brute-force float32 nearest neighbours with FLANN's operation order, Python integers for the
moments, Python floats (IEEE double, + - * / sqrt only) for Horn's closed form with the same cyclic
Jacobi sequence, and the convergence criteria.  Also the case list of tests/golden/icp_small.npz
(make_icp.py writes it, test_icp.py recomputes it, test_icp_gpu.py compares the device with it).
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

f32 = np.float32
DBL_MAX = sys.float_info.max
NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
IDENTITY = np.eye(4, dtype=f32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def transform_points(T, P):
    """x' = ((m00 x + m01 y) + m02 z) + m03 in float32, every operation rounded on its own"""
    T = np.asarray(T, f32).reshape(4, 4)
    P = np.asarray(P, f32)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    out = np.empty_like(P)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    return out


def squared_limit(max_dist):
    md2 = float(max_dist) * float(max_dist)
    return DBL_MAX if md2 > DBL_MAX else md2


def correspondences(W, tgt, max_dist=math.sqrt(DBL_MAX), md2=None):
    """-> (nn int32 [m] (-1: dropped or not finite), d2 float32 [m] (0 where nn = -1))"""
    W = np.asarray(W, f32).reshape(-1, 3)
    tgt = np.asarray(tgt, f32).reshape(-1, 3)
    md2 = squared_limit(max_dist) if md2 is None else md2
    fin_t = np.nonzero(np.isfinite(tgt).all(axis=1))[0]
    tf = tgt[fin_t]
    nn = np.full(len(W), -1, np.int32)
    d2 = np.zeros(len(W), f32)
    fin_w = np.nonzero(np.isfinite(W).all(axis=1))[0]
    step = max(1, (1 << 22) // max(len(tf), 1))
    with np.errstate(all="ignore"):
        for a in range(0, len(fin_w), step):
            ids = fin_w[a:a + step]
            q = W[ids]
            dx = q[:, None, 0] - tf[None, :, 0]
            dy = q[:, None, 1] - tf[None, :, 1]
            dz = q[:, None, 2] - tf[None, :, 2]
            d = ((f32(0) + dx * dx) + dy * dy) + dz * dz
            j = np.argmin(d, axis=1)  # (the first of equal distances: the lowest index)
            dj = d[np.arange(len(ids)), j]
            keep = ~(dj.astype(np.float64) > md2)
            nn[ids[keep]] = fin_t[j[keep]]
            d2[ids[keep]] = dj[keep]
    return nn, d2


# correspondences_fast: a candidate set is certified when the 4th candidate's squared distance (double)
# exceeds the float32 minimum by this relative margin.  A float32 d2 of normal terms carries a few
# 2^-24 (6e-8) of relative error, so the margin is more than 100 x its rounding; below
# FAST_D2_FLOOR the terms may be subnormal, their error is absolute, and nothing is certified.
FAST_MARGIN = 1e-5
FAST_D2_FLOOR = 2.0 ** -100
FAST_K = 4


def correspondences_fast(W, tgt, max_dist=math.sqrt(DBL_MAX), md2=None, info=None):
    """correspondences() with a k-d tree proposing FAST_K candidates per query (double), their d2
    re-evaluated in float32 in FLANN's operation order, the minimum taken with ties to the lowest
    index; every query whose candidate set is not certified (see FAST_MARGIN) is answered by the
    brute force over the whole target.  info (a dict): 'uncertified' = how many went that way."""
    from scipy.spatial import cKDTree
    W = np.asarray(W, f32).reshape(-1, 3)
    tgt = np.asarray(tgt, f32).reshape(-1, 3)
    md2 = squared_limit(max_dist) if md2 is None else md2
    fin_t = np.nonzero(np.isfinite(tgt).all(axis=1))[0]
    tf = tgt[fin_t]
    nn = np.full(len(W), -1, np.int32)
    d2 = np.zeros(len(W), f32)
    fin_w = np.nonzero(np.isfinite(W).all(axis=1))[0]
    slow = fin_w
    if len(tf) > FAST_K and len(fin_w):
        q = W[fin_w]
        dd, cand = cKDTree(tf.astype(np.float64)).query(q.astype(np.float64), k=FAST_K)
        with np.errstate(all="ignore"):
            c = tf[cand]                                        # [m, K, 3] float32
            dx = q[:, None, 0] - c[:, :, 0]
            dy = q[:, None, 1] - c[:, :, 1]
            dz = q[:, None, 2] - c[:, :, 2]
            d = ((f32(0) + dx * dx) + dy * dy) + dz * dz
            dmin = d.min(axis=1)
            # the lowest index among the candidates at the minimum
            j = np.where(d == dmin[:, None], cand, np.iinfo(np.int64).max).min(axis=1)
            fm = dmin.astype(np.float64)
            sure = (fm >= FAST_D2_FLOOR) & np.isfinite(fm) & \
                (dd[:, FAST_K - 1] * dd[:, FAST_K - 1] > fm * (1.0 + FAST_MARGIN))
        keep = sure & ~(fm > md2)
        nn[fin_w[keep]] = fin_t[j[keep]]
        d2[fin_w[keep]] = dmin[keep]
        slow = fin_w[~sure]
    if info is not None:
        info["uncertified"] = info.get("uncertified", 0) + int(len(slow))
        info["queries"] = info.get("queries", 0) + int(len(fin_w))
    if len(slow):
        sn, sd = correspondences(W[slow], tgt, md2=md2)
        nn[slow], d2[slow] = sn, sd
    return nn, d2


def qexp(f):
    f = float(f)
    if not (f > 0.0) or not (f < math.inf):
        return 0
    return math.frexp(f)[1]


def max_abs_finite(P):
    P = np.asarray(P, f32).reshape(-1, 3)
    P = P[np.isfinite(P).all(axis=1)]
    return float(np.abs(P).max()) if len(P) else 0.0


def quantise(v, e):
    """q(v) = trunc(v 2^(48 - e)) as Python integers (object array)"""
    q = np.trunc(np.asarray(v, np.float64) * math.ldexp(1.0, 48 - e))
    return q.astype(np.int64).astype(object)


def moments(w, t, d2, e, e2):
    """the exact integers of one iteration -> dict(m, S, T, P (3x3 nested lists), D)"""
    qw, qt, qd = quantise(w, e), quantise(t, e), quantise(d2, e2)
    m = len(qw)
    S = [int(qw[:, a].sum()) if m else 0 for a in range(3)]
    T = [int(qt[:, a].sum()) if m else 0 for a in range(3)]
    P = [[int((qw[:, a] * qt[:, b]).sum()) if m else 0 for b in range(3)] for a in range(3)]
    return dict(m=m, S=S, T=T, P=P, D=int(qd.sum()) if m else 0)


def _rot(A, V, p, q):
    apq = A[p][q]
    if apq == 0.0:
        return
    app, aqq = A[p][p], A[q][q]
    theta = (aqq - app) / (2.0 * apq)
    if theta > 1e150 or theta < -1e150:
        t = 0.5 / theta
    else:
        t = 1.0 / ((-theta if theta < 0.0 else theta) + math.sqrt(theta * theta + 1.0))
        if theta < 0.0:
            t = -t
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    A[p][p] = app - t * apq
    A[q][q] = aqq + t * apq
    A[p][q] = A[q][p] = 0.0
    for o in range(4):
        if o == p or o == q:
            continue
        aop, aoq = A[o][p], A[o][q]
        A[o][p] = A[p][o] = c * aop - s * aoq
        A[o][q] = A[q][o] = s * aop + c * aoq
    for i in range(4):
        vip, viq = V[i][p], V[i][q]
        V[i][p] = c * vip - s * viq
        V[i][q] = s * vip + c * viq


def jacobi4(A):
    """cyclic Jacobi, rotations (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) per sweep, until the squared
    off-diagonal sum is exactly zero (at most 32 sweeps) -> (A, V)"""
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(32):
        off = ((((A[0][1] * A[0][1] + A[0][2] * A[0][2]) + A[0][3] * A[0][3]) + A[1][2] * A[1][2])
               + A[1][3] * A[1][3]) + A[2][3] * A[2][3]
        if off == 0.0:
            break
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            _rot(A, V, p, q)
    return A, V


def horn(M):
    """M: 3x3 nested list of floats (row = W's axis, column = the target's) -> R (3x3 nested list)"""
    big = max(abs(M[a][b]) for a in range(3) for b in range(3))
    sc = math.ldexp(1.0, 1 - math.frexp(big)[1]) if big > 0.0 else 1.0
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = [[v * sc for v in row] for row in M]
    A = [[0.0] * 4 for _ in range(4)]
    A[0][0] = (Sxx + Syy) + Szz
    A[1][1] = (Sxx - Syy) - Szz
    A[2][2] = (Syy - Sxx) - Szz
    A[3][3] = (Szz - Sxx) - Syy
    A[0][1] = A[1][0] = Syz - Szy
    A[0][2] = A[2][0] = Szx - Sxz
    A[0][3] = A[3][0] = Sxy - Syx
    A[1][2] = A[2][1] = Sxy + Syx
    A[1][3] = A[3][1] = Szx + Sxz
    A[2][3] = A[3][2] = Syz + Szy
    A, V = jacobi4(A)
    k = 0
    for i in range(1, 4):
        if A[i][i] > A[k][k]:
            k = i
    w, x, y, z = V[0][k], V[1][k], V[2][k], V[3][k]
    nq = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / nq, x / nq, y / nq, z / nq
    if w < 0.0:
        w, x, y, z = -w, -x, -y, -z
    return [[((w * w + x * x) - y * y) - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
            [2.0 * (x * y + w * z), ((w * w - x * x) + y * y) - z * z, 2.0 * (y * z - w * x)],
            [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), ((w * w - x * x) - y * y) + z * z]]


def rounded_moments(mo):
    """M_ab = RN(m P_ab - S_a T_b) (float(int) rounds to nearest, ties to even)"""
    m = mo["m"]
    return [[float(m * mo["P"][a][b] - mo["S"][a] * mo["T"][b]) for b in range(3)] for a in range(3)]


def solve(mo, e, e2):
    """-> (T float32 [4,4], mse float, R nested list in double)"""
    R = horn(rounded_moments(mo))
    md, back = float(mo["m"]), math.ldexp(1.0, e - 48)
    cs = [float(mo["S"][a]) / md * back for a in range(3)]
    ct = [float(mo["T"][a]) / md * back for a in range(3)]
    T = np.zeros((4, 4), f32)
    for a in range(3):
        t = ct[a] - ((R[a][0] * cs[0] + R[a][1] * cs[1]) + R[a][2] * cs[2])
        T[a, :3] = [f32(R[a][b]) for b in range(3)]
        T[a, 3] = f32(t)
    T[3, 3] = 1.0
    mse = float(mo["D"]) / md * math.ldexp(1.0, e2 - 48)
    return T, mse, R


def solve_double(mo, e):
    """the solve's R | t before the cast to float, as a float64 [3,4] (for the comparison with an
    SVD solve)"""
    R = horn(rounded_moments(mo))
    md, back = float(mo["m"]), math.ldexp(1.0, e - 48)
    cs = [float(mo["S"][a]) / md * back for a in range(3)]
    ct = [float(mo["T"][a]) / md * back for a in range(3)]
    t = [ct[a] - ((R[a][0] * cs[0] + R[a][1] * cs[1]) + R[a][2] * cs[2]) for a in range(3)]
    return np.concatenate([np.array(R, np.float64), np.array(t, np.float64)[:, None]], axis=1)


def umeyama_svd(w, t):
    """the rigid least-squares motion of w onto t by a float64 SVD (Umeyama without scale), [3,4]"""
    w, t = np.asarray(w, np.float64), np.asarray(t, np.float64)
    cw, ct = w.mean(axis=0), t.mean(axis=0)
    H = (t - ct).T @ (w - cw)
    U, _, Vt = np.linalg.svd(H)
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ S @ Vt
    return np.concatenate([R, (ct - R @ cw)[:, None]], axis=1)


def motion_error(final, motion):
    """final . motion against the identity: (rotation angle in radians, translation norm)"""
    E = np.asarray(final, np.float64).reshape(4, 4) @ np.asarray(motion, np.float64).reshape(4, 4)
    skew = 0.5 * (E[:3, :3] - E[:3, :3].T)  # (its Frobenius norm is sqrt(2) sin(angle))
    return math.asin(min(1.0, float(np.linalg.norm(skew)) / math.sqrt(2.0))), \
        float(np.linalg.norm(E[:3, 3]))


def mul4(a, b):
    """float32 4x4 product, each entry's four products summed left to right"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    out = np.empty((4, 4), f32)
    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(4):
                out[i, j] = ((a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]) \
                    + a[i, 3] * b[3, j]
    return out


class Criteria:
    def __init__(self, max_iterations=10, transformation_epsilon=0.0,
                 euclidean_fitness_epsilon=-DBL_MAX):
        self.max_iterations = max_iterations
        self.rot_thr = 1.0 - transformation_epsilon
        self.trans_thr = transformation_epsilon
        self.rel = euclidean_fitness_epsilon
        self.prev = DBL_MAX

    def check(self, iterations, T, mse):
        if iterations >= self.max_iterations:
            return ITERATIONS
        cos_angle = 0.5 * (((float(T[0, 0]) + float(T[1, 1])) + float(T[2, 2])) - 1.0)
        tx, ty, tz = float(T[0, 3]), float(T[1, 3]), float(T[2, 3])
        if cos_angle >= self.rot_thr and (tx * tx + ty * ty) + tz * tz <= self.trans_thr:
            return TRANSFORM
        ad = abs(mse - self.prev)
        if ad < 1e-12:
            return ABS_MSE
        if ad / self.prev < self.rel:
            return REL_MSE
        self.prev = mse
        return NOT_CONVERGED


def fitness_score(W, tgt, max_range=DBL_MAX, fast=False, info=None):
    """getFitnessScore: the pairs with d2 <= max_range (a NaN or negative range keeps none)"""
    if fast:
        nn, d2 = correspondences_fast(W, tgt, info=info)
    else:
        nn, d2 = correspondences(W, tgt)
    k = (nn >= 0) & (d2.astype(np.float64) <= float(max_range))
    if not k.any():
        return DBL_MAX
    e2 = qexp(d2[k].max())
    return float(int(quantise(d2[k], e2).sum())) / float(int(k.sum())) * math.ldexp(1.0, e2 - 48)


def align(src, tgt, indices=None, guess=None, max_iterations=10, max_dist=math.sqrt(DBL_MAX),
          transformation_epsilon=0.0, euclidean_fitness_epsilon=-DBL_MAX, fitness_max_range=DBL_MAX,
          keep_pairs=False, compute_fitness=True, fast=False, info=None):
    """fast: the correspondences by correspondences_fast (info collects its counts);
    compute_fitness False: fitness 0.0, as the library reports it when it is not asked for.
    -> dict(final [4,4] f32, history (list of dict n_corr, mse, e, e2, T), aligned [m,3] f32,
    state, iterations, converged, fitness, n_corr, mse[, pairs: per iteration (w, t, d2)])"""
    src = np.asarray(src, f32).reshape(-1, 3)
    tgt = np.asarray(tgt, f32).reshape(-1, 3)
    W = src if indices is None else src[np.asarray(indices, np.int64)]
    W = W.copy()
    final = IDENTITY.copy() if guess is None else np.asarray(guess, f32).reshape(4, 4).copy()
    if guess is not None and final.tobytes() != IDENTITY.tobytes():
        W = transform_points(final, W)
    tmax = max_abs_finite(tgt)
    crit = Criteria(max_iterations, transformation_epsilon, euclidean_fitness_epsilon)
    hist, pairs = [], []
    iterations, state, n_corr, mse = 0, NOT_CONVERGED, 0, 0.0
    while True:
        nn, d2 = correspondences_fast(W, tgt, max_dist, info=info) if fast else \
            correspondences(W, tgt, max_dist)
        k = np.nonzero(nn >= 0)[0]
        n_corr = len(k)
        if n_corr < 3:
            state = NO_CORRESPONDENCES
            break
        e = qexp(max(tmax, max_abs_finite(W)))
        e2 = qexp(d2[k].max())
        w, t = W[k], tgt[nn[k]]
        if keep_pairs:
            pairs.append((w.copy(), t.copy(), d2[k].copy()))
        mo = moments(w, t, d2[k], e, e2)
        T, mse, _ = solve(mo, e, e2)
        W = transform_points(T, W)
        final = mul4(T, final)
        hist.append(dict(n_corr=n_corr, mse=mse, e=e, e2=e2, T=T))
        iterations += 1
        state = crit.check(iterations, T, mse)
        if state != NOT_CONVERGED:
            break
    out = dict(final=final, history=hist, aligned=W, state=state, iterations=iterations,
               converged=int(state not in (NOT_CONVERGED, NO_CORRESPONDENCES)), n_corr=n_corr,
               mse=mse, fitness=fitness_score(W, tgt, fitness_max_range, fast, info)
               if compute_fitness else 0.0)
    if keep_pairs:
        out["pairs"] = pairs
    return out


# ---- the cases of tests/golden/icp_small.npz --------------------------------------------------------
def rigid(axis, deg, t):
    """a float32 4x4 from an axis, an angle in degrees and a translation (float64 Rodrigues)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T.astype(f32)


def shadow_split():
    """double_shadow.pcd by its rgb field: (source 446 points, target 545 points)"""
    from dialog_amd import pcd
    path = os.path.join(ROOT, "tests", "golden", "double_shadow.pcd")
    xyz = pcd.read_pcd(path)
    rgb = []
    with open(path) as f:
        body = False
        for ln in f:
            if body and ln.strip():
                rgb.append(int(ln.split()[3]))
            elif ln.startswith("DATA"):
                body = True
    rgb = np.array(rgb[:len(xyz)], np.int64)
    vals, counts = np.unique(rgb, return_counts=True)
    assert sorted(counts.tolist()) == [446, 545], counts
    src = xyz[rgb == vals[np.argmin(counts)]]
    tgt = xyz[rgb == vals[np.argmax(counts)]]
    return np.ascontiguousarray(src, f32), np.ascontiguousarray(tgt, f32)


SHADOW_MOTION = dict(axis=(0.0, 0.0, 1.0), deg=5.0, t=(0.01, 0.0, 0.0))


def build_cases():
    """name -> dict(src, tgt, and align()'s keyword arguments).  Deterministic."""
    from dialog_amd.synth import plane_cloud
    cases = {}
    src, tgt = shadow_split()
    cases["shadow"] = dict(src=src, tgt=tgt)
    moved = transform_points(rigid(**SHADOW_MOTION), src)
    cases["shadow_moved"] = dict(src=moved, tgt=tgt)
    # a max_dist that keeps between 20 % and 80 % of the first iteration's pairs: their median d2
    _, d2 = correspondences(src, tgt)
    md = math.sqrt(float(np.median(d2.astype(np.float64))))
    cases["shadow_maxdist"] = dict(src=src, tgt=tgt, max_dist=md)
    cases["shadow_guess"] = dict(src=src, tgt=tgt, guess=rigid((0.2, 1.0, 0.1), 2.0,
                                                                (0.004, -0.003, 0.002)))
    rng = np.random.default_rng(20240611)
    idx = rng.integers(0, len(src), size=300).astype(np.int32)
    idx[10:20] = idx[0]
    cases["shadow_dups"] = dict(src=src, tgt=tgt, indices=idx)
    # planes: the target is a moved, independently sampled copy
    ps = plane_cloud(5000, 3, seed=771, shard=0)[0]
    pt = transform_points(rigid((0.3, -0.2, 1.0), 1.5, (0.05, -0.03, 0.02)),
                          plane_cloud(7000, 3, seed=771, shard=1)[0])
    cases["planes_mse"] = dict(src=ps, tgt=pt, max_iterations=30, euclidean_fitness_epsilon=1e-3)
    cases["planes_iter"] = dict(src=ps, tgt=pt, max_iterations=4)
    # far: every source point outside the target's extent
    far = (src + f32(3.0)).astype(f32)
    cases["far"] = dict(src=far, tgt=tgt, max_iterations=3)
    # ties: an integer lattice, the source at cell centres (8 equidistant neighbours each)
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1)
    lat = g.reshape(-1, 3).astype(f32)
    cen = (lat[(lat < 5).all(axis=1)] + f32(0.5)).astype(f32)
    cases["ties"] = dict(src=cen, tgt=lat, max_iterations=3)
    # big: coordinates near 1e4; W starts beyond 2^13 = 8192 and moves below it, the target lies
    # below: e changes between iterations
    bs = (plane_cloud(400, 2, seed=99, patch=2.0)[0] + f32([8196.0, 8100.0, 8000.0])).astype(f32)
    bt = (plane_cloud(500, 2, seed=99, patch=2.0, shard=3)[0]
          + f32([8185.0, 8100.0, 8000.0])).astype(f32)
    cases["big"] = dict(src=bs, tgt=bt, max_iterations=6)
    # non-finite points in both clouds
    ns, nt = moved.copy(), tgt.copy()
    ns[5, 0] = np.nan
    ns[77, 2] = np.inf
    ns[200] = np.nan
    nt[0, 1] = np.nan
    nt[300, 0] = -np.inf
    cases["nonfinite"] = dict(src=ns, tgt=nt)
    return cases


CASE_NAMES = ["shadow", "shadow_moved", "shadow_maxdist", "shadow_guess", "shadow_dups", "planes_mse",
              "planes_iter", "far", "ties", "big", "nonfinite"]
ALIGN_KEYS = ("indices", "guess", "max_iterations", "max_dist", "transformation_epsilon",
              "euclidean_fitness_epsilon")


def run_case(case, **kw):
    args = {k: case[k] for k in ALIGN_KEYS if k in case}
    return align(case["src"], case["tgt"], **args, **kw)


# ---- inputs beyond the fixture (deterministic, generated: test_icp.py checks what each is for, ----
# ---- test_icp_gpu.py runs them on the device) -----------------------------------------------------
def neighbour_spacing(P):
    """the median distance of a point of P to its nearest other point (float64)"""
    from scipy.spatial import cKDTree
    P = np.asarray(P, np.float64)
    return float(np.median(cKDTree(P).query(P, k=2)[0][:, 1]))


def tiled_source(src, n, seed=4096):
    """n entries: src repeated, every entry moved by its own float32 jitter of up to a quarter of
    src's neighbour spacing per axis (no two entries equal)"""
    src = np.asarray(src, f32).reshape(-1, 3)
    j = 0.25 * neighbour_spacing(src)
    rng = np.random.default_rng(seed)
    return (src[np.arange(n) % len(src)] + rng.uniform(-j, j, size=(n, 3)).astype(f32)).astype(f32)


SCATTER_RUNGS = 11          # push distances spacing * 2^0 .. 2^10
# the share of each rung: a tenth stays within the neighbour spacing, the rungs between thin the
# deferral queues out level by level, and more than half leave the target's extent altogether
# (so the median d2 lies on rung 9 and the pairs below it span rungs 0..9)
SCATTER_SHARES = [0.10] + [0.04] * 8 + [0.29, 0.29]


def scatter_case(n_src=2987, n_tgt=3001, n_bad=8, seed=31337):
    """dict(src, tgt, spacing): each finite source entry is a target point pushed off in a random
    direction by spacing * 2^rung, n_bad more entries are not finite, and the list is shuffled"""
    from dialog_amd.synth import plane_cloud
    tgt = plane_cloud(n_tgt, 3, seed=seed, patch=2.0)[0]
    s = neighbour_spacing(tgt)
    rng = np.random.default_rng(seed + 1)
    rung = rng.choice(SCATTER_RUNGS, size=n_src, p=SCATTER_SHARES)
    u = rng.normal(size=(n_src, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    base = tgt[rng.integers(0, n_tgt, size=n_src)].astype(np.float64)
    src = (base + u * (s * np.exp2(rung))[:, None]).astype(f32)
    bad = np.zeros((n_bad, 3), f32)
    bad[:] = tgt[:n_bad]
    for k in range(n_bad):
        bad[k, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    src = np.concatenate([src, bad])
    return dict(src=np.ascontiguousarray(src[rng.permutation(len(src))]), tgt=tgt, spacing=s)


def degenerate_cases():
    """name -> dict(src, tgt): a target on the exact plane z = 0.25 under a source on z = 0.26, and a
    target on the x axis (y = z = 0 exactly) beside a source a little off it"""
    rng = np.random.default_rng(2025)
    pt = np.empty((401, 3), f32)
    pt[:, :2] = rng.uniform(0.0, 1.0, size=(401, 2))
    pt[:, 2] = f32(0.25)
    ps = np.empty((333, 3), f32)
    ps[:, :2] = rng.uniform(0.1, 0.9, size=(333, 2))
    ps[:, 2] = f32(0.26)
    ps = transform_points(rigid((0, 0, 1), 2.0, (0.01, -0.02, 0.0)), ps)
    lt = np.zeros((307, 3), f32)
    lt[:, 0] = rng.uniform(0.0, 1.0, size=307)
    ls = np.empty((259, 3), f32)
    ls[:, 0] = rng.uniform(0.05, 0.9, size=259)
    ls[:, 1:] = rng.uniform(-0.01, 0.01, size=(259, 2))
    return dict(plane=dict(src=ps, tgt=pt), line=dict(src=ls, tgt=lt))


SCALE_RUNGS = (-70, -60, -40, 40, 60)


def scaled_case(case, k):
    """the case's clouds times 2^k (exact in float32)"""
    return dict(src=np.ldexp(case["src"], k).astype(f32), tgt=np.ldexp(case["tgt"], k).astype(f32))


LARGE_SRC, LARGE_TGT = 600000, 50000


def large_case():
    """planes_iter's construction at a production launch shape: 600,000 entries against 50,000"""
    from dialog_amd.synth import plane_cloud
    ps = plane_cloud(LARGE_SRC, 3, seed=771, shard=0)[0]
    pt = transform_points(rigid((0.3, -0.2, 1.0), 1.5, (0.05, -0.03, 0.02)),
                          plane_cloud(LARGE_TGT, 3, seed=771, shard=1)[0])
    return dict(src=ps, tgt=pt, max_iterations=2)


def history_arrays(r):
    """the history as arrays: n_corr int64 [k], mse float64 [k], e / e2 int32 [k], T float32 [k,16]"""
    h = r["history"]
    return (np.array([x["n_corr"] for x in h], np.int64), np.array([x["mse"] for x in h], np.float64),
            np.array([[x["e"], x["e2"]] for x in h], np.int32).reshape(-1, 2),
            np.array([x["T"].reshape(16) for x in h], f32).reshape(-1, 16))
