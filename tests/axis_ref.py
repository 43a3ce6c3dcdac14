"""Restatement of the axis-constrained plane models for the tests (no test in this file).

SACMODEL_PERPENDICULAR_PLANE (9) and SACMODEL_PARALLEL_PLANE (15) are SACMODEL_PLANE with an
isModelValid gate (parity unpinned): countWithinDistance returns 0 and
selectWithinDistance returns nothing for an invalid model.  Everything but the gate is composed
from the frozen oracle's primitives: oracle.numpy_twin (Rnd, sample_good, coefficients, within and
sac_segment's loop, restated here with the gate) and oracle.oracle (count_within, count_within_np,
mean_cov, eigen33, refit_exact, fast_qexp).
"""
import math

import numpy as np

from oracle import numpy_twin as T
from oracle import oracle as O

F = np.float32
PLANE, PERP, NORMAL_PLANE, PAR = 0, 9, 11, 15
DBL_EPS = np.finfo(np.float64).eps


def normalized4(v):
    """Eigen Vector4f(v0, v1, v2, 0).normalized() (orc_normalized4's arithmetic)"""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        z = F(F(F(v[0] * v[0]) + F(v[2] * v[2])) + F(F(v[1] * v[1]) + F(F(0) * F(0))))
        if z > F(0):
            s = np.sqrt(z)
            return np.array([v[0] / s, v[1] / s, v[2] / s], F)
    return np.array([v[0], v[1], v[2]], F)


def dot_predux(a, n):
    with np.errstate(all="ignore"):
        return F(F(F(a[0] * n[0]) + F(a[2] * n[2])) + F(F(a[1] * n[1]) + F(F(0) * F(0))))


def perp_angle(rad_f):
    """m of the perpendicular model from the float dot product rad_f"""
    rad = float(rad_f)
    if rad < -1.0:
        rad = -1.0
    elif rad > 1.0:
        rad = 1.0
    th = math.acos(rad) if rad == rad else math.nan
    alt = math.pi - th
    return alt if alt < th else th


def perp_valid_f(rad_f, eps):
    return not (perp_angle(rad_f) > eps)


def par_valid_f(dot_f, eps):
    return not (float(abs(F(dot_f))) > abs(math.sin(eps)))


def model_valid(model, axis, eps, c):
    """isModelValid(c) of `model` (True for the unconstrained models and for eps <= 0)"""
    if model not in (PERP, PAR) or not (eps > 0.0):
        return True
    cn = normalized4(c[:3])
    if model == PERP:
        return perp_valid_f(dot_predux(normalized4(axis), cn), eps)
    return par_valid_f(dot_predux(np.asarray(axis, F), cn), eps)


def refit(points, inl, c, mode, qexp):
    """optimizeModelCoefficients (SACMODEL_PLANE's, unconstrained): PCL's float refit or the
    product's exact-moment fast refit; < 4 inliers keep the coefficients"""
    if inl.shape[0] < 4:
        return c.copy()
    if mode == "fast":
        return O.refit_exact(points, inl.astype(np.int32), c, qexp)
    cov, cen = O.mean_cov(points, inl.astype(np.int32))
    _, v = O.eigen33(cov)
    dot = F(F(F(v[0] * cen[0]) + F(v[2] * cen[2])) + F(F(v[1] * cen[1]) + F(F(0) * cen[3])))
    return np.array([v[0], v[1], v[2], F(F(-1.0) * dot)], F)


def count(model, axis, eps, pts, idx, c, thr, normals=None, lam=0.1):
    if not model_valid(model, axis, eps, c):
        return 0
    if model == NORMAL_PLANE:
        return int(O.count_within_np(pts[idx], normals[idx], c, thr, lam))
    return int(O.count_within(pts, c, thr, indices=idx.astype(np.int32)))


def segment(points, thr, model=PLANE, axis=(0, 0, 0), eps=0.0, indices=None, max_iterations=50,
            probability=0.99, optimize=True, refit_mode="pcl", qexp=None, seed=12345):
    """numpy_twin.sac_segment's loop with the validity gate (models 0, 9, 15)"""
    pts = np.ascontiguousarray(points, F)[:, :3]
    idx = (np.arange(pts.shape[0], dtype=np.int64) if indices is None
           else np.asarray(indices, np.int64))
    n = idx.shape[0]
    sub = pts[idx]
    shuf = idx.copy()
    rnd = T.Rnd(seed)
    it, best, k = 0, -(2 ** 31 - 1), 1.0
    log_p = math.log(1.0 - probability) if probability < 1.0 else -math.inf
    one_over = 1.0 / n if n else math.inf
    best_c = best_s = None
    draws = 0
    while it < k:
        if n < 3:
            it = 2 ** 31 - 2
            break
        found = False
        for _ in range(1000):
            for i in range(3):
                j = i + rnd() % (n - i)
                shuf[i], shuf[j] = shuf[j], shuf[i]
            draws += 1
            s = shuf[:3].copy()
            if T.sample_good(pts[s[0]], pts[s[1]], pts[s[2]]):
                found = True
                break
        if not found:
            break
        c = T.coefficients(pts[s[0]], pts[s[1]], pts[s[2]])
        assert c is not None
        # an invalid model is an ordinary iteration with count 0 (not a skip)
        cnt = count(model, axis, eps, pts, idx, c, thr)
        if cnt > best:
            best, best_c, best_s = cnt, c, s
            w = best * one_over
            pno = 1.0 - w ** 3.0
            pno = min(max(DBL_EPS, pno), 1.0 - DBL_EPS)
            k = log_p / math.log(pno)
        it += 1
        if it > max_iterations:
            break
    if best_c is None:
        return dict(ok=False, coeff=np.zeros(4, F), inliers=np.zeros(0, np.int32), iterations=it,
                    draws=draws, best_sample=None, coeff_unrefined=None, n_unrefined=0,
                    unrefined_valid=True, refined_valid=True)
    none = np.zeros(0, np.int64)
    uv = model_valid(model, axis, eps, best_c)
    inl = idx[T.within(best_c, sub, thr)] if uv else none
    n_unref = inl.shape[0]
    assert n_unref == best
    coeff = best_c
    if optimize:
        q = qexp if qexp is not None else O.fast_qexp(pts, idx.astype(np.int32))
        coeff = refit(pts, inl, best_c, refit_mode, q)
    rv = model_valid(model, axis, eps, coeff)
    inl = idx[T.within(coeff, sub, thr)] if rv else none
    return dict(ok=True, coeff=coeff, inliers=inl.astype(np.int32), iterations=it, draws=draws,
                best_sample=best_s.astype(np.int32), coeff_unrefined=best_c, n_unrefined=n_unref,
                unrefined_valid=uv, refined_valid=rv)


def extract(points, thr, max_planes, min_inliers=0, **kw):
    """numpy_twin.extract_planes' loop over segment() above"""
    pts = np.ascontiguousarray(points, F)[:, :3]
    rem = np.arange(pts.shape[0], dtype=np.int64)
    coeffs, inls, offs = [], [], [0]
    floor_n = max(3, min_inliers)
    if kw.get("refit_mode") == "fast":
        kw = dict(kw, qexp=O.fast_qexp(pts))  # the whole cloud's quantum, fixed for all rounds
    while len(coeffs) < max_planes and rem.shape[0] >= floor_n:
        r = segment(pts, thr, indices=rem, **kw)
        nin = r["inliers"].shape[0]
        if not r["ok"] or nin == 0 or nin < min_inliers:
            break
        coeffs.append(r["coeff"])
        inls.append(r["inliers"])
        offs.append(offs[-1] + nin)
        rem = np.setdiff1d(rem, r["inliers"].astype(np.int64), assume_unique=True)
    return dict(coeffs=np.array(coeffs, F).reshape(-1, 4), offsets=np.array(offs, np.int64),
                inliers=np.concatenate(inls).astype(np.int32) if inls else np.zeros(0, np.int32),
                n_planes=len(coeffs), remaining=rem.astype(np.int32))


def score(points, thr, positions, model, axis=(0, 0, 0), eps=0.0, active=None, normals=None,
          lam=0.1):
    """what dlg_score_samples returns for the draws `positions` ([D, 3] positions into the active
    list `active`, ids into points): counts, good, valid, coeffs"""
    pts = np.ascontiguousarray(points, F)[:, :3]
    idx = (np.arange(pts.shape[0], dtype=np.int64) if active is None
           else np.asarray(active, np.int64))
    d = positions.shape[0]
    counts = np.zeros(d, np.int32)
    good = np.zeros(d, np.int32)
    valid = np.ones(d, np.int32)
    coeffs = np.full((d, 4), np.nan, F)
    for i in range(d):
        s = idx[positions[i]]
        if not T.sample_good(pts[s[0]], pts[s[1]], pts[s[2]]):
            continue
        c = T.coefficients(pts[s[0]], pts[s[1]], pts[s[2]])
        good[i] = 1
        coeffs[i] = c
        valid[i] = 1 if model_valid(model, axis, eps, c) else 0
        counts[i] = count(model, axis, eps, pts, idx, c, thr, normals, lam)
    return dict(counts=counts, good=good, valid=valid, coeffs=coeffs)


def room(n, second_wall=False, floor=True, noise=True, seed=5):
    """floor z = 0 (60 %), wall x = 0 (25 %), a 30-degree ramp (10 %), 5 % noise, shuffled;
    second_wall: a wall y = 0 takes a third of the floor's share; floor / noise False: their
    points go to the wall and the ramp instead"""
    rng = np.random.default_rng(seed + n)
    lab = rng.choice(4, size=n, p=[0.60, 0.25, 0.10, 0.05])
    if n >= 3:
        lab[:3] = [0, 1, 2]  # every structure is present even in the smallest cloud
    for on, k in ((floor, 0), (noise, 3)):
        if not on:
            lab[lab == k] = 1 + (np.arange(n)[lab == k] % 2)
    u = rng.uniform(0.0, 4.0, n)
    v = rng.uniform(0.0, 4.0, n)
    e = rng.normal(0.0, 0.004, n)
    p = np.empty((n, 3), np.float64)
    p[lab == 0] = np.c_[u, v, e][lab == 0]
    p[lab == 1] = np.c_[e, u, v * 0.6][lab == 1]
    t = math.radians(30.0)
    ramp = np.c_[u * math.cos(t) - e * math.sin(t), v, u * math.sin(t) + e * math.cos(t)]
    p[lab == 2] = ramp[lab == 2]
    p[lab == 3] = np.c_[u, v, rng.uniform(0.0, 2.4, n)][lab == 3]
    if second_wall:
        w2 = (lab == 0) & (np.arange(n) % 3 == 0)
        p[w2] = np.c_[u, e, v * 0.6][w2]
    return np.ascontiguousarray(p, F)
