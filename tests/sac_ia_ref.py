"""numpy restatement of dlg_sac_ia_align / dlg_sac_ia_score / dlg_fpfh_knn (include/dialog_ransac.h,
the "SAC-IA initial alignment" section; dialog_amd/csrc/sacia_model.hpp is the C++ it is compared
with): pcl::SampleConsensusInitialAlignment of PCL 1.8 with the default TruncatedError.

rand() replayed (glibc's TYPE_3 generator or MSVC's LCG), brute-force float32 searches in FLANN's
operation order, icp_ref.py's exact moments and Horn solve for the rigid estimate, Python integers
for the hypothesis errors.  Also the case list of tests/golden/sac_ia_small.npz (make_sac_ia.py
writes it, test_sac_ia.py recomputes it, test_sac_ia_gpu.py compares the device with it).
"""
from __future__ import annotations

import math
import sys

import numpy as np

import fpfh_ref as F
import icp_ref as R

f32 = np.float32
f64 = np.float64
DBL_MAX = sys.float_info.max
DIM = 33
RNG_GLIBC, RNG_MSVC = 0, 1
MAX_SAMPLES = 8


# ---- rand() -----------------------------------------------------------------------------------
class Rand:
    """glibc's rand() (TYPE_3: r_i = r_{i-31} + r_{i-3}, output k = r_{k+344} >> 1) or the Visual
    C++ runtime's (s = s 214013 + 2531011, bits 16..30)"""

    def __init__(self, kind=RNG_GLIBC, seed=1):
        self.kind = kind
        if kind == RNG_MSVC:
            self.s = seed & 0xFFFFFFFF
            self.denom = 32768.0
            return
        self.denom = 2147483648.0
        seed &= 0xFFFFFFFF
        w = 1 if seed == 0 else seed
        if w >= 1 << 31:
            w -= 1 << 32
        r = [w & 0xFFFFFFFF]
        for _ in range(1, 31):
            w = (16807 * w) % 2147483647  # (non-negative in Python)
            r.append(w)
        for i in range(31, 34):
            r.append(r[i - 31])
        self.r = r
        for _ in range(34, 344):
            self._step()

    def _step(self):
        r = self.r
        v = (r[-31] + r[-3]) & 0xFFFFFFFF
        r.append(v)
        del r[0]
        return v

    def next(self):
        if self.kind == RNG_MSVC:
            self.s = (self.s * 214013 + 2531011) & 0xFFFFFFFF
            return (self.s >> 16) & 0x7FFF
        return self._step() >> 1

    def index(self, n):
        """getRandomIndex"""
        return int(float(n) * (float(self.next()) / self.denom))


# ---- the pieces ---------------------------------------------------------------------------------
def point_dist(a, b):
    with np.errstate(all="ignore"):
        d = a - b
        return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], dtype=f32)


def select_samples(rng, src, nr, min_sample_distance):
    """-> (samples, rand() calls, halvings of the distance)"""
    msd = f32(min_sample_distance)
    n = len(src)
    out, draws, relax, without = [], 0, 0, 0
    while len(out) < nr:
        idx = rng.index(n)
        draws += 1
        valid = True
        for s in out:
            if idx == s or point_dist(src[idx], src[s]) < msd:
                valid = False
                break
        if valid:
            out.append(idx)
            without = 0
        else:
            without += 1
        if without >= 3 * n:
            msd = f32(msd * f32(0.5))
            relax += 1
            without = 0
    return out, draws, relax


def feature_d2(q, rows):
    """FLANN's L2_Simple: q (a, 33), rows (b, 33) float32 -> (a, b) float32, r = 0; r += d * d
    (fpfh_ref.flann_d2's convention over 33 values)"""
    q = np.asarray(q, f32).reshape(-1, DIM)
    rows = np.asarray(rows, f32).reshape(-1, DIM)
    with np.errstate(all="ignore"):
        acc = np.zeros((len(q), len(rows)), f32)
        for j in range(DIM):
            e = (q[:, j, None] - rows[None, :, j]).astype(f32)
            acc = (acc + (e * e).astype(f32)).astype(f32)
    return acc


def knn(queries, rows, k, valid=None):
    """the k nearest valid rows of every query in (d, index) order -> (idx int32 [nq, k], d float32
    [nq, k]); -1 and 0 for a query with a non-finite value.  valid: a mask over the rows (default:
    the rows with 33 finite values)."""
    queries = np.asarray(queries, f32).reshape(-1, DIM)
    rows = np.asarray(rows, f32).reshape(-1, DIM)
    if valid is None:
        valid = np.isfinite(rows).all(1)
    ids = np.nonzero(valid)[0]
    assert len(ids) >= k, "fewer valid rows than k"
    idx = np.full((len(queries), k), -1, np.int32)
    dd = np.zeros((len(queries), k), f32)
    ok = np.nonzero(np.isfinite(queries).all(1))[0]
    step = max(1, (1 << 21) // max(len(ids), 1))
    for a in range(0, len(ok), step):
        sel = ok[a:a + step]
        d = feature_d2(queries[sel], rows[ids])
        order = np.argsort(d, axis=1, kind="stable")[:, :k]  # (stable: equal d in index order)
        idx[sel] = ids[order]
        dd[sel] = np.take_along_axis(d, order, 1)
    return idx, dd


def threshold(max_correspondence_distance):
    """(float)corr_dist_threshold_; out of range: +inf"""
    with np.errstate(over="ignore"):
        return f32(f64(max_correspondence_distance))


def nearest_d2(W, tgt_valid):
    """per finite row of W the smallest float32 squared distance to the valid target points"""
    out = np.full(len(W), np.inf, f32)
    step = max(1, (1 << 22) // max(len(tgt_valid), 1))
    for a in range(0, len(W), step):
        out[a:a + step] = F.flann_d2(W[a:a + step], tgt_valid).min(axis=1)
    return out


def error_metric(T, src, tgt_valid, thr):
    """computeErrorMetric -> (E, n_far, n_used); E = sum trunc(term 2^48), a Python integer"""
    src = np.asarray(src, f32).reshape(-1, 3)
    W = R.transform_points(T, src)
    ok = np.isfinite(src).all(1) & np.isfinite(W).all(1)
    E, far = error_of_distances(nearest_d2(W[ok], tgt_valid), thr)
    return E, far, int(ok.sum())


def error_of_distances(e, thr):
    """the squared distances of the points that add a term -> (E, n_far)"""
    e, thr = np.asarray(e, f32), f32(thr)
    with np.errstate(all="ignore"):
        term = np.where(e <= thr, e / thr, f32(1.0)).astype(f32)
    term[np.isnan(term)] = f32(1.0)
    q = (term.astype(f64) * 2.0 ** 48).astype(np.uint64)
    E = (int((q >> np.uint64(24)).sum()) << 24) + int((q & np.uint64(0xFFFFFF)).sum())
    return E, int((term == f32(1.0)).sum())


def guess_is_identity(g):
    g = np.asarray(g, f32).reshape(16)
    diff = norm = 0.0
    for k in range(16):
        v = float(g[k])
        d = v - (1.0 if k % 5 == 0 else 0.0)
        diff += d * d
        norm += v * v
    p2 = float(f32(0.01) * f32(0.01))
    return diff <= p2 * min(norm, 4.0)


def estimate(w, t):
    """the rigid estimate of the pairs w_i -> t_i: icp_ref's exact moments with e = the exponent of
    the pairs' largest |coordinate|, Horn, t = ct - R cs, cast to float32"""
    w, t = np.asarray(w, f32), np.asarray(t, f32)
    e = R.qexp(max(float(np.abs(w).max()), float(np.abs(t).max())))
    mo = R.moments(w, t, np.zeros(len(w), f32), e, 0)
    return R.solve(mo, e, 0)[0]


def valid_target(tgt, ft):
    return np.isfinite(np.asarray(tgt, f32)).all(1) & np.isfinite(np.asarray(ft, f32)).all(1)


def align(src, fs, tgt, ft, guess=None, max_iterations=1000, nr_samples=3, k_correspondences=10,
          min_sample_distance=0.0, max_correspondence_distance=math.sqrt(DBL_MAX), rng=RNG_GLIBC,
          seed=1, fitness_max_range=DBL_MAX, compute_fitness=True):
    """-> dict(final, aligned, hyp (a list of dict, one per iteration), converged, best_iteration,
    n_valid, n_invalid, draws, relaxations, n_queries, E (of the lowest scored), error, fitness)"""
    src = np.asarray(src, f32).reshape(-1, 3)
    tgt = np.asarray(tgt, f32).reshape(-1, 3)
    fs = np.asarray(fs, f32).reshape(-1, DIM)
    ft = np.asarray(ft, f32).reshape(-1, DIM)
    assert nr_samples <= len(src)
    thr = threshold(max_correspondence_distance)
    vt = valid_target(tgt, ft)
    tv = tgt[vt]
    assert vt.sum() >= k_correspondences
    final = R.IDENTITY.copy() if guess is None else np.asarray(guess, f32).reshape(4, 4).copy()
    score_guess = not guess_is_identity(final)
    n_rec = max(max_iterations, 1) if score_guess else max_iterations
    gen = Rand(rng, seed)
    src_ok = np.isfinite(src).all(1) & np.isfinite(fs).all(1)
    hyp = []
    for it in range(n_rec):
        h = dict(sample=[-1] * MAX_SAMPLES, match=[-1] * MAX_SAMPLES, rank=[-1] * MAX_SAMPLES,
                 valid=1, relaxations=0, draws=0, T=np.zeros((4, 4), f32), E=0, n_far=0, n_used=0)
        hyp.append(h)
        if it == 0 and score_guess:
            h["T"] = final.copy()
            continue
        s, draws, relax = select_samples(gen, src, nr_samples, min_sample_distance)
        ranks = [gen.index(k_correspondences) for _ in s]
        h["sample"][:nr_samples] = s
        h["rank"][:nr_samples] = ranks
        h["draws"], h["relaxations"] = draws + nr_samples, relax
        h["valid"] = int(all(src_ok[i] for i in s))
    queries = sorted({i for h in hyp if h["valid"] and h["draws"] for i in h["sample"] if i >= 0})
    nn = {}
    if queries:
        idx, _ = knn(fs[queries], ft, k_correspondences, vt)
        nn = {q: idx[u] for u, q in enumerate(queries)}
    scored, lowest, best = False, 0, -1
    for it, h in enumerate(hyp):
        if not h["valid"]:
            continue
        if h["draws"]:
            s = h["sample"][:nr_samples]
            m = [int(nn[i][r]) for i, r in zip(s, h["rank"][:nr_samples])]
            h["match"][:nr_samples] = m
            h["T"] = estimate(src[s], tgt[m])
        h["E"], h["n_far"], h["n_used"] = error_metric(h["T"], src, tv, thr)
        if not scored or h["E"] < lowest:
            scored, lowest = True, h["E"]
            if h["draws"]:
                best = it
                final = h["T"].copy()
    aligned = R.transform_points(final, src)
    drawn = [h for h in hyp if h["draws"]]
    return dict(final=final, aligned=aligned, hyp=hyp, converged=int(best >= 0), best_iteration=best,
                n_valid=sum(h["valid"] for h in drawn), n_invalid=sum(1 - h["valid"] for h in drawn),
                draws=sum(h["draws"] for h in hyp), relaxations=sum(h["relaxations"] for h in hyp),
                n_queries=len(queries), E=lowest if scored else 0,
                error=float(lowest) * 2.0 ** -48 if scored else 0.0,
                fitness=R.fitness_score(aligned, tgt, fitness_max_range) if compute_fitness else 0.0)


# ---- the cases of tests/golden/sac_ia_small.npz --------------------------------------------------
ALIGN_KEYS = ("max_iterations", "nr_samples", "k_correspondences", "min_sample_distance",
              "max_correspondence_distance", "rng", "seed")
CASE_NAMES = ["default", "finite_threshold", "moved_source", "guess_wins", "near_identity_guess",
              "relaxation", "n_src_3", "msvc", "k_1", "k_32", "nr_samples_5", "non_finite",
              "zero_rows"]
FPFH_RADIUS = (0.02, 0.05)  # (normals, descriptors): fpfh_ref's own case on the same scan


def descriptors(points):
    nrm = F.pca_normals(points, FPFH_RADIUS[0])
    return F.fpfh_ref(points, nrm, FPFH_RADIUS[1])["hist"]


def build_cases(fs=None, ft=None):
    """name -> dict(src, fs, tgt, ft[, guess], the ALIGN_KEYS that are not defaults).  fs / ft: the
    descriptors of double_shadow.pcd's two halves when the caller has them already."""
    src, tgt = R.shadow_split()
    fs = descriptors(src) if fs is None else np.asarray(fs, f32)
    ft = descriptors(tgt) if ft is None else np.asarray(ft, f32)
    spacing = R.neighbour_spacing(tgt)
    thr = float(f32((3.0 * spacing) ** 2))  # compared with the squared distance: 3 point spacings
    base = dict(src=src, fs=fs, tgt=tgt, ft=ft)
    fin = dict(base, max_correspondence_distance=thr)
    cases = {}
    cases["default"] = dict(base, max_iterations=60)
    cases["finite_threshold"] = dict(fin, max_iterations=200)
    moved = R.transform_points(R.rigid(**R.SHADOW_MOTION), src)
    cases["moved_source"] = dict(fin, src=moved, max_iterations=100)
    # a source cut from the target and turned by -90 degrees about z: the guess turns it back
    # exactly (its entries are 0 and +-1), so E(guess) = 0 and nothing can be strictly lower
    turn = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], f32)
    cut = np.arange(0, len(tgt), 3)
    back = np.stack([tgt[cut, 1], -tgt[cut, 0], tgt[cut, 2]], 1).astype(f32)
    cases["guess_wins"] = dict(fin, src=back, fs=ft[cut], guess=turn, max_iterations=40)
    near = R.IDENTITY.copy()
    near[0, 3] = 1e-4
    cases["near_identity_guess"] = dict(fin, guess=near, max_iterations=30)
    few = np.arange(0, len(src), 11)[:40]
    diam = float(np.linalg.norm(src.max(0) - src.min(0)))
    cases["relaxation"] = dict(fin, src=src[few], fs=fs[few], min_sample_distance=10.0 * diam,
                               max_iterations=20)
    cases["n_src_3"] = dict(fin, src=src[[5, 200, 400]], fs=fs[[5, 200, 400]], max_iterations=12)
    cases["msvc"] = dict(fin, rng=RNG_MSVC, seed=1, max_iterations=60)
    cases["k_1"] = dict(fin, k_correspondences=1, max_iterations=40)
    cases["k_32"] = dict(fin, k_correspondences=32, max_iterations=40)
    cases["nr_samples_5"] = dict(fin, nr_samples=5, max_iterations=40)
    s2, fs2, t2, ft2 = src.copy(), fs.copy(), tgt.copy(), ft.copy()
    s2[::9] = np.nan
    s2[4, 1] = np.inf
    fs2[3::13, 7] = np.nan
    t2[::7] = np.nan
    ft2[2::5, 30] = np.nan
    ft2[11] = np.inf
    cases["non_finite"] = dict(fin, src=s2, fs=fs2, tgt=t2, ft=ft2, max_iterations=80)
    # the descriptor of an isolated point is all zeros: exact ties among the target rows
    fs3, ft3 = fs.copy(), ft.copy()
    fs3[::4] = 0.0
    ft3[::3] = 0.0
    cases["zero_rows"] = dict(fin, fs=fs3, ft=ft3, max_iterations=60)
    assert list(cases) == CASE_NAMES
    return cases


def run_case(case, **kw):
    args = {k: case[k] for k in ALIGN_KEYS if k in case}
    args.update(kw)
    return align(case["src"], case["fs"], case["tgt"], case["ft"], guess=case.get("guess"), **args)


def hypothesis_arrays(r):
    """the records of a run as arrays: sample, match, rank int32 [H, 8]; valid, relaxations int32
    [H]; draws, n_far, n_used int64 [H]; T float32 [H, 16]; err_hi, err_lo uint64 [H]"""
    h = r["hyp"]
    H = len(h)
    out = dict(sample=np.array([x["sample"] for x in h], np.int32).reshape(H, 8),
               match=np.array([x["match"] for x in h], np.int32).reshape(H, 8),
               rank=np.array([x["rank"] for x in h], np.int32).reshape(H, 8),
               valid=np.array([x["valid"] for x in h], np.int32),
               relaxations=np.array([x["relaxations"] for x in h], np.int32),
               draws=np.array([x["draws"] for x in h], np.int64),
               n_far=np.array([x["n_far"] for x in h], np.int64),
               n_used=np.array([x["n_used"] for x in h], np.int64),
               T=np.array([np.asarray(x["T"], f32).reshape(16) for x in h], f32).reshape(H, 16),
               err_hi=np.array([x["E"] >> 24 for x in h], np.uint64),
               err_lo=np.array([x["E"] & 0xFFFFFF for x in h], np.uint64))
    return out


def check_paths(name, case, r):
    """what each case is there for (make_sac_ia.py and test_sac_ia.py both assert it)"""
    h = r["hyp"]
    n_src = len(case["src"])
    if name == "default":
        assert all(x["E"] == 0 for x in h) and r["best_iteration"] == 0 and r["converged"] == 1
        assert threshold(math.sqrt(DBL_MAX)) == np.inf
    if name == "finite_threshold":
        assert r["best_iteration"] > 0
        assert any(0 < x["n_far"] < n_src for x in h)
    if name == "guess_wins":
        assert h[0]["draws"] == 0 and h[0]["E"] == 0 and r["converged"] == 0
        assert r["best_iteration"] == -1
        assert np.array_equal(r["final"], np.asarray(case["guess"], f32))
        assert any(x["E"] > 0 for x in h[1:])
    if name == "near_identity_guess":
        assert h[0]["draws"] > 0 and r["converged"] == 1
    if name == "relaxation":
        assert r["relaxations"] > 0
    if name == "n_src_3":
        assert all(sorted(x["sample"][:3]) == [0, 1, 2] for x in h)
    if name == "non_finite":
        assert r["n_invalid"] > 0 and r["n_valid"] > 0
        assert all(x["E"] == 0 and x["n_used"] == 0 for x in h if not x["valid"])
    if name == "zero_rows":
        # a zero query's nearest rows are the zero rows, all at distance 0, in index order
        z = np.nonzero((case["ft"] == 0).all(1))[0]
        q = np.nonzero((case["fs"] == 0).all(1))[0][:1]
        idx, d = knn(case["fs"][q], case["ft"], 10)
        assert np.array_equal(idx[0], z[:10]) and (d == 0).all()
        assert any(x["valid"] and any(case["fs"][i].max() == 0 for i in x["sample"] if i >= 0)
                   for x in h)
