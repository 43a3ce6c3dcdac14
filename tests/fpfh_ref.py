"""numpy restatement of pcl::FPFHEstimation<PointXYZ, Normal, FPFHSignature33>::compute with
setRadiusSearch (PCL 1.8 fpfh.hpp and computePairFeatures, from memory: parity unpinned, DESIGN.md
§2), independent of the C code.  All arithmetic is float32 unless marked float64.

    search structure: every finite point of the cloud, listed or not
    neighbours of a point: float32 ((0 + dx^2) + dy^2) + dz^2 < float32(float64(r) * float64(r)),
    itself included, in (d2, index) order; m = their number
    pair (p, n_p) = the SPFH's own point, (q, n_q) = a neighbour:
        d = q - p; f4 = sqrt((dx^2 + dy^2) + dz^2); 0: the pair fails
        a1 = (n_p . d) / f4; a2 = (n_q . d) / f4 (dots summed left to right)
        acos(|a1|) > acos(|a2|): u = n_q, t = n_p, d = -d, f3 = -a2; else u = n_p, t = n_q, f3 = a1
        v = d x u; |v| = sqrt of its squared norm; 0: the pair fails; v /= |v|; w = u x v
        f2 = v . t; f1 = atan2(w . t, u . t)
        acos, atan2: the real function's value rounded to float32 (here: float64, then rounded)
    SPFH: incr = 100.0f / float(m - 1); every neighbour but the point itself (by index) whose pair
        does not fail adds incr to bins floor(11 ((f1 + pi) d_pi)), floor(11 ((f2 + 1) 0.5)),
        floor(11 ((f3 + 1) 0.5)) (float64, d_pi = 1.0f / (2.0f * float(pi)), clamped to 0..10, NaN to
        0) of the three histograms: a bin is the c-fold sequential float32 sum of incr
        a pair with a non-finite normal component adds nothing
    FPFH of a list entry: neighbours in (d2, index) order, d2 == 0 skipped; w = 1.0f / d2;
        val = spfh[nbr][b] * w; hist[b] += val (float32); sum_g += val (float64), neighbour-major,
        bin-minor; then hist[b] *= float32(100.0 / sum_g) where sum_g != 0
        non-finite entry: 33 NaN; no neighbour but itself: 33 zeros

Stability.  The device's and glibc's float64 acos / atan2 are not correctly rounded, so a float32
rounding of their value can differ from the real function's where the value lies next to a float32
rounding boundary.  A pair is stable when its swap decision and its three bin indices keep their
outcome with every float64 acos / atan2 value moved up or down by MARGIN_ULP float64 ulps before the
rounding to float32; an SPFH when all its pairs are; an FPFH row when every neighbour's SPFH is.
MARGIN_ULP should be the sum of the documented float64 error bounds of glibc and of the device
maths library; neither document (the glibc manual's "Errors in Math Functions", the device
library's function table) is installed where this was written, so it is 8.
"""
import numpy as np

f32 = np.float32
f64 = np.float64
MARGIN_ULP = 8
DIM = 33
BINS = 11
CAP = 1024  # fpfh.hpp kFpfhCap: entries with more neighbours count as n_lds_overflow


def flann_d2(q, p):
    """q (a, 3), p (b, 3) float32 -> (a, b) float32, each operation rounded to float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        acc = np.zeros((len(q), len(p)), f32)
        for a in range(3):
            e = (q[:, a, None] - p[None, :, a]).astype(f32)
            acc = (acc + (e * e).astype(f32)).astype(f32)
    return acc


def _nudge(x, k):
    """float64 x moved k float64 ulps (k < 0: down)"""
    return x + k * np.spacing(np.abs(x)) if k else x


def _dot(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(f32)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(f32)


def _bin(x):
    fl = np.floor(x)
    with np.errstate(invalid="ignore"):
        return np.where(~(fl >= 0.0), 0, np.where(fl > 10.0, 10, fl)).astype(np.int64)


def _bins_f1(f1):
    d_pi = f32(1.0) / (f32(2.0) * f32(np.pi))
    return _bin(11.0 * ((f1.astype(f64) + np.pi) * f64(d_pi)))


def _bins_unit(f):
    return _bin(11.0 * ((f.astype(f64) + 1.0) * 0.5))


def pair_features(p, n_p, q, n_q, ja=0, jb=0, jt=0):
    """(k, 3) float32 arrays -> ok (k,), f (k, 3) = f1, f2, f3, swapped (k,); ja / jb / jt: the
    float64 acos(|a1|) / acos(|a2|) / atan2 values moved that many ulps before rounding"""
    with np.errstate(all="ignore"):
        d = (q - p).astype(f32)
        f4 = np.sqrt(_dot(d, d)).astype(f32)
        ok = f4 != 0
        a1 = (_dot(n_p, d) / f4).astype(f32)
        a2 = (_dot(n_q, d) / f4).astype(f32)
        c1 = _nudge(np.arccos(np.abs(a1).astype(f64)), ja).astype(f32)
        c2 = _nudge(np.arccos(np.abs(a2).astype(f64)), jb).astype(f32)
        sw = c1 > c2
        u = np.where(sw[:, None], n_q, n_p)
        t = np.where(sw[:, None], n_p, n_q)
        d = np.where(sw[:, None], -d, d)
        f3 = np.where(sw, -a2, a1)
        v = _cross(d, u)
        vn = np.sqrt(_dot(v, v)).astype(f32)
        ok &= vn != 0
        v = (v / vn[:, None]).astype(f32)
        w = _cross(u, v)
        f2 = _dot(v, t)
        f1 = _nudge(np.arctan2(_dot(w, t).astype(f64), _dot(u, t).astype(f64)), jt).astype(f32)
    return ok, np.stack([f1, f2, f3], 1), sw


def bin_values(m, counts):
    """the c-fold sequential float32 sums of incr = 100.0f / float(m - 1): m (n,), counts (n, 33)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        incr = (f32(100.0) / (m - 1).astype(f32)).astype(f32)
    out = np.zeros(counts.shape, f32)
    s = np.zeros(len(m), f32)
    for c in range(1, int(counts.max(initial=0)) + 1):
        live = (counts >= c).any(1)
        s[live] = (s[live] + incr[live]).astype(f32)
        out = np.where(counts == c, s[:, None], out)
    return out


def _lo(v):
    """float32 v > 0 is an odd multiple of 2^lo (fpfh_model.hpp)"""
    b = v.view(np.uint32).astype(np.int64)
    e = (b >> 23) & 0xff
    mant = np.where(e != 0, (b & 0x7fffff) | 0x800000, b & 0x7fffff)
    e0 = np.where(e != 0, e - 150, -149)
    mant = np.where(mant == 0, 1, mant)
    # (frexp of an integer below 2^24 is exact: exponent - 1 = the index of its highest set bit)
    return e0 + np.frexp((mant & -mant).astype(f64))[1] - 1


def fpfh_ref(points, normals, radius, idx=None, order="d2", margin=MARGIN_ULP):
    """-> dict: hist (n_list, 33) float32, neighbours (n_list,) int32, counts (n, 33) int32 and spfh
    (n, 33) float32 by point, stable_spfh (n,) and stable (n_list,) bool, stats dict.
    order: "d2" = (d2, index), the contract; "index" = ascending index (a wrong build)."""
    pts = np.ascontiguousarray(points, f32)
    nrm = np.ascontiguousarray(normals, f32)[:, :3]
    n = len(pts)
    lst = np.arange(n) if idx is None else np.asarray(idx, np.int64)
    fin = np.isfinite(pts).all(1)
    ci = np.nonzero(fin)[0]
    r2 = f32(f64(f32(radius)) * f64(f32(radius)))
    d2 = flann_d2(pts[ci], pts[ci])
    nbr = d2 < r2
    m_c = nbr.sum(1)
    # ---- SPFH of every finite point
    I, J = np.nonzero(nbr)
    keep = I != J
    I, J = I[keep], J[keep]
    nfin = np.isfinite(nrm[ci]).all(1)
    both = nfin[I] & nfin[J]
    I, J = I[both], J[both]
    P, NP, Q, NQ = pts[ci][I], nrm[ci][I], pts[ci][J], nrm[ci][J]
    ok, f, sw = pair_features(P, NP, Q, NQ)
    b = np.stack([_bins_f1(f[:, 0]), _bins_unit(f[:, 1]), _bins_unit(f[:, 2])], 1)
    # stability: the swap at its two extremes, f1's bin at its two extremes
    _, _, sw_a = pair_features(P, NP, Q, NQ, ja=margin, jb=-margin)
    _, _, sw_b = pair_features(P, NP, Q, NQ, ja=-margin, jb=margin)
    _, f_up, _ = pair_features(P, NP, Q, NQ, jt=margin)
    _, f_dn, _ = pair_features(P, NP, Q, NQ, jt=-margin)
    st_pair = (sw_a == sw) & (sw_b == sw) & (_bins_f1(f_up[:, 0]) == b[:, 0]) & \
        (_bins_f1(f_dn[:, 0]) == b[:, 0])
    st_pair |= ~ok
    nc = len(ci)
    counts_c = np.zeros((nc, DIM), np.int64)
    for g in range(3):
        np.add.at(counts_c, (I[ok], BINS * g + b[ok, g]), 1)
    st_c = np.ones(nc, bool)
    np.logical_and.at(st_c, I, st_pair)
    spfh_c = bin_values(m_c, counts_c)
    pairs_c = counts_c[:, :BINS].sum(1)
    # ---- FPFH of the list entries
    pos = np.full(n, -1, np.int64)
    pos[ci] = np.arange(nc)
    e_fin = fin[lst]
    ec = pos[lst[e_fin]]  # the finite entries' rows of d2
    ne = len(ec)
    dd = d2[ec]
    nb_e = nbr[ec]
    m_e = nb_e.sum(1)
    mmax = int(m_e.max(initial=0))
    if order == "d2":
        key = (dd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
            ci.astype(np.uint64)[None, :]
    else:
        key = np.broadcast_to(ci.astype(np.uint64)[None, :], dd.shape).copy()
    key[~nb_e] = np.uint64(2**64 - 1)
    od = np.argsort(key, axis=1, kind="stable")[:, :mmax]
    hist = np.zeros((ne, DIM), f32)
    sums = np.zeros((ne, 3), f64)
    lo = np.full(ne, 1 << 20, np.int64)
    bad = np.zeros(ne, bool)
    st_e = np.ones(ne, bool)
    rows = np.arange(ne)
    with np.errstate(all="ignore"):
        for k in range(mmax):
            j = od[:, k]
            dk = dd[rows, j]
            live = (k < m_e) & (dk != 0)
            st_e &= st_c[j] | ~(k < m_e)
            w = (f32(1.0) / dk).astype(f32)
            val = (spfh_c[j] * w[:, None]).astype(f32)
            val = np.where(live[:, None], val, f32(0.0))
            hist = (hist + val).astype(f32)
            v3 = val.reshape(ne, 3, BINS).astype(f64)
            for bb in range(BINS):
                sums = sums + v3[:, :, bb]
            nz = val != 0
            bad |= (nz & ~(np.isfinite(val) & (val > 0))).any(1)
            l = _lo(np.where(nz & np.isfinite(val), np.abs(val), f32(1.0)))
            lo = np.minimum(lo, np.where(nz, l, 1 << 20).min(1))
        scale = (100.0 / sums).astype(f32)
        scale = np.where(sums != 0, scale, f32(1.0))
        hist = (hist.reshape(ne, 3, BINS) * scale[:, :, None]).astype(f32).reshape(ne, DIM)
    # the certificate of fpfh_model.hpp: every value a multiple of 2^lo, the largest sum (2^-16 to
    # spare) below 2^(lo + 53)
    with np.errstate(all="ignore"):
        limit = np.ldexp(1.0, np.where(lo == 1 << 20, 0, lo + 53).astype(np.int32))
        holds = ~bad & ((lo == 1 << 20) | (sums.max(1) * (1.0 + 2.0 ** -16) < limit))
    out = np.full((len(lst), DIM), np.nan, f32)
    out[e_fin] = hist
    nbo = np.full(len(lst), -1, np.int32)
    nbo[e_fin] = m_e
    stable = np.ones(len(lst), bool)
    stable[e_fin] = st_e
    counts = np.zeros((n, DIM), np.int32)
    counts[ci] = counts_c
    spfh = np.zeros((n, DIM), f32)
    spfh[ci] = spfh_c
    st_p = np.ones(n, bool)
    st_p[ci] = st_c
    stats = dict(n_finite=int(nc), n_nan_rows=int((~e_fin).sum()), n_zero_rows=int((m_e == 1).sum()),
                 max_neighbours=mmax, n_lds_overflow=int((m_e > CAP).sum()),
                 n_pairs=int(pairs_c[ec].sum()), n_pairs_failed=int((m_e - 1 - pairs_c[ec]).sum()),
                 n_sum_literal=int((~holds).sum()))
    return dict(hist=out, neighbours=nbo, counts=counts, spfh=spfh, stable_spfh=st_p,
                stable=stable, stats=stats)


# ---- normals for the cases: plain float64 PCA over the radius neighbours (any normals do: they are
# an input of the descriptors), NaN with fewer than 3 neighbours as the radius normals give
def pca_normals(points, radius):
    pts = np.ascontiguousarray(points, f32)
    fin = np.isfinite(pts).all(1)
    out = np.full((len(pts), 3), np.nan, f32)
    ci = np.nonzero(fin)[0]
    nb = flann_d2(pts[ci], pts[ci]) < f32(f64(f32(radius)) ** 2)
    P = pts[ci].astype(f64)
    for r, i in enumerate(ci):
        q = P[nb[r]]
        if len(q) < 3:
            continue
        c = q - q.mean(0)
        _, v = np.linalg.eigh(c.T @ c)
        nv = v[:, 0]
        out[i] = (nv if nv @ P[r] <= 0 else -nv).astype(f32)
    return out


# ---- the clouds of the cases (tests/golden/make_fpfh.py, tests/test_fpfh*.py) ------------------
def sphere_cloud(n=1200, seed=31):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * (1.0 + 0.05 * rng.normal(size=(n, 1)))).astype(f32)


def dense_cloud(seed=32):
    """a blob of 1,100 points, the central ones with more neighbours than CAP, on a sparse plane"""
    rng = np.random.default_rng(seed)
    blob = rng.normal(scale=0.038, size=(1100, 3)) * [1, 1, 0.2]
    plane = np.concatenate([rng.uniform(-1, 1, size=(500, 2)), 0.01 * rng.normal(size=(500, 1))], 1)
    return np.concatenate([blob, plane]).astype(f32)


def near_dup_cloud(shadow, radius, seed=33):
    """the scan plus 12 points at about radius / 30000 from existing ones"""
    rng = np.random.default_rng(seed)
    src = rng.choice(len(shadow), 12, replace=False)
    off = rng.normal(size=(12, 3))
    off *= (radius / 30000.0) / np.linalg.norm(off, axis=1, keepdims=True)
    return np.concatenate([shadow, (shadow[src].astype(f64) + off).astype(f32)])


def dups_nan_cloud(seed=34):
    rng = np.random.default_rng(seed)
    base = np.concatenate([rng.uniform(-1, 1, size=(300, 2)), 0.02 * rng.normal(size=(300, 1))], 1)
    pts = np.concatenate([base, base[:40], base[:10]]).astype(f32)  # exact duplicates, some twice
    pts[[5, 77, 301]] = np.nan
    pts[120, 1] = np.inf
    return pts


def thin_cloud(n=1200, seed=35):
    """wide and thin: 400 cells of the search grid along x, one across"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, 400, n), rng.uniform(0, 0.15, n),
                     0.01 * rng.normal(size=n)], 1).astype(f32)


def index_list(n, seed=36):
    rng = np.random.default_rng(seed)
    return rng.choice(n, 400, replace=True).astype(np.int32)


def cases(shadow):
    """name -> (points, normals radius, FPFH radius, index list or None)"""
    import dialog_amd.synth as synth
    planes = synth.plane_cloud(1500, 3)[0]
    return {
        "shadow": (shadow, 0.02, 0.05, None),
        "planes": (planes, 1.0, 1.5, None),
        "sphere": (sphere_cloud(), 0.2, 0.4, None),
        "dense": (dense_cloud(), 0.1, 0.1, None),
        "near_dup": (near_dup_cloud(shadow, 0.05), 0.02, 0.05, None),
        "dups_nan": (dups_nan_cloud(), 0.3, 0.3, None),
        "indices": (shadow, 0.02, 0.05, index_list(len(shadow))),
        "thin": (thin_cloud(), 1.0, 1.0, None),
    }
