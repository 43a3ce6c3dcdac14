"""numpy restatement of pcl::StatisticalOutlierRemoval<PointXYZ>::applyFilterIndices (PCL 1.8, from
memory: parity unpinned), independent of the C code: every float32 operation is
written out and rounded on its own, in the order the semantics list them.

    the search structure: every finite point of the cloud, listed or not
    a non-finite list entry: distance 0.0f, not valid
    else d2 = the mean_k + 1 smallest ((0 + dx^2) + dy^2) + dz^2 (float32) over the finite points,
    ascending (brute force: a chunked d2 matrix, np.partition + np.sort); column 0 dropped
    distance = float32(sequential double sum of float32 sqrt(d2[k]) / mean_k)
    sum, sq_sum: sequential double sums of the distances and of their float32 squares, list order
    mean = sum / valid; variance = (sq_sum - sum * sum / valid) / (valid - 1)
    threshold = mean + mul * sqrt(variance)
    removed: double(distance) > threshold  (negative: <=); kept / removed = index values, list order
"""
import numpy as np

f32 = np.float32


class TooFewPoints(ValueError):
    pass


def flann_d2(q, p):
    """q (a, 3), p (b, 3) float32 -> (a, b) float32, each operation rounded to float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        acc = np.zeros((len(q), len(p)), f32)
        for a in range(3):
            e = (q[:, a, None] - p[None, :, a]).astype(f32)
            acc = (acc + (e * e).astype(f32)).astype(f32)
    return acc


def knn_d2(pts, queries, k, chunk=512):
    """the k smallest d2 from every query to the points, ascending: (len(queries), k) float32"""
    out = np.empty((len(queries), k), f32)
    for s in range(0, len(queries), chunk):
        d = flann_d2(queries[s:s + chunk], pts)
        # (np.sort of the k smallest: the partition only spares sorting the rest of each row)
        out[s:s + chunk] = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1)
    return out


def seq_sum(terms, order="asc"):
    """the literal chain over the rows of float32 terms -> float64 per row"""
    t = terms.astype(np.float64)
    if order == "desc":
        t = t[:, ::-1]
    return np.cumsum(t, axis=1)[:, -1]


def sor_ref(points, mean_k, stddev_mul, idx=None, negative=False, order="asc", sqrt_double=False):
    """order / sqrt_double: the two wrong builds (descending per-query sum, sqrt in double)"""
    p = np.ascontiguousarray(points, f32).reshape(-1, 3)
    n = len(p)
    lst = np.arange(n, dtype=np.int64) if idx is None else np.asarray(idx, np.int64)
    fin_pt = np.isfinite(p).all(1)
    cloud = p[fin_pt]
    n_finite = len(cloud)
    if n_finite < mean_k + 1:
        raise TooFewPoints("fewer than mean_k + 1 finite points")
    m = len(lst)
    valid = fin_pt[lst] if m else np.zeros(0, bool)
    # one search per distinct valid point of the list
    uniq, inv = np.unique(lst[valid], return_inverse=True)
    d2 = knn_d2(cloud, p[uniq], mean_k + 1)[:, 1:]
    with np.errstate(over="ignore"):
        if sqrt_double:
            s = np.cumsum(np.sqrt(d2.astype(np.float64)), axis=1)[:, -1]
        else:
            s = seq_sum(np.sqrt(d2).astype(f32), order)
        du = (s / np.float64(mean_k)).astype(f32)
    dist = np.zeros(m, f32)
    dist[valid] = du[inv.reshape(-1)]
    with np.errstate(all="ignore"):
        sum_ = np.cumsum(dist.astype(np.float64))[-1] if m else np.float64(0)
        sq = (dist * dist).astype(f32)
        sq_sum = np.cumsum(sq.astype(np.float64))[-1] if m else np.float64(0)
        nv = np.float64(int(valid.sum()))
        mean = sum_ / nv
        variance = (sq_sum - sum_ * sum_ / nv) / (nv - np.float64(1.0))
        stddev = np.sqrt(variance)
        threshold = mean + np.float64(stddev_mul) * stddev
        d64 = dist.astype(np.float64)
        removed_mask = (d64 <= threshold) if negative else (d64 > threshold)
    return {
        "distances": dist, "sum": float(sum_), "sq_sum": float(sq_sum), "mean": float(mean),
        "stddev": float(stddev), "threshold": float(threshold),
        "kept": lst[~removed_mask].astype(np.int32), "removed": lst[removed_mask].astype(np.int32),
        "n_finite": int(n_finite), "n_valid": int(valid.sum()), "d2": d2, "uniq": uniq,
    }


# ---- the certificate, restated with Python integers -----------------------------------------------
def _sig_exp(t):
    """a finite float32 >= 0 as (integer significand, exponent)"""
    u = int(np.asarray(t, f32).view(np.uint32)) & 0x7FFFFFFF
    e, mnt = u >> 23, u & 0x7FFFFF
    return ((mnt | 0x800000) if e else mnt), (e if e else 1) - 150


def certificate(terms):
    """-> (certified, exact sum as float or None): Q = the lowest set bit over the non-zero terms;
    certified when the integer sum of term / Q is below 2^53"""
    terms = np.asarray(terms, f32)
    if not np.isfinite(terms).all():
        return False, None
    se = [_sig_exp(t) for t in terms if t != 0]
    if not se:
        return True, 0.0
    q = min(e + ((s & -s).bit_length() - 1) for s, e in se)
    total = sum((s << (e - q)) if e >= q else (s >> (q - e)) for s, e in se)  # (exact shifts)
    if total >= 2**53:
        return False, None
    return True, float(np.ldexp(np.float64(total), q))


# ---- fixtures -------------------------------------------------------------------------------------
def cluster_cloud():
    rng = np.random.RandomState(11)
    n = 4096
    A = rng.uniform(-5, 5, (n, 3)).astype(f32)
    A[:3000, 2] = rng.normal(0, 0.005, 3000).astype(f32)
    A[3000:3040] = (rng.uniform(-1, 1, (40, 3)) * np.logspace(-9, -7, 40)[:, None]).astype(f32)
    return A


def deferral_cloud():
    rng = np.random.RandomState(5)
    n = 8192
    A = np.empty((n, 3), f32)
    A[:, :2] = rng.uniform(-2, 2, (n, 2)).astype(f32)
    A[:, 2] = rng.normal(0, 0.003, n).astype(f32)
    A[-64:] = rng.uniform(-40, 40, (64, 3)).astype(f32)
    return A
