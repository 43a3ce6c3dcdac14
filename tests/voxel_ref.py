"""numpy restatement of pcl::VoxelGrid<PointXYZ>::applyFilter (PCL 1.8, from memory: parity
unpinned), independent of the C code: every float32 operation is written out and
rounded on its own, in the order the semantics list them.

    inv[a] = 1.0f / leaf[a]
    finite entries only; min_p / max_p over them; none: 0 voxels
    d[a] = (int64)((max_p[a] - min_p[a]) * inv[a]) + 1; d0 * d1 * d2 > INT32_MAX: LeafTooSmall
    min_b[a] = (int)floorf(min_p[a] * inv[a]), max_b likewise (outside int: OutOfIntRange)
    div = max_b - min_b + 1; mul = (1, div0, div0 * div1)
    ijk[a] = (int)(floorf(p[a] * inv[a]) - (float)min_b[a]); key = sum ijk * mul  (uint32)
    stable sort by key (list order inside a voxel: our choice, PCL's std::sort leaves it open)
    voxels of fewer than min_points entries dropped
    centroid = three sequential float chains over the members in order, / (float)count
"""
import numpy as np

INT32_MAX = 2**31 - 1
f32 = np.float32


class LeafTooSmall(ValueError):
    pass


class OutOfIntRange(ValueError):
    pass


def grid(mn, mx, leaf):
    """-> (inv float32[3], min_b int64[3], div int64[3]); raises the two verdicts."""
    leaf = np.broadcast_to(np.asarray(leaf, f32), (3,))
    inv = (f32(1) / leaf).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = ((mx - mn).astype(f32) * inv).astype(f32)
    d = []
    for v in t:
        if not v < f32(2**31):  # (an infinite extent or product: over any limit)
            raise LeafTooSmall("leaf size too small")
        d.append(int(v) + 1)  # int(): truncation
    if d[0] * d[1] * d[2] > INT32_MAX:
        raise LeafTooSmall("leaf size too small")
    with np.errstate(over="ignore"):
        lo = np.floor((mn * inv).astype(f32))
        hi = np.floor((mx * inv).astype(f32))
    for v in list(lo) + list(hi):
        if not (-2.0**31 <= float(v) < 2.0**31):
            raise OutOfIntRange("floorf(coordinate / leaf) outside the int range")
    min_b = lo.astype(np.int64)
    div = hi.astype(np.int64) - min_b + 1
    if (div > INT32_MAX).any():
        raise LeafTooSmall("leaf size too small")
    return inv, min_b, div


def keys_of(q, inv, min_b, div):
    """uint32 keys of the finite points q (float32 [m, 3])."""
    mul = np.array([1, div[0], div[0] * div[1]], np.int64) & 0xFFFFFFFF
    cell = np.floor((q * inv).astype(f32))
    ijk = (cell - min_b.astype(f32)).astype(f32).astype(np.int64)
    return ((ijk * mul).sum(1) & 0xFFFFFFFF).astype(np.uint32)


def chain_sums(q, starts, ends):
    """per run [s, e) of q (float32 [m, 3], already in summing order): the three sequential float32
    chains, vectorised over the runs (step j adds member j of every run that has one)."""
    nv = len(starts)
    acc = np.zeros((nv, 3), f32)
    cnt = ends - starts
    order = np.argsort(-cnt, kind="stable")  # longest first: the active runs are a prefix
    s_o, c_o = starts[order], cnt[order]
    a_o = np.zeros((nv, 3), f32)
    for j in range(int(cnt.max()) if nv else 0):
        k = int(np.searchsorted(-c_o, -j, side="left"))  # runs with cnt > j
        a_o[:k] = (a_o[:k] + q[s_o[:k] + j]).astype(f32)
    acc[order] = a_o
    return acc


def voxel_ref(p, leaf, idx=None, min_points=0, order="asc", key_double=False):
    """-> dict(xyz float32 [k, 3], counts int32 [k], voe int32 [n], keys uint32 [k], div, min_b,
    n_finite, n_voxels).  order="desc" and key_double=True are the two WRONG variants the tests
    must tell from the right one (members summed in reverse; keys from double arithmetic)."""
    p = np.ascontiguousarray(p, f32)[:, :3]
    idx = np.arange(len(p), dtype=np.int64) if idx is None else np.asarray(idx, np.int64)
    n = len(idx)
    empty = dict(xyz=np.zeros((0, 3), f32), counts=np.zeros(0, np.int32),
                 voe=np.full(n, -1, np.int32), keys=np.zeros(0, np.uint32), div=None, min_b=None,
                 n_finite=0, n_voxels=0)
    if n == 0:
        return empty
    q = p[idx]
    fin = np.isfinite(q).all(1)
    if not fin.any():
        return empty
    pos = np.flatnonzero(fin)
    qf = q[pos]
    inv, min_b, div = grid(qf.min(0), qf.max(0), leaf)
    if key_double:
        lf = np.broadcast_to(np.asarray(leaf, np.float64), (3,))
        ijk = (np.floor(qf.astype(np.float64) / lf) - min_b).astype(np.int64)
        mul = np.array([1, div[0], div[0] * div[1]], np.int64)
        key = ((ijk * mul).sum(1) & 0xFFFFFFFF).astype(np.uint32)
    else:
        key = keys_of(qf, inv, min_b, div)
    o = np.argsort(key, kind="stable")
    ks, ps = key[o], pos[o]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    ends = np.r_[starts[1:], len(ks)]
    cnt = ends - starts
    qs = q[ps]
    if order == "desc":  # (wrong on purpose: each run reversed)
        rev = np.concatenate([np.arange(e - 1, s - 1, -1) for s, e in zip(starts, ends)])
        qs = qs[rev]
    sums = chain_sums(qs, starts, ends)
    keep = cnt >= min_points
    rows = np.cumsum(keep) - 1
    xyz = (sums[keep] / cnt[keep].astype(f32)[:, None]).astype(f32)
    voe = np.full(n, -1, np.int32)
    vox_of_sorted = np.repeat(np.arange(len(starts)), cnt)
    voe[ps] = np.where(keep[vox_of_sorted], rows[vox_of_sorted], -1).astype(np.int32)
    return dict(xyz=xyz, counts=cnt[keep].astype(np.int32), voe=voe, keys=ks[starts][keep],
                div=div.astype(np.int32), min_b=min_b.astype(np.int32), n_finite=int(len(pos)),
                n_voxels=int(len(starts)))


# ---- the fixtures the CPU and the GPU tests share ---------------------------------------------
def uniform_cloud(n=20000, seed=7):
    """uniform in [-2, 2)^3 (leaf 0.25: 4067 voxels of 1..17 points at n = 20000)"""
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3), dtype=f32) * 4 - 2).astype(f32)


def quantised_cloud(n=20000, seed=7):
    """the uniform cloud rounded to multiples of 0.1f (leaf 0.1: floorf((x * inv)_f32) differs from
    a double floor(x * 10) for most points, so a double-precision key fails on it)"""
    p = uniform_cloud(n, seed)
    return (np.round(p / f32(0.1)) * f32(0.1)).astype(f32)


LADDER = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000)


def ladder_cloud(seed=3):
    """voxels (leaf 1, one per integer x cell) holding exactly LADDER[i] points, shuffled; the
    coordinates spread over the cell and of mixed magnitude so the sums round at every step"""
    rng = np.random.default_rng(seed)
    parts = []
    for i, c in enumerate(LADDER):
        q = rng.random((c, 3), dtype=f32) * f32(0.98) + f32(0.01)
        q[:, 0] += f32(i)
        q[:, 1] *= f32(1e-3)  # (small terms added to a large running sum)
        parts.append(q)
    p = np.concatenate(parts).astype(f32)
    return p[rng.permutation(len(p))]
