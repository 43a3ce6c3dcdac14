"""dlg_cloud_signature (k_signature, kernels.hip): the 64-bit content signature of a cloud as
uploaded, against a numpy restatement of the header's definition in wrapping uint64 arithmetic on
the points' bit patterns, so equality is exact.

The signature is the piece the multi-rank driver's automatic sharding decision (DLG_OPT_HYP_SHARD
-1) lacks: that decision compares counts, id_base and extents only.  The tests here
pin the kernel: sizes around the wave, block and grid limits, NaN payloads, +-inf and +-0.0, the
16-byte-stride layout, index lists through both upload gathers, two id_base values, and that
every single-point edit, swap, id_base change and index permutation changes the value.
"""
import numpy as np
import pytest

import dialog_amd as D


def np_signature(xyz, gid):
    """include/dialog_ransac.h's definition of dlg_cloud_signature, in wrapping uint64 arrays."""
    b = np.ascontiguousarray(xyz, np.float32)[:, :3].copy().view(np.uint32).astype(np.uint64)
    g = np.ascontiguousarray(gid, np.int32).view(np.uint32).astype(np.uint64)
    s32, s29 = np.uint64(32), np.uint64(29)
    h = (np.arange(b.shape[0], dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    h ^= b[:, 0] | (b[:, 1] << s32)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> s29
    h ^= b[:, 2] | (g << s32)
    h *= np.uint64(0x94D049BB133111EB)
    h ^= h >> s32
    return int(h.sum(dtype=np.uint64))


def gpu_signature(ctx, xyz, indices=None, id_base=0):
    c = D.Cloud(ctx, xyz, indices=indices, id_base=id_base)
    try:
        return c.signature()
    finally:
        c.close()


def expected_signature(xyz, indices=None, id_base=0):
    xyz = np.asarray(xyz, np.float32)
    k = np.arange(xyz.shape[0]) if indices is None else np.asarray(indices, np.int64)
    return np_signature(xyz[k], (id_base + k).astype(np.int32))


def random_points(n, seed=7):
    return np.random.default_rng(seed).normal(0.0, 3.0, (n, 3)).astype(np.float32)


def special_points(n=257):
    """random points with NaN (two payloads), +-inf and +-0.0 among them"""
    p = random_points(n, seed=11)
    bits = p.view(np.uint32)
    bits[3, 0] = 0x7FC00000   # quiet NaN
    bits[4, 1] = 0x7FC00001   # ... another payload
    bits[5, 2] = 0xFFC12345   # negative NaN with a payload
    bits[6, 0] = 0x7F800000   # +inf
    bits[7, 1] = 0xFF800000   # -inf
    bits[8, 2] = 0x00000000   # +0.0
    bits[9, 2] = 0x80000000   # -0.0
    bits[n - 1, 0] = 0x80000000
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 100003, 300001])
@pytest.mark.parametrize("id_base", [0, 1000])
def test_signature_matches_numpy(gpu_ctx, n, id_base):
    """random float32 points, packed and in the 16-byte-stride layout: the device's sum is the
    numpy restatement's, exactly (one wave, one block, more than one block; 300001 points are
    more than the 1024 x 256 threads of the largest grid: the grid-stride loop)"""
    p = random_points(n)
    want = expected_signature(p, id_base=id_base)
    assert (want == 0) == (n == 0)
    assert gpu_signature(gpu_ctx, p, id_base=id_base) == want
    p4 = np.concatenate([p, np.full((n, 1), 1.0, np.float32)], axis=1)  # pcl::PointXYZ records
    assert gpu_signature(gpu_ctx, p4, id_base=id_base) == want


@pytest.mark.gpu
@pytest.mark.parametrize("id_base", [0, 1000])
def test_signature_special_values_and_indices(gpu_ctx, id_base):
    """NaN payloads, +-inf and +-0.0 are hashed by their bits; index lists go through both upload
    gathers (device for 4 * n >= N, host below it), in any order and with duplicates"""
    p = special_points()
    assert gpu_signature(gpu_ctx, p, id_base=id_base) == expected_signature(p, id_base=id_base)
    big = random_points(100003, seed=13)
    rng = np.random.default_rng(5)
    for m in (30000, 25001, 25000, 1000, 1):  # 4 * 25001 >= 100003 > 4 * 25000: the switch
        idx = rng.integers(0, big.shape[0], m).astype(np.int32)
        assert gpu_signature(gpu_ctx, big, idx, id_base) == expected_signature(big, idx, id_base), m
    sp = np.array([9, 8, 3, 4, 5, 256, 0, 8], np.int32)  # (host gather: 4 * 8 < 257)
    assert gpu_signature(gpu_ctx, p, sp, id_base) == expected_signature(p, sp, id_base)
    dev = np.concatenate([np.arange(257)[::-1], sp]).astype(np.int32)  # (device gather)
    assert gpu_signature(gpu_ctx, p, dev, id_base) == expected_signature(p, dev, id_base)


@pytest.mark.gpu
def test_signature_changes_with_every_edit(gpu_ctx):
    """one flipped mantissa bit in x, y or z of the first, a middle and the last point, +0.0 ->
    -0.0, two points swapped, another id_base, permuted indices: each changes the signature (and
    each edited cloud's signature is still the restatement's); the same cloud uploaded twice, and
    on a second context, gives the same value"""
    n = 1000
    p = random_points(n, seed=17)
    p[10, 1] = 0.0
    base = gpu_signature(gpu_ctx, p)
    assert base == expected_signature(p)
    assert gpu_signature(gpu_ctx, p) == base
    ctx2 = D.Context(0)
    try:
        assert gpu_signature(ctx2, p) == base
    finally:
        ctx2.close()
    seen = {base}

    def edited(q, **kw):
        s = gpu_signature(gpu_ctx, q, **kw)
        assert s == expected_signature(q, **kw)
        assert s not in seen, kw
        seen.add(s)

    for i in (0, n // 2, n - 1):
        for k in range(3):
            q = p.copy()
            q.view(np.uint32)[i, k] ^= 1
            edited(q)
    q = p.copy()
    q.view(np.uint32)[10, 1] = 0x80000000
    edited(q)
    q = p.copy()
    q[[20, 700]] = q[[700, 20]]
    assert not np.array_equal(p[20], p[700])
    edited(q)
    edited(p, id_base=1)
    idx = np.arange(n, dtype=np.int32)
    assert gpu_signature(gpu_ctx, p, indices=idx) == base  # (the identity list: same points, same ids)
    perm = idx.copy()
    perm[[1, 2]] = perm[[2, 1]]
    edited(p, indices=perm)
    edited(p, indices=np.random.default_rng(3).permutation(n).astype(np.int32))
