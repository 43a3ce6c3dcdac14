"""Inputs of the k-NN normals tests (tests/test_knn_normals.py keeps the oracle honest on them on
the CPU; tests/test_knn_normals_gpu.py compares the library with the oracle on them).  Small,
deterministic, numpy and dialog_amd.synth.plane_cloud only.  Every function returns a fresh
float32 [n, 3] array (callers may write into it)."""
from __future__ import annotations

import functools

import numpy as np

from dialog_amd.synth import plane_cloud

f32 = np.float32

# the ten isolated groups of groups(): the sizes sit on the level-0 kernel's thresholds at k = 20
# (20 resolves inside its group: cnt < K defers; 19 defers by one level; 5 is the first size with
# cnt * 4 < K false; 1..4 take the level-0 jump)
GROUP_SIZES = (1, 2, 4, 5, 19, 20, 21, 3, 19, 20)
TINY_PREFIXES = (1, 2, 3, 4, 19, 20, 21)
TINY_BLOBS = (5, 20, 40)


@functools.lru_cache(maxsize=None)
def _outliers():
    p, _, _ = plane_cloud(2000, 3, outlier_frac=0.05, seed=9, patch=2.0)
    far = np.random.default_rng(19).uniform(-6.0, 6.0, size=(200, 3)).astype(f32)
    return np.concatenate([p, far]).astype(f32)


def outliers():
    """three planes, 5 % outliers in their box, 200 sparse points around them: 2,200 points"""
    return _outliers().copy()


def clean():
    """three planes, no outliers: the level-0 cell tuning reaches its target occupancy"""
    p, _, _ = plane_cloud(2000, 3, outlier_frac=0.0, seed=9, patch=2.0)
    return p.astype(f32)


def quantised():
    """coordinates rounded to 1/64: duplicate rows and many exact ties in d2, where the point
    index decides (test_knn_normals.py asserts the tie count)"""
    p, _, _ = plane_cloud(4000, 3, outlier_frac=0.05, seed=21, patch=1.5)
    return (np.round(p * 64) / 64).astype(f32)


def non_finite():
    """outliers() with 54 bad rows: NaN rows, rows with +inf in y, rows with -inf in z"""
    r = outliers()
    r[::97] = np.nan
    r[5::131, 1] = np.inf
    r[7::151, 2] = -np.inf
    return r


def finite_rows(p):
    return np.isfinite(p).all(axis=1)


def inf_cloud():
    """25 points of a plane pair, every third with x = +inf: 16 finite rows, fewer than k = 20"""
    p, _, _ = plane_cloud(3000, 2, outlier_frac=0.0, seed=5, patch=2.0)
    q = p[:25].astype(f32).copy()
    q[::3, 0] = np.inf
    return q


def tiny():
    """[(name, cloud)]: clouds around and below k = 20, and the inf cloud"""
    c = clean()
    out = [("prefix%d" % n, c[:n].copy()) for n in TINY_PREFIXES]
    out += [("blob%d" % n, np.random.default_rng(3).normal(size=(n, 3)).astype(f32))
            for n in TINY_BLOBS]
    out.append(("inf25", inf_cloud()))
    return out


@functools.lru_cache(maxsize=None)
def _groups():
    base, _, _ = plane_cloud(3000, 2, outlier_frac=0.0, seed=5, patch=2.0)
    rng = np.random.default_rng(23)
    parts, labels = [base.astype(np.float64)], [np.full(len(base), -1, np.int32)]
    for j, s in enumerate(GROUP_SIZES):
        centre = np.array([50.0 * (j + 1) * (-1) ** j, 37.0 * (j + 1),
                           -29.0 * (j + 1) * (-1) ** (j // 2)])
        parts.append(centre + rng.normal(0.0, 0.01, size=(s, 3)))
        labels.append(np.full(s, j, np.int32))
    p = np.concatenate(parts).astype(f32)
    lab = np.concatenate(labels)
    perm = rng.permutation(len(p))
    return p[perm], lab[perm]


def groups():
    """-> (cloud [3114, 3], label [3114]: -1 the two base planes, j the j-th isolated group).  Ten
    tight groups (sigma 0.01) tens of units apart and away from the planes: the extent (about
    950 x 371 x 522) plans a deep hierarchy, and a group's members find their 20 neighbours
    inside the group, one level up or several levels up, by its size."""
    p, lab = _groups()
    return p.copy(), lab.copy()
