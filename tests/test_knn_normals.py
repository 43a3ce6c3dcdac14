"""CPU: the k-NN normals oracle on the inputs of tests/knn_cases.py, so that the GPU tests
(tests/test_knn_normals_gpu.py) compare against a reference that is itself pinned:
  * the grid form of the oracle equals its brute-force definition, bit for bit, on the tie-heavy
    cloud, on the isolated groups and at the register-list boundaries k = 8 | 9, 32 | 33;
  * a row with a non-finite coordinate (NaN or +-inf) is PCL's !isFinite point: its normal is NaN
    and it is nobody's neighbour, so the finite rows get exactly the normals of the cloud without
    the bad rows;
  * fewer than 3 neighbours is NaN (k = 1, 2), 3 is enough;
  * the quantised cloud really has hundreds of queries whose k-th and (k+1)-th d2 tie.
"""
import numpy as np
import pytest

import knn_cases as K
from normals_ref import same_bits
from oracle import oracle as O


@pytest.mark.parametrize("case,k", [("quantised", 20), ("groups", 20), ("outliers", 8),
                                    ("outliers", 9), ("outliers", 32), ("outliers", 33)])
def test_oracle_grid_equals_brute(case, k):
    p = {"quantised": K.quantised, "groups": lambda: K.groups()[0], "outliers": K.outliers}[case]()
    g = O.estimate_normals_knn(p, k)
    b = O.estimate_normals_knn(p, k, brute=True)
    assert same_bits(g, b), int((g.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum())
    assert not np.isnan(b).any()


@pytest.mark.parametrize("case", ["non_finite", "inf25"])
def test_oracle_non_finite_rows_are_pcls_invalid_points(case):
    """pcl::isFinite rejects the query and KdTreeFLANN leaves the point out of the tree: +-inf
    rows as well as NaN rows.  (Before the oracle skipped candidates by their coordinates, the
    25-point cloud's 9 inf rows all got normals, its 16 finite rows took inf rows as neighbours
    at d = inf, and 1 of non_finite's 31 inf-only rows got a normal.)"""
    q = K.non_finite() if case == "non_finite" else K.inf_cloud()
    fin = K.finite_rows(q)
    assert (~fin).sum() == (54 if case == "non_finite" else 9)
    assert fin.sum() == (2146 if case == "non_finite" else 16)
    o = O.estimate_normals_knn(q, 20)
    assert np.isnan(o[~fin]).all()
    want = O.estimate_normals_knn(q[fin], 20)
    assert not np.isnan(want).any()
    assert same_bits(o[fin], want)
    # the grid form runs on the all-finite cloud; the definition agrees with it
    assert same_bits(O.estimate_normals_knn(q[fin], 20, brute=True), want)


def test_oracle_fewer_than_three_neighbours_is_nan():
    p = K.outliers()
    assert np.isnan(O.estimate_normals_knn(p, 1)).all()
    assert np.isnan(O.estimate_normals_knn(p, 2)).all()
    assert not np.isnan(O.estimate_normals_knn(p, 3)).any()


def kth_ties(p, k):
    """queries whose k-th and (k+1)-th smallest FLANN d2 = ((0 + dx^2) + dy^2) + dz^2 are equal"""
    n = 0
    for i in range(len(p)):
        d = p[i][None, :] - p
        d2 = ((np.float32(0) + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        s = np.partition(d2, (k - 1, k))
        n += int(s[k - 1] == s[k])
    return n


def test_quantised_cloud_has_ties_and_duplicates():
    """a condition on the input: the tie-break by index decides hundreds of neighbour lists"""
    p = K.quantised()
    assert p.dtype == np.float32 and p.shape == (4000, 3)
    _, counts = np.unique(p, axis=0, return_counts=True)
    assert len(counts) < len(p) and counts.max() >= 2
    for k in (8, 20, 32, 64):
        assert kth_ties(p, k) >= 500, k


def test_case_shapes():
    """the recipes keep their sizes (the GPU tests' thresholds are stated for them)"""
    assert K.outliers().shape == (2200, 3) and K.clean().shape == (2000, 3)
    p, lab = K.groups()
    assert p.shape == (3114, 3) and np.isfinite(p).all()
    assert [int((lab == j).sum()) for j in range(10)] == list(K.GROUP_SIZES)
    ext = p.max(axis=0) - p.min(axis=0)
    assert np.all(ext > 300) and np.all(ext < 1000)
    names = [n for n, _ in K.tiny()]
    assert len(names) == 11 and len(set(names)) == 11
    assert all(c.dtype == np.float32 and c.shape[1] == 3 for _, c in K.tiny())
