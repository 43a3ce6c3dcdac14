"""GPU: estimate_normals(k=...) against the oracle at every k, on ties, non-finite rows, tiny
clouds and clouds that send queries up the grid hierarchy (inputs: tests/knn_cases.py; the oracle
on them is pinned on the CPU by tests/test_knn_normals.py).

The rule in PCL-float mode: bit-equal where the oracle is finite, NaN exactly where the oracle is
NaN (normals_ref.same_bits; a NaN's payload is not pinned).  No ulp allowance: with the same
(d2, index)-ordered neighbour list everything after it is the float arithmetic the random-cloud
tests of test_normals.py already match bit for bit.  Double mode is held to the float64
restatement under test_gpu_knn_normals' rule.  dlg_knn_stats (Context.knn_stats) tells which
levels of the hierarchy a call used, so the tests assert the paths they mean to run."""
import functools

import numpy as np
import pytest

import dialog_amd as D
import knn_cases as K
from normals_ref import angle, f64_normals, knn_sets, same_bits
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CASES = {"outliers": K.outliers, "clean": K.clean, "quantised": K.quantised,
         "non_finite": K.non_finite}


@functools.lru_cache(maxsize=None)
def case(name):
    p = CASES[name]()
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def oracle_knn(name, k):
    o = O.estimate_normals_knn(case(name), k)
    o.setflags(write=False)
    return o


def n_diff(g, o):
    return int(((g.view(np.uint32) != o.view(np.uint32)) & ~(np.isnan(g) & np.isnan(o)))
               .any(axis=1).sum())


# ------------------------------------------------------------------------------------- every k
# one group per instantiation of k_normals_knn<KP> (KP = 8, 16, 24, 32, 64); k = 1, 2 have fewer
# than 3 neighbours
K_GROUPS = {"1-2": range(1, 3), "3-8": range(3, 9), "9-16": range(9, 17), "17-24": range(17, 25),
            "25-32": range(25, 33), "33-64": range(33, 65)}


@pytest.mark.parametrize("name", ["outliers", "clean"])
@pytest.mark.parametrize("group", list(K_GROUPS))
def test_every_k_bit_exact(gpu_ctx, name, group):
    p = case(name)
    for k in K_GROUPS[group]:
        g = D.estimate_normals(p, k=k, ctx=gpu_ctx)
        o = oracle_knn(name, k)
        assert same_bits(g, o), (name, k, n_diff(g, o))
        assert np.isnan(g).all() if k < 3 else not np.isnan(g).any(), (name, k)
        st = gpu_ctx.knn_stats()
        assert st["valid"] and st["k"] == k and st["n"] == len(p) and st["queries"][0] == len(p)


@pytest.mark.parametrize("k", [8, 9, 16, 17, 24, 25, 32, 33])
def test_double_mode_at_the_template_boundaries(gpu_ctx, k):
    """mode "double" on both sides of every register-list boundary, against the float64
    restatement under test_normals.py::test_gpu_knn_normals' rule"""
    p = case("outliers")
    g = D.estimate_normals(p, k=k, ctx=gpu_ctx, mode="double")
    ref, gap = f64_normals(p, knn_sets(p, k))
    ok = gap > 1e-3
    assert ok.sum() > 0.9 * len(p)
    assert not np.isnan(g).any()
    a = angle(g[ok], ref[ok])
    assert a.max() < 1e-5, (k, a.max())
    np.testing.assert_allclose(g[ok, 3], ref[ok, 3], rtol=1e-4, atol=1e-7)


# ------------------------------------------------------------------------ ties and duplicates
@pytest.mark.parametrize("k", [8, 20, 32, 64])
def test_ties_and_duplicates_bit_exact(gpu_ctx, k):
    """coordinates on a 1/64 lattice: ~950 of the 4,000 queries tie at the k-th place and rows
    repeat up to 3-fold, so the index decides the neighbour list (and its order, hence the sums)"""
    p = case("quantised")
    g = D.estimate_normals(p, k=k, ctx=gpu_ctx)
    o = oracle_knn("quantised", k)
    assert not np.isnan(o).any()
    assert same_bits(g, o), (k, n_diff(g, o))


# ------------------------------------------------------------------------------ non-finite rows
@pytest.mark.parametrize("via", ["host", "cloud"])
@pytest.mark.parametrize("mode", ["pcl", "double"])
def test_non_finite_rows(gpu_ctx, mode, via):
    """NaN, +inf and -inf rows: a NaN normal each, and invisible to the finite rows, which get
    the bits of the call on the cloud without them (and, PCL-float, the oracle's bits)"""
    q = case("non_finite")
    fin = K.finite_rows(q)
    assert (~fin).sum() == 54

    def run(pts):
        if via == "host":
            return D.estimate_normals(pts, k=20, ctx=gpu_ctx, mode=mode)
        cl = D.Cloud(gpu_ctx, pts)
        try:
            return cl.estimate_normals(k=20, mode=mode, copy_out=True)
        finally:
            cl.close()

    g = run(q)
    assert np.isnan(g[~fin]).all()
    assert not np.isnan(g[fin]).any()
    st = gpu_ctx.knn_stats()
    assert st["valid"] and st["n"] == len(q) and st["queries"][0] == len(q)
    own = run(np.ascontiguousarray(q[fin]))
    assert np.array_equal(g[fin].view(np.uint32), own.view(np.uint32)), n_diff(g[fin], own)
    if mode == "pcl":
        o = oracle_knn("non_finite", 20)
        assert same_bits(g, o), n_diff(g, o)


# ---------------------------------------------------------------------------------- tiny clouds
def test_tiny_clouds(gpu_ctx):
    """n <= k, n just above k, and 16 finite rows among 25.  Across the set the hierarchy is a
    single level at least once -- the only route to the per-thread kernel without the level-0
    histogram variant -- and deeper at least once.  Seen on the MI355X: one level for prefix2,
    3, 4, 19, 20, 21, blob5 and inf25; 6 levels for prefix1, 2 for blob20 and blob40 (DESIGN.md,
    "Which levels a k-NN call used")."""
    planned = {}
    for name, p in K.tiny():
        g = D.estimate_normals(p, k=20, ctx=gpu_ctx)
        o = O.estimate_normals_knn(p, 20)
        assert same_bits(g, o), (name, n_diff(g, o))
        st = gpu_ctx.knn_stats()
        assert st["valid"] and st["k"] == 20 and st["n"] == len(p) and st["queries"][0] == len(p)
        assert st["built"][0] == 1 and 1 <= st["levels_planned"] <= 12
        planned[name] = st["levels_planned"]
        fin = K.finite_rows(p)
        if fin.sum() < 3:
            assert np.isnan(g).all(), name
        else:
            assert np.isnan(g[~fin]).all() and not np.isnan(g[fin]).any(), name
    print("levels_planned:", planned)
    assert any(v == 1 for v in planned.values()), planned
    assert any(v > 1 for v in planned.values()), planned
    # the inf cloud: fewer finite rows (16) than k, so every finite row uses exactly those 16
    q = K.inf_cloud()
    fin = K.finite_rows(q)
    assert fin.sum() == 16
    g = D.estimate_normals(q, k=20, ctx=gpu_ctx)
    for k in (16, 20):
        own = D.estimate_normals(np.ascontiguousarray(q[fin]), k=k, ctx=gpu_ctx)
        assert np.array_equal(g[fin].view(np.uint32), own.view(np.uint32)), k
    assert same_bits(g[fin], O.estimate_normals_knn(q[fin], 16))


# --------------------------------------------------------------------------------------- levels
def test_groups_defer_and_skip_levels(gpu_ctx):
    """Ten tight groups far from two planes and from each other, k = 20: a group of 20 or 21
    resolves inside itself at level 0, one of 5 or 19 defers level by level, one of 1..4 jumps
    three levels from level 0; level 1's own deferrals then skip level 2, which nothing was sent
    to, so it is never built.

    The record seen on the MI355X: 12 planned levels, queries [3114, 43, 0, 53, 53, 53, 53, 53,
    53, 52, 50, 3], built [1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1] ("Which levels a k-NN
    call used")."""
    p, lab = K.groups()
    n = len(p)
    g = D.estimate_normals(p, k=20, ctx=gpu_ctx)
    st = gpu_ctx.knn_stats()
    print("knn_stats:", st)
    o = O.estimate_normals_knn(p, 20)
    assert not np.isnan(o).any()
    assert same_bits(g, o), n_diff(g, o)
    # oracle-free: a group that holds its own 20 neighbours gives the same (d2, index) lists alone
    for j, size in enumerate(K.GROUP_SIZES):
        if size < 20:
            continue
        rows = np.flatnonzero(lab == j)  # cloud order
        alone = D.estimate_normals(np.ascontiguousarray(p[rows]), k=20, ctx=gpu_ctx)
        assert np.array_equal(g[rows].view(np.uint32), alone.view(np.uint32)), j
    # the record
    g2 = D.estimate_normals(p, k=20, ctx=gpu_ctx)
    st2 = gpu_ctx.knn_stats()
    assert np.array_equal(g.view(np.uint32), g2.view(np.uint32)) and st2 == st
    assert st["valid"] and st["k"] == 20 and st["n"] == n
    q, built, m = st["queries"], st["built"], st["levels_planned"]
    assert m >= 6 and len(q) == m and len(built) == m
    assert q[0] == n and built[0] == 1
    used = [l for l in range(m) if q[l] > 0]
    assert len(used) >= 3, q
    assert all(built[l] == 1 for l in used), (q, built)
    assert all(0 <= q[l] <= n for l in range(m))
    skipped = [l for l in range(used[0] + 1, used[-1]) if q[l] == 0 and built[l] == 0]
    assert skipped, (q, built)
    # what level 0 must send on: every member of a group smaller than 20 (73 points), and the
    # members of the groups of 1..4 (10 points) go three levels up, not to level 1
    small = sum(s for s in K.GROUP_SIZES if s < 20)
    jumpers = sum(s for s in K.GROUP_SIZES if s * 4 < 20)
    assert q[1] >= small - jumpers and q[3] >= jumpers, q


# -------------------------------------------------------------------------------- stats hygiene
def test_knn_stats_hygiene():
    p = case("clean")
    ctx = D.Context(0)
    try:
        st0 = ctx.knn_stats()
        assert not st0["valid"] and st0["levels_planned"] == 0 and st0["queries"] == []
        D.estimate_normals(p, radius=0.1, ctx=ctx)
        assert ctx.knn_stats() == st0  # a radius call leaves the record alone
        D.estimate_normals(p, k=8, ctx=ctx)
        st8 = ctx.knn_stats()
        D.estimate_normals(p, k=20, ctx=ctx)
        st20 = ctx.knn_stats()
        assert st8["valid"] and st20["valid"] and st8["k"] == 8 and st20["k"] == 20
        assert st8 != st20 and st8["n"] == st20["n"] == len(p)
        D.estimate_normals(p, radius=0.1, ctx=ctx)
        assert ctx.knn_stats() == st20
        # the cloud entry point fills the same record
        cl = D.Cloud(ctx, p)
        try:
            cl.estimate_normals(k=8)
        finally:
            cl.close()
        assert ctx.knn_stats() == st8
        with pytest.raises(D.DialogError):
            D.estimate_normals(p, k=65, ctx=ctx)  # refused before any search: record kept
        assert ctx.knn_stats() == st8
    finally:
        ctx.close()


def test_knn_stats_on_a_two_rank_group():
    """a context of a 2-rank group: the cloud call is refused there (the cloud is a shard), so no
    search runs and the record stays invalid on both ranks"""
    p = case("clean")
    ctxs = D.Context.loopback_group(2, 0)
    try:
        cl = D.Cloud(ctxs[0], p[:1000], id_base=0)
        try:
            with pytest.raises(D.DialogError) as ei:
                cl.estimate_normals(k=20)
            assert ei.value.status == 1 and "world > 1" in str(ei.value)
        finally:
            cl.close()
        for c in ctxs:
            assert not c.knn_stats()["valid"]
    finally:
        for c in ctxs:
            c.close()
