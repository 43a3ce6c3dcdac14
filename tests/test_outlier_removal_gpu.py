"""GPU: dlg_statistical_outlier_removal / dlg_statistical_outlier_removal_cloud bit for bit against
tests/sor_ref.py (the numpy restatement of pcl::StatisticalOutlierRemoval's applyFilterIndices), at
every shape where the device path changes: the mean_k ladder across the register counts of
k_sor_knn, the literal and the certified sums, queries deferred up the grid hierarchy, clouds of
exactly mean_k + 1 points, non-finite points, index lists, strides, the status codes, and the
device-resident result as a cloud.

Run once against two wrong implementations (recorded in DESIGN.md §5f): the per-query sum in
descending order with the certificate disabled changes no float distance and fails only the two
DLG_OPT_SOR_LITERAL tests (the order itself is pinned by the host model test); sqrt evaluated in
double fails 22 of the 29 tests then written.

In every equality test the bits of the distances, of sum, sq_sum and threshold, the kept and
removed lists, n_finite and n_valid equal the reference's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dialog_amd as D
import sor_ref as S
from dialog_amd import _lib, pcd
from dialog_amd.sac import _f32p, _i32p
from dialog_amd.synth import plane_cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def dbits(x):
    return np.float64(x).view(np.uint64)


def raw_call(ctx, pts, mean_k, mul, idx=None, negative=0, cap=None, cap_removed=None,
             want_removed=True, want_dist=True, want_stats=True):
    """dlg_statistical_outlier_removal through ctypes"""
    L = _lib.load()
    a = np.ascontiguousarray(pts, f32)
    P = _lib.Points(_f32p(a), a.shape[0], 4 * a.shape[1])
    prm = _lib.SorParams(int(mean_k), int(negative), float(mul))
    ix = None if idx is None else np.ascontiguousarray(idx, np.int32)
    n = a.shape[0] if ix is None else ix.shape[0]
    cap = n if cap is None else cap
    cap_removed = n if cap_removed is None else cap_removed
    kept = np.full(max(cap, 1), -7, np.int32)
    rem = np.full(max(cap_removed, 1), -7, np.int32)
    dist = np.full(max(n, 1), -7.0, f32)
    nk, nr = C.c_int64(-1), C.c_int64(-1)
    st = _lib.SorStats()
    s = L.dlg_statistical_outlier_removal(
        ctx.h, C.byref(P), None if ix is None else _i32p(ix), n if ix is not None else 0,
        C.byref(prm), _i32p(kept), cap, C.byref(nk), _i32p(rem) if want_removed else None,
        cap_removed, C.byref(nr) if want_removed else None, _f32p(dist) if want_dist else None,
        C.byref(st) if want_stats else None)
    return dict(status=s, n_kept=nk.value, n_removed=nr.value, kept=kept, removed=rem,
                distances=dist[:n], stats=st)


def assert_equal(r, ref):
    assert r["status"] == 0
    st = r["stats"]
    assert np.array_equal(bits(r["distances"]), bits(ref["distances"]))
    assert dbits(st.sum) == dbits(ref["sum"]) and dbits(st.sq_sum) == dbits(ref["sq_sum"])
    assert dbits(st.threshold) == dbits(ref["threshold"]) or (
        np.isnan(st.threshold) and np.isnan(ref["threshold"]))
    assert r["n_kept"] == len(ref["kept"]) and r["n_removed"] == len(ref["removed"])
    assert np.array_equal(r["kept"][:r["n_kept"]], ref["kept"])
    assert np.array_equal(r["removed"][:r["n_removed"]], ref["removed"])
    assert st.n_finite == ref["n_finite"] and st.n_valid == ref["n_valid"]


def check_equal(ctx, pts, mean_k, mul, idx=None, negative=0):
    ref = S.sor_ref(np.ascontiguousarray(pts, f32)[:, :3], mean_k, mul, idx=idx,
                    negative=bool(negative))
    r = raw_call(ctx, pts, mean_k, mul, idx, negative)
    assert r["status"] == 0, _lib.load().dlg_last_error(ctx.h)
    assert_equal(r, ref)
    return r, ref


@pytest.fixture(scope="module")
def shadow():
    return np.ascontiguousarray(
        pcd.read_pcd(os.path.join(ROOT, "tests", "golden", "double_shadow.pcd"))[:, :3], f32)


@pytest.fixture(scope="module")
def cluster():
    A = S.cluster_cloud()
    return A, {k: S.sor_ref(A, k, 1.0) for k in (20, 100)}


# ---- the mean_k ladder: every register count of k_sor_knn and its boundaries -------------------
@pytest.mark.parametrize("mean_k", [1, 8, 50, 63, 64, 127, 128, 191, 192, 255])
def test_mean_k_ladder(gpu_ctx, shadow, mean_k):
    r, ref = check_equal(gpu_ctx, shadow, mean_k, 1.0)
    want = {8: 148, 50: 133, 150: 122, 255: 116}.get(mean_k)
    if want is not None:
        assert r["n_removed"] == want


def test_fixture_figures_and_python_mirror(gpu_ctx, shadow):
    r, ref = check_equal(gpu_ctx, shadow, 63, 0.5)
    assert r["n_removed"] == 190
    r, ref = check_equal(gpu_ctx, shadow, 50, 1.0)
    assert r["stats"].threshold == 0.021751963317590422
    kept, rem, dist, st = D.statistical_outlier_removal(shadow, 50, 1.0, ctx=gpu_ctx,
                                                        return_stats=True)
    assert np.array_equal(kept, ref["kept"]) and np.array_equal(rem, ref["removed"])
    assert np.array_equal(bits(dist), bits(ref["distances"]))
    assert st["threshold"] == ref["threshold"] and st["n_valid"] == 991
    idx = np.arange(990, -1, -3)
    k2, r2, d2 = D.statistical_outlier_removal(shadow, 8, 1.0, indices=idx, negative=True,
                                               ctx=gpu_ctx)
    ref2 = S.sor_ref(shadow, 8, 1.0, idx=idx, negative=True)
    assert np.array_equal(k2, ref2["kept"]) and np.array_equal(r2, ref2["removed"])
    assert np.array_equal(bits(d2), bits(ref2["distances"]))


# ---- the literal and the certified paths ---------------------------------------------------------
@pytest.mark.parametrize("mean_k", [20, 100])
def test_literal_paths_give_identical_bits(gpu_ctx, cluster, mean_k):
    """DLG_OPT_SOR_LITERAL 0..3: every query's sum and the statistics by the literal loops or by
    the certified reductions -- the same bits.  mean_k 20: both statistics certificates fail on
    their own; mean_k 100: the per-query certificate fails for 36 queries"""
    A, refs = cluster
    ref = refs[mean_k]
    assert len(ref["removed"]) == {20: 864, 100: 730}[mean_k]
    assert gpu_ctx.get_option(D.DLG_OPT_SOR_LITERAL) == 0
    try:
        for opt in (0, 1, 2, 3):
            gpu_ctx.set_option(D.DLG_OPT_SOR_LITERAL, opt)
            r = raw_call(gpu_ctx, A, mean_k, 1.0)
            assert_equal(r, ref)
            st = r["stats"]
            if opt & 1:
                assert st.literal_queries == st.n_valid == 4096
            else:
                assert st.literal_queries == {20: 0, 100: 36}[mean_k]
            if opt & 2:
                assert st.exact_sums == 0
            else:
                assert st.exact_sums == {20: 0, 100: 1}[mean_k]
    finally:
        gpu_ctx.set_option(D.DLG_OPT_SOR_LITERAL, 0)
    with pytest.raises(D.DialogError):
        gpu_ctx.set_option(D.DLG_OPT_SOR_LITERAL, 4)


# ---- deferral up the hierarchy -------------------------------------------------------------------
def test_sparse_outliers_defer_up_the_hierarchy(gpu_ctx):
    """a thin slab with 64 points scattered 20 times wider: their neighbours lie far outside the
    cells of the fine levels"""
    A = S.deferral_cloud()
    r, ref = check_equal(gpu_ctx, A, 50, 1.0)
    assert r["n_removed"] == 63 and (r["removed"][:63] >= 8192 - 64).all()


# ---- small clouds ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mean_k", [(2, 1), (9, 8), (65, 64), (129, 128), (256, 255),
                                      (257, 64), (300, 10)])
def test_small_clouds(gpu_ctx, shadow, n, mean_k):
    """n = mean_k + 1: every query's neighbours are the whole cloud; 65 and 257 points at
    mean_k 64; 300 identical points"""
    if n == 300:
        p = np.full((300, 3), 1.25, f32)
        r, ref = check_equal(gpu_ctx, p, mean_k, 1.0)
        assert r["stats"].threshold == 0.0 and r["n_removed"] == 0
    else:
        check_equal(gpu_ctx, shadow[:n], mean_k, 1.0)


def test_certificate_refuses_a_term_whose_units_need_more_than_64_bits(gpu_ctx):
    """neighbours at 2^-12 and at 4097 * 2^40: in units of 2^-12 the far term is 4097 * 2^52,
    which a 64-bit shift would wrap to 2^52 and so pass below 2^53.  The two queries that see both
    terms must take the literal loop; the third sees the far term twice and certifies."""
    p = np.array([[0, 0, 0], [2.0**-12, 0, 0], [4097 * 2.0**40, 0, 0]], f32)
    r, ref = check_equal(gpu_ctx, p, 2, 1.0)
    terms = np.sqrt(ref["d2"]).astype(f32)
    assert [S.certificate(t)[0] for t in terms] == [False, False, True]
    assert r["stats"].literal_queries == 2


# ---- argument forms --------------------------------------------------------------------------------
def test_nonfinite_points(gpu_ctx, shadow):
    p = shadow.copy()
    p[::37, 0] = np.nan
    p[5::111, 1] = np.inf
    p[9::185, 2] = -np.inf
    r, ref = check_equal(gpu_ctx, p, 8, 1.0)
    bad = ~np.isfinite(p).all(1)
    assert (r["distances"][bad] == 0).all() and r["stats"].n_valid == 991 - bad.sum()
    assert np.isin(np.flatnonzero(bad), r["kept"][:r["n_kept"]]).all()
    r, ref = check_equal(gpu_ctx, p, 8, -100.0)  # (a negative threshold removes them)
    assert np.isin(np.flatnonzero(bad), r["removed"][:r["n_removed"]]).all()
    check_equal(gpu_ctx, p, 70, 0.25, negative=1)


def test_index_lists(gpu_ctx, shadow):
    rng = np.random.default_rng(3)
    p = shadow.copy()
    p[::53, 2] = np.nan
    check_equal(gpu_ctx, p, 8, 1.0, idx=np.arange(0, 991, 3))              # subset
    check_equal(gpu_ctx, p, 8, 1.0, idx=rng.permutation(991))              # permuted
    check_equal(gpu_ctx, p, 66, 1.0, idx=rng.integers(0, 991, 1500))       # duplicated
    check_equal(gpu_ctx, p, 8, 1.0, idx=rng.integers(0, 991, 700), negative=1)
    r, ref = check_equal(gpu_ctx, p, 8, 1.0, idx=[17])                     # one entry
    assert not np.isfinite(r["stats"].threshold) and r["n_kept"] == 1 and r["n_removed"] == 0
    r, ref = check_equal(gpu_ctx, p, 8, 1.0, idx=[53])                     # one entry, not finite
    assert r["stats"].n_valid == 0 and r["n_kept"] + r["n_removed"] == 1


def test_strides_and_null_outputs(gpu_ctx, shadow):
    ref = S.sor_ref(shadow, 8, 1.0)
    wide = np.full((991, 4), 1.0, f32)
    wide[:, :3] = shadow
    assert_equal(raw_call(gpu_ctx, wide, 8, 1.0), ref)
    wider = np.full((991, 8), np.nan, f32)  # (the padding is never read as a coordinate)
    wider[:, :3] = shadow
    assert_equal(raw_call(gpu_ctx, wider, 8, 1.0), ref)
    r = raw_call(gpu_ctx, shadow, 8, 1.0, want_removed=False, want_dist=False, want_stats=False)
    assert r["status"] == 0 and r["n_kept"] == len(ref["kept"])
    assert np.array_equal(r["kept"][:r["n_kept"]], ref["kept"])
    assert (r["removed"] == -7).all() and (r["distances"] == -7).all() and r["n_removed"] == -1


# ---- status codes ---------------------------------------------------------------------------------
def test_status_codes(gpu_ctx, shadow):
    L = _lib.load()
    ref = S.sor_ref(shadow, 8, 1.0)
    nk, nr = len(ref["kept"]), len(ref["removed"])
    # cap one short: the sizes are reported, nothing is written; then success with those sizes
    r = raw_call(gpu_ctx, shadow, 8, 1.0, cap=nk - 1)
    assert r["status"] == _lib.DLG_ERR_CAPACITY and r["n_kept"] == nk and r["n_removed"] == nr
    assert (r["kept"] == -7).all() and (r["removed"] == -7).all()
    r = raw_call(gpu_ctx, shadow, 8, 1.0, cap_removed=nr - 1)
    assert r["status"] == _lib.DLG_ERR_CAPACITY and r["n_kept"] == nk and r["n_removed"] == nr
    assert (r["kept"] == -7).all() and (r["removed"] == -7).all()
    assert_equal(raw_call(gpu_ctx, shadow, 8, 1.0, cap=nk, cap_removed=nr), ref)
    # fewer than mean_k + 1 finite points
    p = shadow[:20].copy()
    p[3, 0] = np.nan
    r = raw_call(gpu_ctx, p, 19, 1.0)
    assert r["status"] == _lib.DLG_ERR_INVALID
    assert b"fewer than mean_k + 1 finite points" in L.dlg_last_error(gpu_ctx.h)
    with pytest.raises(S.TooFewPoints):
        S.sor_ref(p, 19, 1.0)
    assert raw_call(gpu_ctx, p, 18, 1.0)["status"] == 0
    for mean_k in (0, 256, -1):
        assert raw_call(gpu_ctx, shadow, mean_k, 1.0)["status"] == _lib.DLG_ERR_INVALID
    for mul in (np.nan, np.inf, -np.inf):
        assert raw_call(gpu_ctx, shadow, 8, mul)["status"] == _lib.DLG_ERR_INVALID
    for bad in ([0, 991], [-1, 5]):
        assert raw_call(gpu_ctx, shadow, 8, 1.0, idx=bad)["status"] == _lib.DLG_ERR_INVALID
    # an empty list: nothing kept or removed, but too few finite points is still an error, as is
    # an empty cloud
    empty = np.zeros(1, np.int32)[:0]
    r = raw_call(gpu_ctx, shadow, 8, 1.0, idx=empty)
    assert r["status"] == 0 and r["n_kept"] == 0 and r["n_removed"] == 0
    assert r["stats"].n_finite == 991 and (r["kept"] == -7).all()
    assert raw_call(gpu_ctx, p, 19, 1.0, idx=empty)["status"] == _lib.DLG_ERR_INVALID
    assert raw_call(gpu_ctx, shadow[:0], 8, 1.0)["status"] == _lib.DLG_ERR_INVALID
    assert b"fewer than mean_k + 1 finite points" in L.dlg_last_error(gpu_ctx.h)


def test_several_ranks_are_refused(shadow):
    """a context of a 2-rank communicator holds a shard: DLG_ERR_INVALID, and no collective runs
    (the other rank never calls)"""
    ctxs = D.Context.loopback_group(2, 0)
    try:
        r = raw_call(ctxs[0], shadow, 8, 1.0)
        assert r["status"] == _lib.DLG_ERR_INVALID
        assert b"world > 1" in _lib.load().dlg_last_error(ctxs[0].h)
        with pytest.raises(D.DialogError):
            D.statistical_outlier_removal_cloud(shadow, 8, 1.0, ctx=ctxs[1])
    finally:
        for c in ctxs:
            c.close()


# ---- the shim ---------------------------------------------------------------------------------------
def test_cpp_sor_shim_runs_on_gpu(tmp_path, shadow):
    """tests/cpp/shim_sor.cpp: dialog::StatisticalOutlierRemoval on double_shadow at mean_k 50"""
    exe = tmp_path / "shim_sor"
    lib = os.path.dirname(D.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_sor.cpp"), "-o", str(exe), "-L", lib,
                    "-ldialog_amd", f"-Wl,-rpath,{lib}"], check=True)
    raw = tmp_path / "shadow.f32"
    shadow.tofile(str(raw))
    out = subprocess.run([str(exe), str(raw), "50", "1.0"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.strip().splitlines()}
    ref = S.sor_ref(shadow, 50, 1.0)

    def lsum(v):
        return sum((i + 1) * int(x) for i, x in enumerate(v))

    assert lines["lists"] == ["991", "858", "133", str(lsum(ref["kept"])), str(lsum(ref["removed"]))]
    assert float.fromhex(lines["threshold"][0]) == 0.021751963317590422 == ref["threshold"]
    assert lines["cloud"] == ["858", "1"]
    neg = S.sor_ref(shadow[ref["kept"]], 50, 1.0, negative=True)
    assert lines["negative"] == [str(len(neg["kept"])), str(len(neg["removed"]))]
    assert lines["empty"] == ["0"]


# ---- the device-resident result -------------------------------------------------------------------
@pytest.fixture(scope="module")
def sor_clouds(gpu_ctx):
    """about 20,000 points of three planes with 5 % outliers, filtered both ways: to the host and
    re-uploaded, and left on the device"""
    p, _, _ = plane_cloud(20000, 3, outlier_frac=0.05, seed=77)
    kept, rem, dist = D.statistical_outlier_removal(p, 20, 1.0, ctx=gpu_ctx)
    up = D.Cloud(gpu_ctx, p[kept], id_base=1000)
    dev, kept_d, st = D.statistical_outlier_removal_cloud(p, 20, 1.0, id_base=1000, ctx=gpu_ctx,
                                                          return_stats=True)
    yield p, kept, rem, up, dev, kept_d, st
    up.close()
    dev.close()


def test_sor_cloud_equals_upload_of_the_host_result(sor_clouds):
    p, kept, rem, up, dev, kept_d, st = sor_clouds
    assert 0 < len(rem) < len(p) // 4 and len(kept) + len(rem) == len(p)
    assert np.array_equal(kept, kept_d) and st["n_valid"] == len(p)
    assert dev.n == up.n == len(kept) and dev.n_active == up.n_active
    assert dev.signature() == up.signature()
    # (the host result itself, on a prefix the numpy search finishes quickly)
    ref = S.sor_ref(p[:4000], 20, 1.0)
    k2, r2, d2 = D.statistical_outlier_removal(p[:4000], 20, 1.0, ctx=up.ctx)
    assert np.array_equal(k2, ref["kept"]) and np.array_equal(bits(d2), bits(ref["distances"]))


def test_sor_cloud_planes_equal(sor_clouds):
    p, kept, rem, up, dev, _, _ = sor_clouds
    prm = D.make_params(0.02, max_iterations=200, probability=0.99)
    ra = D.extract_planes(up, prm, max_planes=3)
    rb = D.extract_planes(dev, prm, max_planes=3)
    assert ra["n_planes"] == rb["n_planes"] == 3
    assert np.array_equal(bits(ra["coeffs"]), bits(rb["coeffs"]))
    assert np.array_equal(ra["offsets"], rb["offsets"])
    assert np.array_equal(ra["inliers"], rb["inliers"])
