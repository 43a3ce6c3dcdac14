"""GPU: dlg_sac_ia_align, dlg_sac_ia_score and dlg_fpfh_knn against the numpy restatement
(tests/sac_ia_ref.py) -- every case of tests/golden/sac_ia_small.npz bit-equal, the descriptor
search and the scorer against brute force at the sizes where their kernels change path (wave,
slab and batch boundaries, the block-stride loop, the coarser levels, an error beyond 64 bits), the
refusals, the Python mirror, the C++ shim and one production launch shape.

Nothing has a tolerance: integers are equal, floats are bit-equal.
"""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import dialog_amd as D
import icp_ref as R
import sac_ia_ref as S
from dialog_amd import _lib
from dialog_amd.sac import _f32p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SLAB = 8192  # sacia.hpp kSaciaSlab
HYP_KEYS = ("sample", "match", "rank", "valid", "relaxations", "draws", "n_far", "n_used",
            "err_hi", "err_lo")
SCALARS = ("converged", "best_iteration", "n_valid", "n_invalid", "draws", "relaxations",
           "n_queries")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def dbits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_floats(a, b):
    """bit-equal where finite, non-finite in the same places (a NaN's payload is not pinned)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    fin = np.isfinite(a)
    return a.shape == b.shape and np.array_equal(fin, np.isfinite(b)) and \
        np.array_equal(bits(a)[fin], bits(b)[fin]) and np.array_equal(np.isnan(a), np.isnan(b))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "sac_ia_small.npz"))
    return z, json.loads(str(z["meta"]))


def load_case(golden, name):
    z, meta = golden
    m = meta[name]
    case = {k: z[key] for k, key in m["inputs"].items()}
    if "guess" in case:
        case["guess"] = case["guess"].reshape(4, 4)
    case.update(m["args"])
    return case


def run(ctx, case, **kw):
    args = {k: case[k] for k in S.ALIGN_KEYS if k in case}
    args.update(kw)
    return D.sac_ia_align(case["src"], case["fs"], case["tgt"], case["ft"], guess=case.get("guess"),
                          fitness_max_range=R.DBL_MAX, ctx=ctx, return_hypotheses=True,
                          return_stats=True, **args)


def assert_equals_golden(golden, name, res):
    z, meta = golden
    final, aligned, hyp, st = res
    m = meta[name]
    assert same_floats(final, z[name + "/final"])
    assert same_floats(aligned, z[name + "/aligned"])
    assert len(hyp) == len(z[name + "/valid"]) == st["iterations"]
    for k in HYP_KEYS:
        got = np.array([h[k] for h in hyp])
        assert np.array_equal(got.astype(z[f"{name}/{k}"].dtype), z[f"{name}/{k}"]), (name, k)
    assert same_floats(np.array([h["T"].reshape(16) for h in hyp], f32).reshape(-1, 16),
                       z[name + "/T"])
    for k in SCALARS:
        assert st[k] == m[k], (name, k)
    assert dbits(st["error"])[0] == dbits(m["error"])[0]
    assert dbits(st["fitness"])[0] == dbits(m["fitness"])[0]
    assert 1 <= st["host_syncs"] <= 2 + st["batches"]


# ---- the golden cases ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_bit_equal_with_the_golden(gpu_ctx, golden, name):
    assert_equals_golden(golden, name, run(gpu_ctx, load_case(golden, name)))


@pytest.mark.parametrize("name", ["finite_threshold", "non_finite", "guess_wins"])
def test_same_bits_twice_and_under_other_launch_shapes(gpu_ctx, golden, name):
    """E is an exact integer: neither a second run, the batch size nor the grid shows in any bit"""
    case = load_case(golden, name)
    for kw in (dict(), dict(max_blocks=1), dict(batch=7), dict(batch=1, max_blocks=2)):
        res = run(gpu_ctx, case, **kw)
        assert_equals_golden(golden, name, res)
        if "batch" in kw:
            scored = res[3]["n_valid"] + int("guess" in case)
            assert res[3]["batches"] == -(-scored // kw["batch"])


# ---- the descriptor search ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables():
    """rows of small integers (many exact ties: the index order shows) and 130 queries, with the
    (d, index) order of every query over the first n rows, n the sizes the tests use"""
    rng = np.random.default_rng(1234)
    rows = rng.integers(0, 3, size=(SLAB + 1, 33)).astype(f32)
    q = rng.integers(0, 3, size=(130, 33)).astype(f32)
    real_rows = (rng.random((257, 33)) * 100).astype(f32)
    real_q = (rng.random((130, 33)) * 100).astype(f32)
    return rows, q, real_rows, real_q


N_ROWS = (63, 64, 65, 257, SLAB - 1, SLAB, SLAB + 1)
N_QUERIES = (1, 63, 64, 65, 130)


@pytest.mark.parametrize("k", [1, 2, 10, 32])
def test_fpfh_knn_against_brute_force(gpu_ctx, tables, k):
    rows, q, real_rows, real_q = tables
    for n in sorted(set((k, k + 1) + N_ROWS)):
        if n < k:
            continue
        want_i, want_d = S.knn(q, rows[:n], k)
        for nq in N_QUERIES:
            idx, d = D.fpfh_knn(q[:nq], rows[:n], k, ctx=gpu_ctx)
            assert np.array_equal(idx, want_i[:nq]), (n, nq)
            assert np.array_equal(bits(d), bits(want_d[:nq])), (n, nq)
    want_i, want_d = S.knn(real_q, real_rows, k)
    idx, d = D.fpfh_knn(real_q, real_rows, k, ctx=gpu_ctx)
    assert np.array_equal(idx, want_i) and np.array_equal(bits(d), bits(want_d))


def test_fpfh_knn_duplicates_nan_rows_and_nan_queries(gpu_ctx, tables):
    _, _, rows, q = tables
    rows, q = rows.copy(), q[:70].copy()
    rows[100:140] = rows[:40]          # duplicated rows: equal distances, the lower index first
    rows[[3, 64, 200]] = np.nan        # skipped
    rows[7, 32] = np.inf
    q[5, 0] = np.nan
    q[69, 32] = -np.inf
    want_i, want_d = S.knn(q, rows, 10)
    assert (want_i[[5, 69]] == -1).all() and not np.isin(want_i, [3, 7, 64, 200]).any()
    idx, d = D.fpfh_knn(q, rows, 10, ctx=gpu_ctx)
    assert np.array_equal(idx, want_i) and np.array_equal(bits(d), bits(want_d))
    # a query equal to a duplicated row finds both copies first, in index order
    idx, d = D.fpfh_knn(rows[10:11], rows, 2, ctx=gpu_ctx)
    assert idx.tolist() == [[10, 110]] and d.tolist() == [[0.0, 0.0]]
    # strided records
    wide = np.full((len(rows), 40), 7.5, f32)
    wide[:, :33] = rows
    idx2, _ = D.fpfh_knn(q, wide, 10, ctx=gpu_ctx)
    assert np.array_equal(idx2, want_i)


def test_fpfh_knn_refusals(gpu_ctx, tables):
    rows = tables[2][:10].copy()
    q = tables[3][:4]
    with pytest.raises(D.DialogError):
        D.fpfh_knn(q, rows, 11, ctx=gpu_ctx)       # fewer rows than k
    rows[[1, 4, 8]] = np.nan
    with pytest.raises(D.DialogError):
        D.fpfh_knn(q, rows, 8, ctx=gpu_ctx)        # 7 valid rows
    assert D.fpfh_knn(q, rows, 7, ctx=gpu_ctx)[0].min() >= 0
    for bad in (0, 33):
        with pytest.raises(D.DialogError):
            D.fpfh_knn(q, rows, bad, ctx=gpu_ctx)
    L = _lib.load()
    out_i, out_d = np.zeros((4, 2), np.int32), np.zeros((4, 2), f32)
    from dialog_amd.sac import _i32p
    for qs, rs in ((128, 132), (132, 134), (132, 64)):
        assert L.dlg_fpfh_knn(gpu_ctx.h, _f32p(q), qs, 4, _f32p(rows), rs, 10, 2, _i32p(out_i),
                              _f32p(out_d)) == _lib.DLG_ERR_INVALID


# ---- the scorer ---------------------------------------------------------------------------------
def motions(n, seed=5, scale=1.0, shift=0.01):
    """n rigid motions: a few degrees about a random axis and a shift of about scale * shift"""
    rng = np.random.default_rng(seed)
    return np.array([R.rigid(rng.normal(size=3), scale * 4.0 * rng.normal(),
                             scale * shift * rng.normal(size=3)) for _ in range(n)], f32)


def assert_scores(hyp, src, tgt, T, thr):
    tv = tgt[np.isfinite(tgt).all(1)]
    for h, t in zip(hyp, T):
        E, far, used = S.error_metric(t, src, tv, S.threshold(thr))
        assert (h["E"], h["n_far"], h["n_used"]) == (E, far, used)
        assert h["err_lo"] < 1 << 24 and np.array_equal(bits(h["T"]), bits(t.reshape(4, 4)))


@pytest.mark.parametrize("thr", [math.sqrt(R.DBL_MAX), 1e-12, None])
def test_score_against_brute_force(gpu_ctx, golden, thr):
    """thr: +inf (no search: every term 0), tiny (every term 1.0), three point spacings squared"""
    case = load_case(golden, "finite_threshold")
    src, tgt = case["src"].copy(), case["tgt"].copy()
    src[7] = np.nan
    tgt[3, 2] = np.inf
    thr = case["max_correspondence_distance"] if thr is None else thr
    T = motions(9, shift=0.03)  # (the threshold's root is 0.024: some points land beyond it)
    for n in (1, 63, 64, 65, 257):
        for nt in (1, 3, 4, 5, 9):
            for mb in (0, 1, 2):
                hyp = D.sac_ia_score(src[:n], tgt, T[:nt], thr, batch=4, max_blocks=mb, ctx=gpu_ctx)
                assert len(hyp) == nt
                assert_scores(hyp, src[:n], tgt, T[:nt], thr)
    full = D.sac_ia_score(src, tgt, T, thr, ctx=gpu_ctx)
    assert_scores(full, src, tgt, T, thr)
    if thr == case["max_correspondence_distance"]:
        assert any(0 < h["n_far"] < h["n_used"] for h in full)
    elif thr < 1:
        assert all(h["n_far"] == h["n_used"] == 445 and h["E"] == 445 << 48 for h in full)
    else:
        assert all(h["n_far"] == 0 and h["E"] == 0 and h["n_used"] == 445 for h in full)


def test_score_a_pair_exactly_at_the_threshold(gpu_ctx):
    """d2 == thr: e <= thr holds and e / thr is 1.0 by division"""
    tgt = np.zeros((1, 3), f32)
    src = np.array([[0.5, 0, 0], [0.25, 0, 0], [1.0, 0, 0]], f32)
    h = D.sac_ia_score(src, tgt, np.eye(4, dtype=f32), 0.25, ctx=gpu_ctx)[0]
    assert (h["n_far"], h["n_used"]) == (2, 3)
    assert h["E"] == (2 << 48) + (1 << 46)


def test_score_an_error_beyond_64_bits(gpu_ctx, golden):
    """65,537 points, every term 1.0: E = 65,537 x 2^48 needs both words"""
    tgt = load_case(golden, "default")["tgt"]
    rng = np.random.default_rng(9)
    src = (rng.random((65537, 3)) + 100.0).astype(f32)
    T = np.array([np.eye(4), R.rigid((0, 0, 1), 3.0, (0.5, 0, 0))], f32)
    for mb in (0, 1):
        for h in D.sac_ia_score(src, tgt, T, 1e-6, max_blocks=mb, ctx=gpu_ctx):
            assert h["E"] == 65537 << 48 > 1 << 64
            assert (h["err_hi"], h["err_lo"]) == (65537 << 24, 0)
            assert h["n_far"] == h["n_used"] == 65537


@pytest.fixture(scope="module")
def thrown():
    """3,000 source points well outside the target's box, a threshold no level's radius exceeds"""
    rng = np.random.default_rng(21)
    tgt = rng.random((4000, 3)).astype(f32)
    src = (rng.random((3000, 3)) * 0.5 + [6.0, -4.0, 9.0]).astype(f32)
    return src, tgt, motions(5, seed=8, scale=0.3), 1e6


def test_score_deferred_pairs_settle_at_the_coarser_levels(gpu_ctx, thrown):
    src, tgt, T, thr = thrown
    for kw in (dict(), dict(batch=2), dict(max_blocks=1), dict(batch=3, max_blocks=2)):
        hyp = D.sac_ia_score(src, tgt, T, thr, ctx=gpu_ctx, **kw)
        assert_scores(hyp, src, tgt, T, thr)
        assert all(h["n_far"] == 0 and h["n_used"] == 3000 and h["E"] > 0 for h in hyp)


def test_a_far_guess_reaches_the_coarser_levels(gpu_ctx, thrown):
    """only the guess is scored (no iteration is drawn): a small shift settles near level 0, a
    shift far outside the target's box goes up the hierarchy"""
    src, tgt, _, thr = thrown
    rng = np.random.default_rng(3)
    fs, ft = rng.random((3000, 33)).astype(f32), rng.random((4000, 33)).astype(f32)

    def guess_only(shift):
        g = R.rigid((0, 0, 1), 0.0, shift)
        assert not S.guess_is_identity(g)
        res = D.sac_ia_align(tgt[:3000], fs, tgt, ft, guess=g, max_iterations=0, ctx=gpu_ctx,
                             max_correspondence_distance=thr, return_hypotheses=True,
                             return_stats=True)
        assert np.array_equal(res[0], g) and res[3]["converged"] == 0 and len(res[2]) == 1
        h = res[2][0]
        assert h["draws"] == 0 and (h["sample"] == -1).all()
        E, nfar, used = S.error_metric(g, tgt[:3000], tgt, S.threshold(thr))
        assert (h["E"], h["n_far"], h["n_used"]) == (E, nfar, used) and E > 0
        assert res[3]["error"] == float(E) * 2.0 ** -48
        return res[3]["levels"]

    near, far = guess_only((0.021, 0.0, 0.0)), guess_only((6.0, -4.0, 9.0))
    assert 1 <= near < far and far >= 3


# ---- refusals, the mirror, the shim -------------------------------------------------------------
def test_status_codes(gpu_ctx, golden):
    case = load_case(golden, "finite_threshold")
    ok = dict(max_iterations=3)

    def refused(msg=None, **kw):
        c = dict(case)
        for k in ("src", "fs", "tgt", "ft", "guess"):
            if k in kw:
                c[k] = kw.pop(k)
        with pytest.raises(D.DialogError) as e:
            run(gpu_ctx, c, **dict(ok, **kw))
        assert e.value.status == _lib.DLG_ERR_INVALID
        if msg:
            assert msg in str(e.value)

    refused("nr_samples", src=case["src"][:2], fs=case["fs"][:2])
    for bad in (dict(nr_samples=2), dict(nr_samples=9), dict(k_correspondences=0),
                dict(k_correspondences=33), dict(max_iterations=-1), dict(rng=2),
                dict(batch=-1), dict(max_blocks=-1)):
        refused(**bad)
    for md in (0.0, -1.0, math.nan):
        refused("max_correspondence_distance", max_correspondence_distance=md)
    g = np.eye(4, dtype=f32)
    g[1, 3] = np.inf
    refused("guess", guess=g)
    ft = case["ft"].copy()
    ft[9:] = np.nan
    refused("fewer valid rows", ft=ft)                  # 9 valid rows, k = 10
    refused("fewer valid rows", tgt=case["tgt"][:4], ft=case["ft"][:4])
    L = _lib.load()
    prm = _lib.SacIaParams()
    L.dlg_sac_ia_params_default(C.byref(prm))
    a, b = np.ascontiguousarray(case["src"]), np.ascontiguousarray(case["tgt"])
    fa, fb = np.ascontiguousarray(case["fs"]), np.ascontiguousarray(case["ft"])
    ps, pt = _lib.Points(_f32p(a), len(a), 12), _lib.Points(_f32p(b), len(b), 12)
    fin = np.zeros(16, f32)

    def raw(fs=_f32p(fa), ft_=_f32p(fb), s1=132, s2=132, out=None, ostride=12):
        return L.dlg_sac_ia_align(gpu_ctx.h, C.byref(ps), fs, s1, C.byref(pt), ft_, s2, C.byref(prm),
                                  None, _f32p(fin), out, ostride, None, 0, None)
    prm.max_iterations = 2
    assert raw() == 0
    assert raw(fs=None) == _lib.DLG_ERR_INVALID and raw(ft_=None) == _lib.DLG_ERR_INVALID
    assert raw(s1=128) == _lib.DLG_ERR_INVALID and raw(s2=134) == _lib.DLG_ERR_INVALID
    out = np.zeros((len(a), 4), f32)
    assert raw(out=_f32p(out), ostride=20) == _lib.DLG_ERR_INVALID
    assert raw(out=_f32p(out), ostride=16) == 0 and (out[:, 3] == 1.0).all()
    with pytest.raises(D.DialogError):
        D.sac_ia_score(case["src"], case["tgt"], np.eye(4), -1.0, ctx=gpu_ctx)
    with pytest.raises(D.DialogError):
        D.sac_ia_score(case["src"], np.full((3, 3), np.nan, f32), np.eye(4), 1.0, ctx=gpu_ctx)
    # nothing to draw: the result is the guess, nothing converged
    final, _, hyp, st = run(gpu_ctx, case, max_iterations=0)
    assert np.array_equal(final, np.eye(4)) and hyp == [] and st["converged"] == 0
    assert (st["best_iteration"], st["iterations"], st["error"]) == (-1, 0, 0.0)


def test_several_ranks_are_refused(golden):
    """a context of a 2-rank communicator holds a shard: DLG_ERR_INVALID, and no collective runs"""
    case = load_case(golden, "default")
    ctxs = D.Context.loopback_group(2, 0)
    try:
        with pytest.raises(D.DialogError) as e:
            run(ctxs[0], case, max_iterations=2)
        assert e.value.status == _lib.DLG_ERR_INVALID and "world > 1" in str(e.value)
        with pytest.raises(D.DialogError):
            D.sac_ia_score(case["src"], case["tgt"], np.eye(4), 1.0, ctx=ctxs[1])
    finally:
        for c in ctxs:
            c.close()


def test_python_mirror_and_stats(gpu_ctx, golden):
    z, meta = golden
    case = load_case(golden, "default")
    plain = D.sac_ia_align(case["src"], case["fs"], case["tgt"], case["ft"], max_iterations=60,
                           ctx=gpu_ctx)
    assert len(plain) == 2 and same_floats(plain[0], z["default/final"])
    assert same_floats(plain[1], z["default/aligned"])
    final, aligned, st = D.sac_ia_align(case["src"], case["fs"], case["tgt"], case["ft"],
                                        max_iterations=60, ctx=gpu_ctx, return_stats=True)
    # PCL's default distance: thr = +inf, every error 0, the first hypothesis wins
    assert (st["best_iteration"], st["converged"], st["error"], st["fitness"]) == (0, 1, 0.0, 0.0)
    assert st["iterations"] == 60 and st["n_valid"] == 60 and st["batches"] == 1
    assert st["levels"] >= 1 and st["device_ms"] >= 0 and "reserved" not in st
    msvc = load_case(golden, "msvc")
    res = D.sac_ia_align(msvc["src"], msvc["fs"], msvc["tgt"], msvc["ft"], max_iterations=60,
                         max_correspondence_distance=msvc["max_correspondence_distance"],
                         rng=D.registration.RNG_MSVC, ctx=gpu_ctx)
    assert same_floats(res[0], z["msvc/final"])


def test_cpp_sac_ia_shim_runs_on_gpu(tmp_path, gpu_ctx, golden):
    """tests/cpp/shim_sac_ia.cpp: PCLViewer.cpp:546-558's calls, aligning into the source cloud"""
    z, meta = golden
    exe = tmp_path / "shim_sac_ia"
    lib = os.path.dirname(D.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_sac_ia.cpp"), "-o", str(exe), "-L", lib,
                    "-ldialog_amd", f"-Wl,-rpath,{lib}"], check=True)
    for name, dist in (("default", 0.0), ("finite_threshold", None)):
        case = load_case(golden, name)
        files = []
        for k in ("src", "fs", "tgt", "ft"):
            files.append(str(tmp_path / f"{name}_{k}.f32"))
            np.ascontiguousarray(case[k], f32).tofile(files[-1])
        dist = case["max_correspondence_distance"] if dist is None else dist
        out = subprocess.run([str(exe), *files, str(case["max_iterations"]), repr(float(dist))],
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.strip().splitlines()}
        m = meta[name]
        assert lines["converged"] == [str(m["converged"])]
        assert lines["final"] == [str(int(b)) for b in bits(z[name + "/final"]).reshape(16)]
        assert lines["fitness"] == [str(int(dbits(m["fitness"])[0]))]
        u = bits(z[name + "/aligned"])
        chk = sum((i * 3 + j + 1) * int(u[i, j]) for i in range(len(u)) for j in range(3)) % 2**64
        assert lines["aligned"] == [str(len(u)), str(chk)]
        assert lines["stats"] == [str(len(z[name + "/valid"])), str(m["best_iteration"]),
                                  str(m["n_valid"])]


# ---- a production launch shape ------------------------------------------------------------------
def test_production_launch_shape(gpu_ctx):
    """200,000 source entries against 50,000 target points, 8 transformations, default options: the
    level-0 kernel's capped grid, a full batch, the coarser levels behind it.  The reference is
    icp_ref.correspondences_fast (k-d tree candidates re-evaluated in float32, every uncertified
    query answered by the brute force), its d2 through the restatement's terms."""
    c = R.large_case()
    src, tgt = c["src"][:200000], c["tgt"]
    assert len(src) == 200000 and len(tgt) == 50000
    T = motions(8, seed=77, scale=0.2)
    spacing = R.neighbour_spacing(tgt[:2000])
    thr = float(f32(spacing * spacing))
    hyp = D.sac_ia_score(src, tgt, T, thr, ctx=gpu_ctx)
    info = {}
    for h, t in zip(hyp, T):
        W = R.transform_points(t, src)
        nn, d2 = R.correspondences_fast(W, tgt, info=info)
        assert (nn >= 0).all()
        E, far = S.error_of_distances(d2, S.threshold(thr))
        assert (h["E"], h["n_far"], h["n_used"]) == (E, far, len(src))
        assert 0 < far < len(src)
    assert info["uncertified"] <= 0.01 * info["queries"]
