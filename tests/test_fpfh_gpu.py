"""GPU: dlg_fpfh_estimate / dlg_cloud_fpfh against tests/fpfh_ref.py (the numpy restatement of
pcl::FPFHEstimation) on the inputs of the fixture tests/golden/fpfh_small.npz.

The parity rule (tests/test_fpfh.py): neighbour counts, NaN rows, zero rows and the integer stats
equal the reference's; the SPFH counts equal it at its stable points; the descriptors are bit-equal
at its stable rows.  No ulp allowance: given equal counts everything after them is IEEE + * / in a
fixed order."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import dialog_amd as D
import fpfh_ref as F
from dialog_amd import _lib
from dialog_amd.sac import _f32p, _i32p

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CASES = ("shadow", "planes", "sphere", "dense", "near_dup", "dups_nan", "indices", "thin")
STAT_KEYS = ("n_finite", "n_nan_rows", "n_zero_rows", "max_neighbours", "n_lds_overflow", "n_pairs",
             "n_pairs_failed", "n_sum_literal")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fpfh_small.npz"))
    return z, json.loads(str(z["meta"]))


@pytest.fixture(scope="module")
def refs(golden):
    """the reference on the fixture's inputs, once per case"""
    z, meta = golden
    out = {}

    def get(name):
        if name not in out:
            idx = z[name + "/idx"] if name + "/idx" in z.files else None
            out[name] = F.fpfh_ref(z[name + "/points"], z[name + "/normals"], meta[name]["radius"],
                                   idx)
        return out[name]
    return get


def raw_call(ctx, pts, nrm, radius, idx=None, hist_stride=132, want_nb=True, want_counts=True,
             want_stats=True, null_normals=False, nrm_stride=None):
    """dlg_fpfh_estimate through ctypes"""
    L = _lib.load()
    a = np.ascontiguousarray(pts, f32)
    b = np.ascontiguousarray(nrm, f32)
    P = _lib.Points(_f32p(a), a.shape[0], 4 * a.shape[1])
    prm = _lib.FpfhParams(float(radius))
    ix = None if idx is None else np.ascontiguousarray(idx, np.int32)
    n = a.shape[0] if ix is None else ix.shape[0]
    hist = np.full((max(n, 1), max(hist_stride, 132) // 4), -7.0, f32)
    nb = np.full(max(n, 1), -7, np.int32)
    cnt = np.full((max(a.shape[0], 1), 33), -7, np.int32)
    st = _lib.FpfhStats()
    s = L.dlg_fpfh_estimate(
        ctx.h, C.byref(P), None if null_normals else _f32p(b),
        4 * b.shape[1] if nrm_stride is None else nrm_stride,
        None if ix is None else _i32p(ix), n if ix is not None else 0, C.byref(prm), _f32p(hist),
        hist_stride, _i32p(nb) if want_nb else None, _i32p(cnt) if want_counts else None,
        C.byref(st) if want_stats else None)
    return dict(status=s, hist=hist[:n], nb=nb[:n], counts=cnt[:a.shape[0]], stats=st)


def check(r, ref):
    """a call's result under the parity rule"""
    assert np.array_equal(r["nb"], ref["neighbours"])
    got = {k: getattr(r["stats"], k) for k in STAT_KEYS}
    assert got == ref["stats"]
    sp, st = ref["stable_spfh"], ref["stable"]
    assert np.array_equal(r["counts"][sp], ref["counts"][sp])
    assert np.array_equal(bits(r["hist"][:, :33][st]), bits(ref["hist"][st]))
    nan_rows = ref["neighbours"] < 0
    assert np.isnan(r["hist"][:, :33][nan_rows]).all()
    assert not np.isnan(r["hist"][:, :33][~nan_rows & st]).any()


@pytest.mark.parametrize("name", CASES)
def test_case_against_the_reference(gpu_ctx, golden, refs, name):
    z, meta = golden
    idx = z[name + "/idx"] if name + "/idx" in z.files else None
    r = raw_call(gpu_ctx, z[name + "/points"], z[name + "/normals"], meta[name]["radius"], idx=idx)
    assert r["status"] == 0, _lib.load().dlg_last_error(gpu_ctx.h)
    ref = refs(name)
    check(r, ref)
    if name == "dense":  # the windows of an entry with more neighbours than the on-chip buffer
        assert r["stats"].n_lds_overflow == ref["stats"]["n_lds_overflow"] > 100
    if name == "near_dup":  # the literal double sums
        assert r["stats"].n_sum_literal == ref["stats"]["n_sum_literal"] > 0
    if name == "planes":
        zero = ref["neighbours"] == 1
        assert zero.sum() == r["stats"].n_zero_rows > 0 and (bits(r["hist"][zero]) == 0).all()


def test_index_list_rows_are_the_full_run_s(gpu_ctx, golden):
    z, meta = golden
    pts, nrm, idx = z["shadow/points"], z["shadow/normals"], z["indices/idx"]
    full = raw_call(gpu_ctx, pts, nrm, meta["shadow"]["radius"])
    part = raw_call(gpu_ctx, pts, nrm, meta["shadow"]["radius"], idx=idx)
    assert full["status"] == 0 and part["status"] == 0
    assert np.array_equal(bits(part["hist"]), bits(full["hist"][idx]))
    assert np.array_equal(part["nb"], full["nb"][idx])
    assert np.array_equal(part["counts"], full["counts"])  # (by point either way)


def test_strides_and_optional_outputs(gpu_ctx, golden, refs):
    """pcl::PointXYZ, pcl::Normal and padded descriptor records; every optional output NULL"""
    z, meta = golden
    pts, nrm, radius = z["dups_nan/points"], z["dups_nan/normals"], meta["dups_nan"]["radius"]
    p4 = np.concatenate([pts, np.ones((len(pts), 1), f32)], 1)
    n8 = np.concatenate([nrm, np.full((len(pts), 5), 9.0, f32)], 1)
    r = raw_call(gpu_ctx, p4, n8, radius, hist_stride=160)
    assert r["status"] == 0
    check(r, refs("dups_nan"))
    assert (r["hist"][:, 33:] == -7.0).all()  # (the rest of a record is not written)
    q = raw_call(gpu_ctx, pts, nrm, radius, want_nb=False, want_counts=False, want_stats=False)
    assert q["status"] == 0 and np.array_equal(bits(q["hist"]), bits(r["hist"][:, :33]))
    assert (q["nb"] == -7).all() and (q["counts"] == -7).all()


def test_wrong_arguments_are_invalid(gpu_ctx, golden):
    z, _ = golden
    pts, nrm = z["dups_nan/points"], z["dups_nan/normals"]
    bad = _lib.DLG_ERR_INVALID
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        assert raw_call(gpu_ctx, pts, nrm, radius)["status"] == bad
    for idx in ([0, len(pts)], [-1]):
        assert raw_call(gpu_ctx, pts, nrm, 0.3, idx=idx)["status"] == bad
    assert raw_call(gpu_ctx, pts, nrm, 0.3, null_normals=True)["status"] == bad
    for hs in (128, 134, 0):
        assert raw_call(gpu_ctx, pts, nrm, 0.3, hist_stride=hs)["status"] == bad
    for ns in (8, 14):
        assert raw_call(gpu_ctx, pts, nrm, 0.3, nrm_stride=ns)["status"] == bad
    L = _lib.load()
    prm = _lib.FpfhParams(0.3)
    a = np.ascontiguousarray(pts, f32)
    hist = np.zeros((len(a), 33), f32)
    for n, n_idx in ((2**31, 0), (len(a), 2**31)):
        P = _lib.Points(_f32p(a), n, 12)
        one = np.zeros(1, np.int32)
        assert L.dlg_fpfh_estimate(gpu_ctx.h, C.byref(P), _f32p(nrm), 12,
                                   _i32p(one) if n_idx else None, n_idx, C.byref(prm), _f32p(hist),
                                   132, None, None, None) == bad
    # a cloud without normals
    cl = D.Cloud(gpu_ctx, pts)
    try:
        assert L.dlg_cloud_fpfh(gpu_ctx.h, cl.h, C.byref(prm), _f32p(hist), 132, None, None) == bad
        with pytest.raises(D.DialogError):
            D.cloud_fpfh(cl, 0.3)
    finally:
        cl.close()
    assert raw_call(gpu_ctx, pts, nrm, 0.3)["status"] == 0  # (the context is still good)


def test_several_ranks_are_refused(golden):
    """a context of a 2-rank communicator holds a shard: DLG_ERR_INVALID, and no collective runs"""
    z, _ = golden
    pts, nrm = z["dups_nan/points"], z["dups_nan/normals"]
    ctxs = D.Context.loopback_group(2, 0)
    try:
        assert raw_call(ctxs[0], pts, nrm, 0.3)["status"] == _lib.DLG_ERR_INVALID
        assert b"world > 1" in _lib.load().dlg_last_error(ctxs[0].h)
        with pytest.raises(D.DialogError):
            D.fpfh_estimation(pts, nrm, 0.3, ctx=ctxs[1])
    finally:
        for c in ctxs:
            c.close()


def test_python_mirror_equals_the_raw_call(gpu_ctx, golden, refs):
    z, meta = golden
    pts, nrm, radius = z["planes/points"], z["planes/normals"], meta["planes"]["radius"]
    r = raw_call(gpu_ctx, pts, nrm, radius)
    hist, nb, counts, st = D.fpfh_estimation(pts, nrm, radius, ctx=gpu_ctx, return_counts=True,
                                             return_stats=True)
    assert hist.shape == (len(pts), 33) and hist.dtype == f32 and nb.dtype == np.int32
    assert np.array_equal(bits(hist), bits(r["hist"])) and np.array_equal(nb, r["nb"])
    assert np.array_equal(counts, r["counts"])
    assert {k: st[k] for k in STAT_KEYS} == refs("planes")["stats"]
    idx = z["indices/idx"][:50] % len(pts)
    h2, nb2 = D.fpfh_estimation(pts, nrm, radius, indices=idx, ctx=gpu_ctx)
    assert np.array_equal(bits(h2), bits(hist[idx])) and np.array_equal(nb2, nb[idx])
    # an empty cloud and an empty list
    h0, nb0 = D.fpfh_estimation(np.zeros((0, 3), f32), np.zeros((0, 3), f32), radius, ctx=gpu_ctx)
    assert h0.shape == (0, 33) and nb0.shape == (0,)
    h0, nb0, st0 = D.fpfh_estimation(pts, nrm, radius, indices=np.zeros(0, np.int32), ctx=gpu_ctx,
                                     return_stats=True)
    assert h0.shape == (0, 33) and st0["n_finite"] == len(pts)


def test_cloud_chain_equals_the_host_call(gpu_ctx, golden):
    """upload -> dlg_cloud_estimate_normals -> dlg_cloud_fpfh against dlg_fpfh_estimate fed the
    same points and the normals that call returned"""
    z, meta = golden
    pts = z["shadow/points"]
    cl = D.Cloud(gpu_ctx, pts)
    try:
        nrm = cl.estimate_normals(radius=meta["shadow"]["r_normals"], copy_out=True)
        hist, nb, st = D.cloud_fpfh(cl, meta["shadow"]["radius"], return_stats=True)
        h2, nb2, st2 = D.fpfh_estimation(pts, nrm, meta["shadow"]["radius"], ctx=gpu_ctx,
                                         return_stats=True)
        assert np.array_equal(bits(hist), bits(h2)) and np.array_equal(nb, nb2)
        assert {k: st[k] for k in STAT_KEYS} == {k: st2[k] for k in STAT_KEYS}
        assert np.array_equal(nb, z["shadow/nb"].astype(np.int32))  # (the search is the same)
        sums = hist.astype(np.float64).reshape(-1, 3, 11).sum(2)
        assert np.abs(sums - 100.0).max() < 1e-3
    finally:
        cl.close()


def test_cpp_fpfh_shim_runs_on_gpu(tmp_path, gpu_ctx, golden):
    """tests/cpp/shim_fpfh.cpp: the reference's normals + FPFH calls on double_shadow"""
    z, meta = golden
    shadow = z["shadow/points"]
    exe = tmp_path / "shim_fpfh"
    lib = os.path.dirname(D.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_fpfh.cpp"), "-o", str(exe), "-L", lib,
                    "-ldialog_amd", f"-Wl,-rpath,{lib}"], check=True)
    raw = tmp_path / "shadow.f32"
    shadow.tofile(str(raw))
    rn, r = meta["shadow"]["r_normals"], meta["shadow"]["radius"]
    out = subprocess.run([str(exe), str(raw), repr(rn), repr(r)], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.strip().splitlines()}
    nrm = D.estimate_normals(shadow, radius=rn, ctx=gpu_ctx)
    hist, nb, st = D.fpfh_estimation(shadow, nrm, r, ctx=gpu_ctx, return_stats=True)
    u = bits(hist).astype(object)
    w = np.arange(1, u.size + 1, dtype=object).reshape(u.shape)
    assert lines["rows"] == ["991", "991", str(int((u * w).sum()) % 2**64)]
    assert lines["stats"] == [str(st[q]) for q in ("n_finite", "n_nan_rows", "n_zero_rows",
                                                   "max_neighbours", "n_pairs", "n_pairs_failed")]
    assert lines["indices"] == ["331"] and lines["empty"] == ["0"]
