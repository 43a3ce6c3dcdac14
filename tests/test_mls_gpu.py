"""GPU: dlg_moving_least_squares / dlg_moving_least_squares_cloud against tests/mls_ref.py (the
numpy restatement of pcl::MovingLeastSquares), through the fixture tests/golden/mls_small.npz.

The parity rule (tests/test_mls.py): n_out, src_index, neighbours and the branch counts equal the
reference's; at the reference's stable rows every one of the 7 float components is within 1 float
ulp and at least 99 % of them are bit-equal.  shadow_r01 and any case outside M.QUALIFYING: the
exact part only."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import dialog_amd as D
import mls_ref as M
from dialog_amd import _lib
from dialog_amd.sac import _f32p, _i32p
from dialog_amd.synth import plane_cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mls_small.npz"))
    return z, json.loads(str(z["meta"]))


def raw_call(ctx, pts, radius, order=2, fit=1, normals=1, sqr_gauss=0.0, idx=None, cap=None,
             out_stride=12, want_normals=True, want_src=True, want_nb=True, want_stats=True):
    """dlg_moving_least_squares through ctypes"""
    L = _lib.load()
    a = np.ascontiguousarray(pts, f32)
    P = _lib.Points(_f32p(a), a.shape[0], 4 * a.shape[1])
    prm = _lib.MlsParams(float(radius), int(fit), int(order), int(normals), float(sqr_gauss))
    ix = None if idx is None else np.ascontiguousarray(idx, np.int32)
    n = a.shape[0] if ix is None else ix.shape[0]
    cap = n if cap is None else cap
    sf = out_stride // 4
    xyz = np.full((max(cap, 1), sf), -7.0, f32)
    nrm = np.full((max(cap, 1), 4), -7.0, f32)
    src = np.full(max(cap, 1), -7, np.int32)
    nb = np.full(max(n, 1), -7, np.int32)
    k = C.c_int64(-1)
    st = _lib.MlsStats()
    s = L.dlg_moving_least_squares(
        ctx.h, C.byref(P), None if ix is None else _i32p(ix), n if ix is not None else 0,
        C.byref(prm), _f32p(xyz), out_stride, _f32p(nrm) if want_normals else None, cap,
        C.byref(k), _i32p(src) if want_src else None, _i32p(nb) if want_nb else None,
        C.byref(st) if want_stats else None)
    return dict(status=s, n_out=k.value, xyz=xyz, normals=nrm, src=src, nb=nb[:n], stats=st)


def check_case(ctx, golden, name, **over):
    """one fixture case through the C ABI under the parity rule -> the call's result"""
    z, meta = golden
    m = dict(meta[name])
    pts = z[name + "/points"]
    idx = z[name + "/idx"] if name + "/idx" in z.files else None
    r = raw_call(ctx, pts, m["radius"], order=m.get("poly_order", 2),
                 fit=int(m.get("polynomial_fit", True)), normals=int(m.get("compute_normals", True)),
                 sqr_gauss=m.get("sqr_gauss_param", 0.0), idx=idx, **over)
    assert r["status"] == 0, _lib.load().dlg_last_error(ctx.h)
    want = dict(zip(M.STAT_KEYS, z[name + "/stats"]))
    k = r["n_out"]
    # exact: the counts, the index values, the neighbour counts, the branches
    assert k == want["n_out"] == len(z[name + "/src"])
    assert np.array_equal(r["src"][:k], z[name + "/src"])
    assert np.array_equal(r["nb"], z[name + "/nb"])
    st = r["stats"]
    assert {q: getattr(st, q) for q in M.STAT_KEYS} == want
    assert st.n_lds_overflow == int((z[name + "/nb"] > 1024).sum())
    # values at the stable rows
    if name in M.QUALIFYING:
        got = np.concatenate([r["xyz"][:k, :3], r["normals"][:k]], 1)
        stable = z[name + "/stable"]
        assert (~stable).sum() <= 0.01 * len(stable)
        mx, eq = M.value_rule(got, z[name + "/rows"], stable)
        print(f"{name}: {k} rows, max {mx} ulp, {100 * eq:.3f} % bit-equal at "
              f"{int(stable.sum())} stable rows")
        assert mx <= 1 and eq >= 0.99, (name, mx, eq)
    return r


# ---- the inputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wave_o1", "wave_o2", "wave_o3", "sphere", "sparse", "shadow_r02",
                                  "shadow_r04", "shadow_r01", "blob", "blob600"])
def test_parity_on_the_inputs(gpu_ctx, golden, name):
    check_case(gpu_ctx, golden, name)


def test_blob_takes_the_reread_path_and_blob600_does_not(gpu_ctx, golden):
    """1100 neighbours are past the on-chip buffer (the same rows come from the grid's candidates
    read three more times); 600 are staged"""
    assert check_case(gpu_ctx, golden, "blob")["stats"].n_lds_overflow == 1100
    assert check_case(gpu_ctx, golden, "blob600")["stats"].n_lds_overflow == 0


# ---- options -----------------------------------------------------------------------------------------
def test_polynomial_fit_off(gpu_ctx, golden):
    r = check_case(gpu_ctx, golden, "opt_nofit")
    assert r["stats"].n_plane_only == r["n_out"] == 700


def test_compute_normals_off(gpu_ctx, golden):
    z, _ = golden
    r = check_case(gpu_ctx, golden, "opt_nonormals")
    assert (bits(r["normals"][:r["n_out"]]) == 0).all()
    # the positions are those of the run with normals, and out_normals may be NULL
    on = raw_call(gpu_ctx, z["opt_nonormals/points"], 0.1)
    assert np.array_equal(bits(on["xyz"][:700]), bits(r["xyz"][:700]))
    assert (on["normals"][:700, :3] != 0).any()
    null = raw_call(gpu_ctx, z["opt_nonormals/points"], 0.1, normals=0, want_normals=False)
    assert null["status"] == 0 and null["n_out"] == 700
    assert np.array_equal(bits(null["xyz"][:700]), bits(r["xyz"][:700]))
    assert (null["normals"] == -7).all()


def test_sqr_gauss_param(gpu_ctx, golden):
    z, _ = golden
    r = check_case(gpu_ctx, golden, "opt_gauss")
    dflt = raw_call(gpu_ctx, z["opt_gauss/points"], 0.1)
    assert (bits(dflt["xyz"][:700]) != bits(r["xyz"][:700])).mean() > 0.5
    # <= 0 is the default, r^2, and so is r^2 itself
    r2 = float(np.float64(f32(0.1)) ** 2)
    for g in (-1.0, r2):
        e = raw_call(gpu_ctx, z["opt_gauss/points"], 0.1, sqr_gauss=g)
        assert np.array_equal(bits(e["xyz"][:700]), bits(dflt["xyz"][:700]))
        assert np.array_equal(bits(e["normals"][:700]), bits(dflt["normals"][:700]))


def test_index_lists(gpu_ctx, golden):
    """permuted, duplicated, a subset: the rows are the whole-cloud rows of the entries"""
    z, _ = golden
    r = check_case(gpu_ctx, golden, "opt_index")
    idx = z["opt_index/idx"]
    whole = raw_call(gpu_ctx, z["opt_index/points"], 0.1)
    assert whole["n_out"] == 700
    assert np.array_equal(bits(r["xyz"][:500]), bits(whole["xyz"][idx]))
    assert np.array_equal(bits(r["normals"][:500]), bits(whole["normals"][idx]))
    # an empty list: nothing out, the finite points still counted
    e = raw_call(gpu_ctx, z["opt_index/points"], 0.1, idx=np.zeros(0, np.int32))
    assert e["status"] == 0 and e["n_out"] == 0 and e["stats"].n_finite == 700


def test_nonfinite_points(gpu_ctx, golden):
    """NaN and inf points in the cloud and as queries: no row, neighbours -1, never a neighbour"""
    z, _ = golden
    r = check_case(gpu_ctx, golden, "opt_nonfinite")
    assert (r["nb"][[5, 77, 300, 699]] == -1).all() and r["stats"].n_finite == 696
    assert np.isfinite(r["xyz"][:r["n_out"]]).all()
    r = check_case(gpu_ctx, golden, "opt_nonfinite_index")
    assert (r["nb"][-5:] == -1).all()
    allnan = raw_call(gpu_ctx, np.full((10, 3), np.nan, f32), 0.1)
    assert allnan["status"] == 0 and allnan["n_out"] == 0 and allnan["stats"].n_finite == 0
    assert (allnan["nb"] == -1).all()


def test_identical_points(gpu_ctx, golden):
    """covariance 0: eigen33's scale guard, a singular A, c[0] not finite, the projection stands"""
    r = check_case(gpu_ctx, golden, "identical")
    assert r["stats"].n_fit_nonfinite == 40


def test_strides(gpu_ctx, golden):
    z, _ = golden
    pts = z["sparse/points"]
    a = check_case(gpu_ctx, golden, "sparse")
    k = a["n_out"]
    wide = np.full((len(pts), 4), np.nan, f32)  # (16-byte input records: the pad is never read)
    wide[:, :3] = pts
    b = raw_call(gpu_ctx, wide, 0.08, out_stride=16)
    assert b["status"] == 0 and b["n_out"] == k
    assert np.array_equal(bits(b["xyz"][:k, :3]), bits(a["xyz"][:k]))
    assert (b["xyz"][:k, 3] == 1.0).all() and (b["xyz"][k:] == -7).all()
    assert np.array_equal(bits(b["normals"][:k]), bits(a["normals"][:k]))
    assert raw_call(gpu_ctx, pts, 0.08, out_stride=20)["status"] == _lib.DLG_ERR_INVALID


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_tiny_clouds(gpu_ctx, golden, n):
    z, _ = golden
    p = z["wave_o2/points"][:3].copy()
    p[1] = p[0] + f32(0.01)
    p[2] = p[0] - f32(0.01)
    p = p[:n]
    ref = M.mls_ref(p, 0.08)
    r = raw_call(gpu_ctx, p, 0.08)
    assert r["status"] == 0 and r["n_out"] == ref["stats"]["n_out"] == (3 if n == 3 else 0)
    assert np.array_equal(r["nb"], ref["neighbours"])
    assert {q: getattr(r["stats"], q) for q in M.STAT_KEYS} == ref["stats"]
    if n == 3:  # 3 collinear points: the plane branch (a rank-1 covariance: the exact part only)
        assert np.array_equal(r["src"][:3], [0, 1, 2]) and r["stats"].n_plane_only == 3


# ---- status codes ---------------------------------------------------------------------------------
def test_status_codes(gpu_ctx, golden):
    z, _ = golden
    L = _lib.load()
    pts = z["sphere/points"]
    k = int(z["sphere/stats"][1])
    r = raw_call(gpu_ctx, pts, 0.15, cap=k - 1)
    assert r["status"] == _lib.DLG_ERR_CAPACITY and r["n_out"] == k
    assert b"need " + str(k).encode() in L.dlg_last_error(gpu_ctx.h)
    assert (r["xyz"] == -7).all() and (r["src"] == -7).all()  # nothing written
    assert raw_call(gpu_ctx, pts, 0.15, cap=k)["status"] == 0
    for order in (0, 4, -1):
        assert raw_call(gpu_ctx, pts, 0.15, order=order)["status"] == _lib.DLG_ERR_INVALID
    assert b"polynomial_order" in L.dlg_last_error(gpu_ctx.h)
    for radius in (0.0, -1.0, np.nan, np.inf):
        assert raw_call(gpu_ctx, pts, radius)["status"] == _lib.DLG_ERR_INVALID
    assert b"search_radius" in L.dlg_last_error(gpu_ctx.h)
    for bad in ([0, len(pts)], [-1]):
        assert raw_call(gpu_ctx, pts, 0.15, idx=bad)["status"] == _lib.DLG_ERR_INVALID
    # every optional output may be NULL
    r = raw_call(gpu_ctx, pts, 0.15, want_normals=False, want_src=False, want_nb=False,
                 want_stats=False)
    assert r["status"] == 0 and r["n_out"] == k


def test_several_ranks_are_refused(golden):
    """a context of a 2-rank communicator holds a shard: DLG_ERR_INVALID, and no collective runs"""
    z, _ = golden
    pts = z["sphere/points"]
    ctxs = D.Context.loopback_group(2, 0)
    try:
        r = raw_call(ctxs[0], pts, 0.15)
        assert r["status"] == _lib.DLG_ERR_INVALID
        assert b"world > 1" in _lib.load().dlg_last_error(ctxs[0].h)
        with pytest.raises(D.DialogError):
            D.moving_least_squares_cloud(pts, 0.15, ctx=ctxs[1])
    finally:
        for c in ctxs:
            c.close()


# ---- the Python mirror -----------------------------------------------------------------------------
def test_python_mirror_and_stats(gpu_ctx, golden):
    z, _ = golden
    pts = z["sparse/points"]
    xyz, nrm, src, nb, st = D.moving_least_squares(pts, 0.08, ctx=gpu_ctx, return_stats=True)
    r = raw_call(gpu_ctx, pts, 0.08)
    k = r["n_out"]
    assert xyz.shape == (k, 3) and nrm.shape == (k, 4) and src.shape == (k,) and len(nb) == len(pts)
    assert np.array_equal(bits(xyz), bits(r["xyz"][:k])) and np.array_equal(src, r["src"][:k])
    assert np.array_equal(bits(nrm), bits(r["normals"][:k])) and np.array_equal(nb, r["nb"])
    assert {q: st[q] for q in M.STAT_KEYS} == dict(zip(M.STAT_KEYS, z["sparse/stats"]))
    assert st["n_lds_overflow"] == 0 and st["device_ms"] >= 0
    o3 = D.moving_least_squares(pts, 0.08, order=3, polynomial_fit=True, compute_normals=False,
                                sqr_gauss_param=0.01, indices=[4, 4, 9], ctx=gpu_ctx)
    assert list(o3[2]) == [4, 4, 9] and (o3[1] == 0).all()
    with pytest.raises(D.DialogError):
        D.moving_least_squares(pts, 0.08, order=7, ctx=gpu_ctx)


# ---- the shim ---------------------------------------------------------------------------------------
def test_cpp_mls_shim_runs_on_gpu(tmp_path, gpu_ctx, golden):
    """tests/cpp/shim_mls.cpp: on_rebuildPlaneAction_triggered's calls on double_shadow"""
    z, _ = golden
    shadow = z["shadow_r04/points"]
    exe = tmp_path / "shim_mls"
    lib = os.path.dirname(D.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_mls.cpp"), "-o", str(exe), "-L", lib,
                    "-ldialog_amd", f"-Wl,-rpath,{lib}"], check=True)
    raw = tmp_path / "shadow.f32"
    shadow.tofile(str(raw))
    out = subprocess.run([str(exe), str(raw), "0.04"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.strip().splitlines()}
    xyz, nrm, src, nb, st = D.moving_least_squares(shadow, 0.04, ctx=gpu_ctx, return_stats=True)

    def bsum(a):
        u = bits(a)
        return sum((i * 7 + j + 1) * int(u[i, j]) for i in range(len(u)) for j in range(u.shape[1]))

    sp = bsum(xyz)
    sn = bsum(nrm[:, :3]) + sum(int((i * 7 + 1) * int(b)) for i, b in enumerate(bits(nrm[:, 3])))
    si = sum((i + 1) * int(s) for i, s in enumerate(src))
    m = 2**64
    assert lines["rows"] == ["991", "991", str(sp % m), str(sn % m), str(si % m)]
    assert lines["stats"] == [str(st[q]) for q in ("n_finite", "n_too_few", "n_plane_only",
                                                   "n_fit_nonfinite", "max_neighbours")]
    assert lines["plane"] == ["991", "991"] and lines["empty"] == ["0"]


# ---- the device-resident result -------------------------------------------------------------------
@pytest.fixture(scope="module")
def mls_clouds(gpu_ctx):
    """about 20,000 points of three noisy planes, smoothed both ways: to the host and re-uploaded
    with its normals, and left on the device"""
    p, _, _ = plane_cloud(20000, 3, outlier_frac=0.02, seed=78)
    xyz, nrm, src, nb = D.moving_least_squares(p, 0.3, ctx=gpu_ctx)
    up = D.Cloud(gpu_ctx, xyz, id_base=500)
    up.set_normals(nrm)
    dev, src_d, st = D.moving_least_squares_cloud(p, 0.3, id_base=500, ctx=gpu_ctx,
                                                  return_stats=True)
    yield p, xyz, nrm, src, up, dev, src_d, st
    up.close()
    dev.close()


def test_mls_cloud_equals_upload_of_the_host_result(mls_clouds):
    p, xyz, nrm, src, up, dev, src_d, st = mls_clouds
    assert 0 < len(xyz) <= len(p) and st["n_out"] == len(xyz)
    assert np.array_equal(src, src_d)
    assert dev.n == up.n == len(xyz) and dev.n_active == up.n_active
    assert dev.signature() == up.signature()


def test_mls_cloud_planes_equal(mls_clouds):
    """SACMODEL_PLANE and SACMODEL_NORMAL_PLANE (the attached normals are the host call's)"""
    p, xyz, nrm, src, up, dev, _, _ = mls_clouds
    for model in (D.SACMODEL_PLANE, D.SACMODEL_NORMAL_PLANE):
        prm = D.make_params(0.02, max_iterations=200, probability=0.99, model=model)
        ra = D.extract_planes(up, prm, max_planes=3)
        rb = D.extract_planes(dev, prm, max_planes=3)
        assert ra["n_planes"] == rb["n_planes"] >= 1
        assert np.array_equal(bits(ra["coeffs"]), bits(rb["coeffs"]))
        assert np.array_equal(ra["offsets"], rb["offsets"])
        assert np.array_equal(ra["inliers"], rb["inliers"])
        up.reset()
        dev.reset()


def test_mls_cloud_without_normals(gpu_ctx, golden):
    z, _ = golden
    pts = z["sparse/points"]
    dev, src = D.moving_least_squares_cloud(pts, 0.08, compute_normals=False, ctx=gpu_ctx)
    xyz = D.moving_least_squares(pts, 0.08, compute_normals=False, ctx=gpu_ctx)[0]
    up = D.Cloud(gpu_ctx, xyz)
    try:
        assert dev.n == up.n == int(z["sparse/stats"][1]) and np.array_equal(src, z["sparse/src"])
        assert dev.signature() == up.signature()
    finally:
        dev.close()
        up.close()
