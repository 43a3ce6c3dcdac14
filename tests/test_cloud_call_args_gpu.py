"""GPU: the argument checks that the calls taking a cloud and an index list share
(csrc/call_args.hpp), driven through raw ctypes so that nothing is rejected in Python first.

Every bad row must come back as DLG_ERR_INVALID with a dlg_last_error text, hand out no cloud and
(the _cloud forms) leave the bytes held in device buffers as they were; after all rows of an entry
point a valid call on the same context returns the bytes it returned before them."""
import ctypes as C

import numpy as np
import pytest

from dialog_amd import _lib
from dialog_amd.sac import _f32p, _i32p

pytestmark = pytest.mark.gpu

f32 = np.float32
N = 64
NULL = "null"  # (a row's stand-in for a null record)

_rng = np.random.default_rng(20250)
# the records sit at the front of a larger allocation: a check that let a stride of 14 through
# would still read inside it
BACK = np.zeros((96, 3), f32)
BACK[:N] = _rng.uniform(-1.0, 1.0, (N, 3)).astype(f32)
BACK_T = np.zeros((96, 3), f32)
BACK_T[:N] = BACK[:N] + f32(0.01)
NRM = _rng.normal(size=(N, 3)).astype(f32)
NRM /= np.linalg.norm(NRM, axis=1, keepdims=True).astype(f32)
FEAT_S = _rng.uniform(0.0, 100.0, (N, 33)).astype(f32)
FEAT_T = _rng.uniform(0.0, 100.0, (N, 33)).astype(f32)
IDX = np.arange(0, N, 2, dtype=np.int32)
IDENT = np.eye(4, dtype=f32)


def points(back=BACK, n=N, stride=12, null_xyz=False):
    return _lib.Points(None if null_xyz else _f32p(back), n, stride)


def ref(p, back):
    """the dlg_points argument of a row: NULL, a record, or (None) the valid one"""
    if isinstance(p, str):
        return None
    return C.byref(points(back) if p is None else p)


def live(L, pinned=0):
    return L.dlg_debug_live_bytes(pinned)


# ---- one caller per entry point: (status, the bytes it wrote, the cloud it handed out) ------------
def _list(idx, n_idx):
    if idx is None:
        return None, 0
    return _i32p(idx), (idx.shape[0] if n_idx is None else n_idx)


def call_voxel(L, h, pts=None, idx=None, n_idx=None, out_stride=12):
    prm = _lib.VoxelParams((C.c_float * 3)(0.25, 0.25, 0.25), 0)
    ip, ni = _list(idx, n_idx)
    out = np.full((N, 5), -7.0, f32)
    cnt = np.full(N, -7, np.int32)
    voe = np.full(N, -7, np.int32)
    k = C.c_int64(-1)
    s = L.dlg_voxel_grid(h, ref(pts, BACK), ip, ni, C.byref(prm), _f32p(out), out_stride, N,
                         C.byref(k), _i32p(cnt), _i32p(voe), None)
    return s, (k.value, out.tobytes(), cnt.tobytes(), voe.tobytes()), None


def call_voxel_cloud(L, h, pts=None, idx=None, n_idx=None):
    prm = _lib.VoxelParams((C.c_float * 3)(0.25, 0.25, 0.25), 0)
    ip, ni = _list(idx, n_idx)
    voe = np.full(N, -7, np.int32)
    k = C.c_int64(-1)
    cl = C.c_void_p(0xdead)
    s = L.dlg_voxel_grid_cloud(h, ref(pts, BACK), ip, ni, C.byref(prm), 0, C.byref(cl),
                               C.byref(k), _i32p(voe), None)
    return s, (k.value, voe.tobytes()), cl.value


def call_sor(L, h, pts=None, idx=None, n_idx=None):
    prm = _lib.SorParams(4, 0, 1.0)
    ip, ni = _list(idx, n_idx)
    kept = np.full(N, -7, np.int32)
    rem = np.full(N, -7, np.int32)
    dist = np.full(N, -7.0, f32)
    nk, nr = C.c_int64(-1), C.c_int64(-1)
    s = L.dlg_statistical_outlier_removal(h, ref(pts, BACK), ip, ni, C.byref(prm), _i32p(kept), N,
                                          C.byref(nk), _i32p(rem), N, C.byref(nr), _f32p(dist),
                                          None)
    return s, (nk.value, nr.value, kept.tobytes(), rem.tobytes(), dist.tobytes()), None


def call_sor_cloud(L, h, pts=None, idx=None, n_idx=None):
    prm = _lib.SorParams(4, 0, 1.0)
    ip, ni = _list(idx, n_idx)
    kept = np.full(N, -7, np.int32)
    nk = C.c_int64(-1)
    cl = C.c_void_p(0xdead)
    s = L.dlg_statistical_outlier_removal_cloud(h, ref(pts, BACK), ip, ni, C.byref(prm), 0,
                                                C.byref(cl), C.byref(nk), _i32p(kept), None)
    return s, (nk.value, kept.tobytes()), cl.value


def call_mls(L, h, pts=None, idx=None, n_idx=None, out_stride=12):
    prm = _lib.MlsParams(0.6, 1, 2, 1, 0.0)
    ip, ni = _list(idx, n_idx)
    xyz = np.full((N, 5), -7.0, f32)
    nrm = np.full((N, 4), -7.0, f32)
    src = np.full(N, -7, np.int32)
    nb = np.full(N, -7, np.int32)
    k = C.c_int64(-1)
    s = L.dlg_moving_least_squares(h, ref(pts, BACK), ip, ni, C.byref(prm), _f32p(xyz), out_stride,
                                   _f32p(nrm), N, C.byref(k), _i32p(src), _i32p(nb), None)
    return s, (k.value, xyz.tobytes(), nrm.tobytes(), src.tobytes(), nb.tobytes()), None


def call_mls_cloud(L, h, pts=None, idx=None, n_idx=None):
    prm = _lib.MlsParams(0.6, 1, 2, 1, 0.0)
    ip, ni = _list(idx, n_idx)
    src = np.full(N, -7, np.int32)
    k = C.c_int64(-1)
    cl = C.c_void_p(0xdead)
    s = L.dlg_moving_least_squares_cloud(h, ref(pts, BACK), ip, ni, C.byref(prm), 0, C.byref(cl),
                                         C.byref(k), _i32p(src), None)
    return s, (k.value, src.tobytes()), cl.value


def call_fpfh(L, h, pts=None, idx=None, n_idx=None):
    prm = _lib.FpfhParams(0.6)
    ip, ni = _list(idx, n_idx)
    hist = np.full((N, 33), -7.0, f32)
    nb = np.full(N, -7, np.int32)
    s = L.dlg_fpfh_estimate(h, ref(pts, BACK), _f32p(NRM), 12, ip, ni, C.byref(prm), _f32p(hist),
                            132, _i32p(nb), None, None)
    return s, (hist.tobytes(), nb.tobytes()), None


def call_icp_align(L, h, pts=None, tgt=None, idx=None, n_idx=None, out_stride=12, guess=None):
    prm = _lib.IcpParams()
    L.dlg_icp_params_default(C.byref(prm))
    prm.max_iterations = 3
    ip, ni = _list(idx, n_idx)
    fin = np.full(16, -7.0, f32)
    out = np.full((N, 5), -7.0, f32)
    s = L.dlg_icp_align(h, ref(pts, BACK), ip, ni, ref(tgt, BACK_T), C.byref(prm),
                        None if guess is None else _f32p(guess), _f32p(fin), _f32p(out),
                        out_stride, None, 0, None)
    return s, (fin.tobytes(), out.tobytes()), None


def call_icp_corr(L, h, pts=None, tgt=None, idx=None, n_idx=None, guess=None):
    ip, ni = _list(idx, n_idx)
    nn = np.full(N, -7, np.int32)
    d2 = np.full(N, -7.0, f32)
    k = C.c_int64(-1)
    s = L.dlg_icp_correspondences(h, ref(pts, BACK), ip, ni, ref(tgt, BACK_T),
                                  None if guess is None else _f32p(guess), 0.5, _i32p(nn),
                                  _f32p(d2), C.byref(k))
    return s, (k.value, nn.tobytes(), d2.tobytes()), None


def call_sacia_score(L, h, pts=None, tgt=None):
    xf = np.stack([IDENT, IDENT]).copy()
    xf[1, 0, 3] = 0.05
    hyp = (_lib.SacIaHypothesis * 2)()
    s = L.dlg_sac_ia_score(h, ref(pts, BACK), ref(tgt, BACK_T), _f32p(xf), 2, 0.5, 0, 0, hyp)
    return s, (bytes(hyp),), None


def call_sacia_align(L, h, pts=None, tgt=None, out_stride=12, guess=None):
    prm = _lib.SacIaParams()
    L.dlg_sac_ia_params_default(C.byref(prm))
    prm.max_iterations = 8
    prm.k_correspondences = 2
    prm.max_correspondence_distance = 0.5
    fin = np.full(16, -7.0, f32)
    out = np.full((N, 5), -7.0, f32)
    s = L.dlg_sac_ia_align(h, ref(pts, BACK), _f32p(FEAT_S), 132, ref(tgt, BACK_T), _f32p(FEAT_T),
                           132, C.byref(prm), None if guess is None else _f32p(guess), _f32p(fin),
                           _f32p(out), out_stride, None, 0, None)
    return s, (fin.tobytes(), out.tobytes()), None


# ---- the bad rows ------------------------------------------------------------------------------------
def cloud_rows(key, back):
    return [
        (f"{key}: null record", {key: NULL}),
        (f"{key}: n = -1", {key: points(back, n=-1)}),
        (f"{key}: xyz null, n > 0", {key: points(back, null_xyz=True)}),
        (f"{key}: stride 8", {key: points(back, stride=8)}),
        (f"{key}: stride 14", {key: points(back, stride=14)}),
    ]


def list_rows():
    low, high = IDX.copy(), IDX.copy()
    low[5] = -1
    high[7] = N
    return [
        ("list: n_indices = -1", {"idx": IDX, "n_idx": -1}),
        ("list: entry -1", {"idx": low}),
        ("list: entry n", {"idx": high}),
    ]


def guess_rows():
    nan, inf = IDENT.copy(), IDENT.copy()
    nan[1, 2] = np.nan
    inf[3, 0] = np.inf
    return [("guess: one NaN", {"guess": nan}), ("guess: one inf", {"guess": inf})]


STRIDE_ROW = [("out_stride_bytes = 20", {"out_stride": 20})]
PTS = cloud_rows("pts", BACK)
TGT = cloud_rows("tgt", BACK_T)

# entry point -> (caller, keywords of its valid call, bad rows)
CASES = {
    "dlg_voxel_grid": (call_voxel, {"idx": IDX}, PTS + list_rows() + STRIDE_ROW),
    "dlg_voxel_grid_cloud": (call_voxel_cloud, {"idx": IDX}, PTS + list_rows()),
    "dlg_statistical_outlier_removal": (call_sor, {"idx": IDX}, PTS + list_rows()),
    "dlg_statistical_outlier_removal_cloud": (call_sor_cloud, {"idx": IDX}, PTS + list_rows()),
    "dlg_moving_least_squares": (call_mls, {"idx": IDX}, PTS + list_rows() + STRIDE_ROW),
    "dlg_moving_least_squares_cloud": (call_mls_cloud, {"idx": IDX}, PTS + list_rows()),
    "dlg_fpfh_estimate": (call_fpfh, {"idx": IDX}, PTS + list_rows()),
    "dlg_icp_align": (call_icp_align, {"idx": IDX},
                      PTS + TGT + list_rows() + STRIDE_ROW + guess_rows()),
    "dlg_icp_correspondences": (call_icp_corr, {"idx": IDX}, PTS + TGT + list_rows() + guess_rows()),
    "dlg_sac_ia_score": (call_sacia_score, {}, PTS + TGT),
    "dlg_sac_ia_align": (call_sacia_align, {}, PTS + TGT + STRIDE_ROW + guess_rows()),
}


@pytest.mark.parametrize("entry", sorted(CASES))
def test_bad_rows_are_invalid_and_leave_nothing_behind(gpu_ctx, entry):
    L = _lib.load()
    h = gpu_ctx.h
    call, valid, rows = CASES[entry]
    hands_out_a_cloud = entry.endswith("_cloud")

    def valid_call():
        s, out, cl = call(L, h, **valid)
        assert s == _lib.DLG_OK, L.dlg_last_error(h)
        if hands_out_a_cloud:
            assert cl not in (None, 0xdead)
            assert L.dlg_cloud_destroy(cl) == _lib.DLG_OK
        return out

    before = valid_call()
    for name, kw in rows:
        held = live(L)
        s, _, cl = call(L, h, **{**valid, **kw})
        assert s == _lib.DLG_ERR_INVALID, (entry, name, s)
        assert L.dlg_last_error(h), (entry, name)
        if hands_out_a_cloud:
            assert cl is None, (entry, name)  # (*out was set to null)
            assert live(L) == held, (entry, name)
    assert valid_call() == before
