"""GPU: who owns device memory.  Every DevBuf / PinBuf frees itself when its owner goes (csrc/
driver.hpp), and dlg_debug_live_bytes counts what this process holds: the device is shared, so a
device-wide free-memory reading could not show a leak, this count can."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import dialog_amd as D
from dialog_amd import _lib
from dialog_amd.features import fpfh_estimation
from dialog_amd.sac import _f32p, _i32p
from dialog_amd.synth import plane_cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def live():
    """(device bytes, pinned bytes) held right now; clouds that tests before this one dropped
    without closing are collected first, so that none of them goes in the middle of a reading"""
    gc.collect()
    L = _lib.load()
    return L.dlg_debug_live_bytes(0), L.dlg_debug_live_bytes(1)


def test_float_sums_frees_its_scratch():
    xyz = np.random.default_rng(5).uniform(-1, 1, (1000, 3)).astype(f32)
    ctx = D.Context(0)
    held = []
    for _ in range(5):
        ctx.float_sums(xyz, walk_stats=True)
        held.append(live())
    ctx.close()
    assert held[4] == held[0], held


def test_a_context_and_its_cloud_give_everything_back():
    z = np.load(os.path.join(ROOT, "tests", "golden", "normal_plane_small.npz"))
    pts, _, _ = plane_cloud(1500, 3, seed=11)
    tgt = (pts + f32(0.01)).astype(f32)
    nrm = np.zeros((pts.shape[0], 3), f32)
    nrm[:, 2] = 1.0
    feats = np.random.default_rng(6).uniform(0, 100, (pts.shape[0], 33)).astype(f32)
    idx = np.arange(0, pts.shape[0], 3, dtype=np.int32)
    before = live()

    ctx = D.Context(0)
    ctx.set_option(D.DLG_OPT_PRUNE, 1)  # (applies at upload: the cloud gets its spatial copy)
    ctx.set_option(D.DLG_OPT_PRUNE_NP, 1)
    cloud = D.Cloud(ctx, z["points"])
    cloud.set_normals(z["normals"])
    prm = D.make_params(float(z["ex_threshold"]), max_iterations=int(z["ex_max_iterations"]),
                        probability=1.0, model=D.SACMODEL_NORMAL_PLANE,
                        normal_distance_weight=float(z["ex_lambda"]))
    ctx.set_option(D.DLG_OPT_PRUNE_STATS, 1)
    e = D.extract_planes(cloud, prm, max_planes=int(z["ex_max_planes"]),
                         min_inliers=int(z["ex_min_inliers"]))
    assert e["n_planes"] >= 1
    # the pruned NORMAL_PLANE scorer ran: its normals buffer (np_cn) is allocated
    assert ctx.prune_stats()["pairs"] > 0
    # one call of each of the six drivers
    D.voxel_grid(pts, 0.1, indices=idx, ctx=ctx)
    D.statistical_outlier_removal(pts, 8, 1.0, indices=idx, ctx=ctx)
    D.moving_least_squares(pts, 0.2, indices=idx, ctx=ctx)
    fpfh_estimation(pts, nrm, 0.2, indices=idx, ctx=ctx)
    D.icp_align(pts, tgt, indices=idx, max_iterations=2, ctx=ctx)
    D.sac_ia_align(pts, feats, tgt, feats, max_iterations=8, k_correspondences=2,
                   fitness_max_range=1.0, ctx=ctx)
    during = live()
    assert during[0] > before[0] and during[1] > before[1]
    cloud.close()
    ctx.close()
    assert live() == before


def test_a_failed_upload_frees_its_cloud(gpu_ctx):
    """an out-of-range index in a list long enough for the device gather (4 m >= n)"""
    L = _lib.load()
    pts, _, _ = plane_cloud(4000, 2, seed=12)
    idx = np.arange(0, 4000, 2, dtype=np.int32)
    D.Cloud(gpu_ctx, pts, indices=idx).close()  # (the context's own staging is grown here)
    idx[1500] = 4000
    P = _lib.Points(_f32p(pts), pts.shape[0], 12)
    before = live()
    h = C.c_void_p(0xdead)
    s = L.dlg_cloud_upload(gpu_ctx.h, C.byref(P), _i32p(idx), idx.shape[0], 0, C.byref(h))
    assert s == _lib.DLG_ERR_INVALID and h.value is None
    assert b"index out of range" in L.dlg_last_error(gpu_ctx.h)
    assert live() == before
