"""GPU: dlg_voxel_grid / dlg_voxel_grid_cloud bit for bit against tests/voxel_ref.py (the numpy
restatement of pcl::VoxelGrid's applyFilter with list order inside a voxel), at every shape where
the device path changes: tiny clouds, the occupancy ladder around the wave width under every
long-run cut-off, one voxel for the whole cloud, non-finite entries, index lists, strides,
min_points, the status codes, and the device-resident result as a cloud.

Run once against two wrong implementations (recorded in DESIGN.md §5e): summing a voxel's members
in descending sorted position fails 17 of these tests, the uniform fixture and the ladder among
them; forming the key in double precision fails the quantised fixture."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dialog_amd as D
import voxel_ref as V
from dialog_amd import _lib
from dialog_amd.sac import _f32p, _i32p
from dialog_amd.synth import plane_cloud

pytestmark = pytest.mark.gpu

INT32_MAX = 2**31 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def raw_call(ctx, pts, leaf, idx=None, min_points=0, out_stride=12, cap=None, want_counts=True,
             want_voe=True):
    """dlg_voxel_grid through ctypes -> (status, n_out, out [cap, stride / 4], counts, voe, stats)"""
    L = _lib.load()
    a = np.ascontiguousarray(pts, np.float32)
    P = _lib.Points(_f32p(a), a.shape[0], 4 * a.shape[1])
    lf = np.broadcast_to(np.asarray(leaf, np.float32), (3,))
    prm = _lib.VoxelParams((C.c_float * 3)(*[float(v) for v in lf]), int(min_points))
    ix = None if idx is None else np.ascontiguousarray(idx, np.int32)
    n = a.shape[0] if ix is None else ix.shape[0]
    cap = n if cap is None else cap
    out = np.full((max(cap, 1), out_stride // 4), -7.0, np.float32)
    cnt = np.full(max(cap, 1), -7, np.int32)
    voe = np.full(max(n, 1), -7, np.int32)
    k = C.c_int64(-1)
    st = _lib.VoxelStats()
    s = L.dlg_voxel_grid(ctx.h, C.byref(P), None if ix is None else _i32p(ix),
                         n if ix is not None else 0, C.byref(prm), _f32p(out), out_stride, cap,
                         C.byref(k), _i32p(cnt) if want_counts else None,
                         _i32p(voe) if want_voe else None, C.byref(st))
    return s, k.value, out, cnt, voe[:n], st


def check_equal(ctx, pts, leaf, idx=None, min_points=0, out_stride=12):
    ref = V.voxel_ref(pts, leaf, idx=idx, min_points=min_points)
    s, k, out, cnt, voe, st = raw_call(ctx, pts, leaf, idx, min_points, out_stride)
    assert s == 0, _lib.load().dlg_last_error(ctx.h)
    assert k == len(ref["xyz"])
    assert np.array_equal(bits(out[:k, :3]), bits(ref["xyz"]))
    if out_stride == 16:
        assert (out[:k, 3] == 1.0).all()
    assert np.array_equal(cnt[:k], ref["counts"])
    assert np.array_equal(voe, ref["voe"])
    assert st.n_finite == ref["n_finite"] and st.n_voxels == ref["n_voxels"]
    if ref["div"] is not None:
        assert list(st.div) == list(ref["div"]) and list(st.min_b) == list(ref["min_b"])
    return ref


@pytest.fixture(scope="module")
def uniform():
    return V.uniform_cloud()


def test_uniform_fixture(gpu_ctx, uniform):
    ref = check_equal(gpu_ctx, uniform, 0.25)
    assert len(ref["xyz"]) == 4067 and ref["counts"].max() == 17
    # the Python mirror
    xyz, cnt, voe, st = D.voxel_grid(uniform, 0.25, ctx=gpu_ctx, return_stats=True)
    assert np.array_equal(bits(xyz), bits(ref["xyz"])) and np.array_equal(cnt, ref["counts"])
    assert np.array_equal(voe, ref["voe"]) and st["n_voxels"] == 4067


def test_quantised_fixture(gpu_ctx):
    """coordinates on multiples of 0.1f, leaf 0.1: every point sits on a cell boundary, where only
    the float product floorf((x * inv)_f32) gives PCL's cell"""
    check_equal(gpu_ctx, V.quantised_cloud(), 0.1)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65])
def test_tiny_clouds(gpu_ctx, uniform, n):
    check_equal(gpu_ctx, uniform[:n], 0.25)
    check_equal(gpu_ctx, uniform[:n] + np.float32(3), 100.0)  # (all in one voxel)


@pytest.fixture(scope="module")
def ladder():
    p = V.ladder_cloud()
    ref = V.voxel_ref(p, 1.0)
    assert sorted(ref["counts"]) == sorted(V.LADDER)
    return p, ref


@pytest.mark.parametrize("long_run", [1, 64, None, INT32_MAX])
def test_occupancy_ladder_every_cutoff(gpu_ctx, ladder, long_run):
    """voxels of exactly 1, 2, 3, 31..33, 63..65, 127..129 and 1000 points; the wave kernel takes
    the voxels of >= DLG_OPT_VOXEL_LONG_RUN points: identical bits for every cut-off"""
    p, ref = ladder
    default = gpu_ctx.get_option(D.DLG_OPT_VOXEL_LONG_RUN)
    try:
        if long_run is not None:
            gpu_ctx.set_option(D.DLG_OPT_VOXEL_LONG_RUN, long_run)
            assert gpu_ctx.get_option(D.DLG_OPT_VOXEL_LONG_RUN) == long_run
        s, k, out, cnt, voe, _ = raw_call(gpu_ctx, p, 1.0)
    finally:
        gpu_ctx.set_option(D.DLG_OPT_VOXEL_LONG_RUN, default)
    assert s == 0 and k == len(V.LADDER)
    assert np.array_equal(bits(out[:k]), bits(ref["xyz"]))
    assert np.array_equal(cnt[:k], ref["counts"]) and np.array_equal(voe, ref["voe"])


def test_long_run_option_range(gpu_ctx):
    with pytest.raises(D.DialogError):
        gpu_ctx.set_option(D.DLG_OPT_VOXEL_LONG_RUN, 0)


@pytest.mark.parametrize("long_run", [1, None, INT32_MAX])
def test_one_voxel_for_the_whole_cloud(gpu_ctx, uniform, long_run):
    p = (uniform[:5000] + np.float32(3)).astype(np.float32)
    default = gpu_ctx.get_option(D.DLG_OPT_VOXEL_LONG_RUN)
    try:
        if long_run is not None:
            gpu_ctx.set_option(D.DLG_OPT_VOXEL_LONG_RUN, long_run)
        ref = check_equal(gpu_ctx, p, 100.0)
    finally:
        gpu_ctx.set_option(D.DLG_OPT_VOXEL_LONG_RUN, default)
    assert list(ref["counts"]) == [5000]


def test_cloud_straddling_zero_gives_eight_voxels(gpu_ctx, uniform):
    """floorf of a negative coordinate is -1: a cloud around the origin spans 2 cells per axis"""
    ref = check_equal(gpu_ctx, uniform[:5000], 100.0)
    assert len(ref["xyz"]) == 8 and ref["counts"].sum() == 5000


def test_negative_coordinates_and_exact_multiples(gpu_ctx, uniform):
    p = uniform[:6000].copy()
    p[::3] = (np.round(p[::3] * 4) * np.float32(0.25)).astype(np.float32)  # multiples of the leaf
    p[1::50, 0] = -0.0
    check_equal(gpu_ctx, p, 0.25)
    check_equal(gpu_ctx, (p - np.float32(7)).astype(np.float32), 0.25)


def test_anisotropic_leaf(gpu_ctx, uniform):
    check_equal(gpu_ctx, uniform[:8000], (0.5, 0.125, 2.0))


def test_nonfinite_entries_are_skipped(gpu_ctx, uniform):
    p = uniform[:7400].copy()
    vals = [np.nan, np.inf, -np.inf]
    for j, i in enumerate(range(0, len(p), 37)):
        p[i, j % 3] = vals[(j // 3) % 3]
    ref = check_equal(gpu_ctx, p, 0.25)
    assert (ref["voe"][::37] == -1).all() and ref["n_finite"] == len(p) - len(range(0, len(p), 37))


def test_all_nan_cloud_gives_no_voxels(gpu_ctx):
    p = np.full((100, 3), np.nan, np.float32)
    s, k, _, _, voe, st = raw_call(gpu_ctx, p, 1e-9)  # (before any leaf check)
    assert s == 0 and k == 0 and (voe == -1).all() and st.n_finite == 0
    s, k, _, _, _, _ = raw_call(gpu_ctx, np.zeros((0, 3), np.float32), 1.0)
    assert s == 0 and k == 0


def test_indices_shuffled_with_duplicates(gpu_ctx, uniform):
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 3000, 9000).astype(np.int32)  # every point ~3 times, any order
    ref = check_equal(gpu_ctx, uniform[:3000], 0.5, idx=idx)
    assert ref["counts"].sum() == 9000
    # a small subset of a larger cloud
    check_equal(gpu_ctx, uniform, 0.5, idx=idx[:300] * 6)
    s, _, _, _, _, _ = raw_call(gpu_ctx, uniform[:3000], 0.5, idx=np.array([0, 3000], np.int32))
    assert s == _lib.DLG_ERR_INVALID
    s, _, _, _, _, _ = raw_call(gpu_ctx, uniform[:3000], 0.5, idx=np.array([-1], np.int32))
    assert s == _lib.DLG_ERR_INVALID


def test_strides_in_and_out(gpu_ctx, uniform):
    p4 = np.concatenate([uniform[:5000], np.full((5000, 1), 9.0, np.float32)], 1)  # pcl::PointXYZ
    a = check_equal(gpu_ctx, p4, 0.25, out_stride=16)
    b = check_equal(gpu_ctx, uniform[:5000], 0.25, out_stride=12)
    assert np.array_equal(bits(a["xyz"]), bits(b["xyz"]))
    s, _, _, _, _, _ = raw_call(gpu_ctx, uniform[:100], 0.25, out_stride=20)
    assert s == _lib.DLG_ERR_INVALID


@pytest.mark.parametrize("min_points", [0, 1, 2, 5])
def test_min_points_per_voxel(gpu_ctx, uniform, min_points):
    ref = check_equal(gpu_ctx, uniform, 0.25, min_points=min_points)
    full = V.voxel_ref(uniform, 0.25)
    dropped = full["counts"][full["voe"]] < min_points
    assert (ref["voe"][dropped] == -1).all() and (ref["voe"][~dropped] >= 0).all()
    assert len(ref["xyz"]) == (full["counts"] >= min_points).sum()


def test_status_codes(gpu_ctx, uniform):
    L = _lib.load()
    for leaf in (0.0, -0.25, np.nan, np.inf, (0.25, 0.0, 0.25)):
        s, _, _, _, _, _ = raw_call(gpu_ctx, uniform[:100], leaf)
        assert s == _lib.DLG_ERR_INVALID, leaf
    s, _, _, _, _, _ = raw_call(gpu_ctx, uniform[:100], 0.25, min_points=-1)
    assert s == _lib.DLG_ERR_INVALID
    s, _, out, _, _, _ = raw_call(gpu_ctx, uniform, 1e-4)
    assert s == _lib.DLG_ERR_INVALID
    assert L.dlg_last_error(gpu_ctx.h).decode().startswith(
        "leaf size too small: voxel indices would overflow")
    with pytest.raises(V.LeafTooSmall):
        V.voxel_ref(uniform, 1e-4)
    far = np.array([[3e12, 0, 0], [3e12, 1, 1]], np.float32)
    s, _, _, _, _, _ = raw_call(gpu_ctx, far, 1.0)
    assert s == _lib.DLG_ERR_INVALID and b"int range" in L.dlg_last_error(gpu_ctx.h)
    # cap one short: the size is reported, nothing is written; then success with that size
    s, k, out, cnt, voe, _ = raw_call(gpu_ctx, uniform, 0.25, cap=4066)
    assert s == _lib.DLG_ERR_CAPACITY and k == 4067
    assert (out == -7.0).all() and (cnt == -7).all() and (voe == -7).all()
    s, k2, out, _, _, _ = raw_call(gpu_ctx, uniform, 0.25, cap=k)
    assert s == 0 and k2 == 4067
    assert np.array_equal(bits(out[:k2]), bits(V.voxel_ref(uniform, 0.25)["xyz"]))
    # nullable outputs
    s, k3, _, cnt, voe, _ = raw_call(gpu_ctx, uniform, 0.25, want_counts=False, want_voe=False)
    assert s == 0 and k3 == 4067 and (cnt == -7).all() and (voe == -7).all()


def test_several_ranks_are_refused(uniform):
    """a context of a 2-rank communicator holds a shard: DLG_ERR_INVALID, and no collective runs
    (the other rank never calls)"""
    ctxs = D.Context.loopback_group(2, 0)
    try:
        s, _, _, _, _, _ = raw_call(ctxs[0], uniform[:100], 0.25)
        assert s == _lib.DLG_ERR_INVALID
        assert b"world > 1" in _lib.load().dlg_last_error(ctxs[0].h)
        with pytest.raises(D.DialogError):
            D.voxel_grid_cloud(uniform[:100], 0.25, ctx=ctxs[1])
    finally:
        for c in ctxs:
            c.close()


def test_cpp_voxel_shim_runs_on_gpu(tmp_path):
    """tests/cpp/shim_voxel.cpp: dialog::VoxelGrid filtering a cloud into itself, then a
    setIndices + minimum-occupancy filter of the result, then PCL's leaf-too-small copy-through;
    sizes and the xor of the output bits (pad 1.0f included) equal the reference's"""
    exe = tmp_path / "shim_voxel"
    lib = os.path.dirname(D.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_voxel.cpp"), "-o", str(exe), "-L", lib,
                    "-ldialog_amd", f"-Wl,-rpath,{lib}"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "Leaf size is too small" in out.stderr
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.strip().splitlines()}

    def xor(xyz):
        b = np.concatenate([bits(xyz), np.full((len(xyz), 1), np.float32(1)).view(np.uint32)], 1)
        m = np.array([1, 3, 5, 7], np.uint32)
        return int(np.bitwise_xor.reduce((b * m).reshape(-1))) if len(xyz) else 0

    i = np.arange(4000)
    p = np.stack([np.float32(0.001) * (i % 100).astype(np.float32),
                  np.float32(0.002) * (i // 100).astype(np.float32),
                  np.float32(0.0005) * (i % 7).astype(np.float32)], 1).astype(np.float32)
    a = V.voxel_ref(p, 0.01)
    assert lines["first"] == ["4000", str(len(a["xyz"])), str(a["n_voxels"]),
                              "%08x" % xor(a["xyz"])]
    idx = np.arange(0, len(a["xyz"]), 2)
    b = V.voxel_ref(a["xyz"], 0.05, idx=idx, min_points=2)
    assert lines["second"] == [str(len(idx)), str(len(b["xyz"])), "2", "%08x" % xor(b["xyz"])]
    assert lines["empty"] == ["0"]
    assert lines["tiny"] == [str(len(a["xyz"]))]


# ---- the device-resident result ----------------------------------------------------------------
THRESHOLD = 0.02
LEAF = 0.04  # (leaf 0.05 gives 121,439 voxels on this cloud, short of the rule; 0.04: 143,626)


@pytest.fixture(scope="module")
def voxel_clouds(gpu_ctx):
    """a 200,000-point cloud filtered both ways: to the host and re-uploaded, and left on the
    device.  The voxel cloud reaches the 131,072-point spatial-copy rule."""
    p, _, _ = plane_cloud(200000, 3, seed=77)
    xyz, counts, voe = D.voxel_grid(p, LEAF, ctx=gpu_ctx)
    assert len(xyz) >= 131072, len(xyz)
    up = D.Cloud(gpu_ctx, xyz, id_base=1000)
    dev, voe_d = D.voxel_grid_cloud(p, LEAF, id_base=1000, ctx=gpu_ctx)
    yield p, xyz, counts, voe, up, dev, voe_d
    up.close()
    dev.close()


def test_voxel_cloud_equals_upload_of_the_host_result(voxel_clouds):
    p, xyz, counts, voe, up, dev, voe_d = voxel_clouds
    assert dev.n == up.n == len(xyz) and dev.n_active == up.n_active
    assert np.array_equal(voe, voe_d)
    assert dev.signature() == up.signature()
    # (the host result itself, on a prefix the numpy chains finish quickly)
    ref = V.voxel_ref(p[:30000], LEAF)
    x2, c2, v2 = D.voxel_grid(p[:30000], LEAF, ctx=up.ctx)
    assert np.array_equal(bits(x2), bits(ref["xyz"])) and np.array_equal(v2, ref["voe"])


def test_voxel_cloud_planes_and_normals_equal(voxel_clouds):
    p, xyz, counts, voe, up, dev, _ = voxel_clouds
    prm = D.make_params(THRESHOLD, max_iterations=200, probability=0.99)
    ra = D.extract_planes(up, prm, max_planes=3)
    rb = D.extract_planes(dev, prm, max_planes=3)
    assert ra["n_planes"] == rb["n_planes"] == 3
    assert np.array_equal(bits(ra["coeffs"]), bits(rb["coeffs"]))
    assert np.array_equal(ra["offsets"], rb["offsets"])
    assert np.array_equal(ra["inliers"], rb["inliers"])
    assert ra["stats"]["lean_rounds"] == rb["stats"]["lean_rounds"]  # (same spatial-copy path)
    na = up.estimate_normals(k=20, copy_out=True)
    nb = dev.estimate_normals(k=20, copy_out=True)
    assert np.array_equal(bits(na), bits(nb))
    # voxel_of_entry maps a plane found on the voxel cloud back to the original points: every
    # member of an inlier voxel lies within the voxel's diagonal of its centroid
    assert (voe >= 0).all()  # (a finite cloud, min_points 0: every point went into a voxel)
    bound = THRESHOLD + LEAF * np.sqrt(3.0)
    for k in range(3):
        co = rb["coeffs"][k].astype(np.float64)
        rows = rb["inliers"][rb["offsets"][k]:rb["offsets"][k + 1]] - 1000  # ids -> rows
        assert rows.min() >= 0 and rows.max() < len(xyz)
        is_inlier_row = np.zeros(len(xyz), bool)
        is_inlier_row[rows] = True
        orig = np.flatnonzero(is_inlier_row[voe])  # the original points of every inlier row
        assert len(orig) == counts[rows].sum() >= len(rows)
        d = np.abs(p[orig].astype(np.float64) @ co[:3] + co[3]) / np.linalg.norm(co[:3])
        assert d.max() <= bound, (k, d.max())
