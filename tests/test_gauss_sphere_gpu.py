"""GPU: the Gaussian-sphere plane seeds (dlg_gs_vote, dlg_gs_segment, dlg_cloud_gs_segment) equal to
the numpy restatement (tests/gsphere_ref.py) on the cases of tests/gsphere_cases.py: the cell of
every point, raw and filtered votes, sink_init and sink of every cell, the sink list, the planes'
offsets and ids.  tests/test_gauss_sphere.py asserts on the CPU that every cell of every case is
stable, so no cell is excluded here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gsphere_cases as K
import dialog_amd as D
from dialog_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = tuple(K.cases())


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    yield c
    c.close()


def check_equal(got, ref):
    for k in ("cell_of_point", "raw_vote", "filtered_vote", "sink_init", "sink", "sink_cells",
              "sink_votes", "plane_offsets", "plane_ids"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["n_cells"] == len(ref["P"])


@pytest.mark.parametrize("name", NAMES)
def test_segment_equals_the_restatement(ctx, name):
    pts, nrm, prm = K.cases()[name]
    ref = K.reference(name)
    got = D.gauss_sphere_segment(pts, nrm, prm, ctx=ctx, debug=True, return_stats=True)
    check_equal(got, ref)
    st = got["stats"]
    assert st["n_cells"] == len(ref["P"])
    assert st["n_occupied"] == np.count_nonzero(ref["raw_vote"])
    assert st["n_voters"] == ref["raw_vote"].sum() == np.count_nonzero(ref["cell_of_point"] >= 0)
    assert st["n_sinks"] == len(ref["sink_cells"])
    assert st["n_planes"] == len(ref["plane_offsets"]) - 1
    assert st["n_plane_points"] == len(ref["plane_ids"])
    if name == "non_unit":
        assert st["n_fallback_votes"] > 0
    if name in ("box_corner", "negative"):
        assert st["n_fallback_votes"] == 0
    if name == "coplanar_gap":  # one sink, two planes, in order; then the second sink's
        assert len(got["sink_cells"]) == 2 and len(got["plane_offsets"]) == 4
        a, b, _ = D.gauss_sphere.planes_of(got)
        assert a.max() < 700 <= b.min() and b.max() < 1200 and a[0] == 0
    if name == "non_finite":
        bad = ~np.isfinite(nrm).all(1)
        assert (got["cell_of_point"][bad] == -1).all()
        assert not np.isin(np.nonzero(bad)[0], got["plane_ids"]).any()


@pytest.mark.parametrize("name", ["noisy", "non_unit", "non_finite"])
def test_vote_alone(ctx, name):
    _, nrm, prm = K.cases()[name]
    ref = K.reference(name)
    wide = np.zeros((len(nrm), 5), f32)  # (a stride of 20 bytes)
    wide[:, :3] = nrm
    cell, votes, st = D.gauss_sphere_vote(wide, prm, ctx=ctx, return_stats=True)
    assert np.array_equal(cell, ref["cell_of_point"])
    assert np.array_equal(votes, ref["raw_vote"])
    assert st["n_occupied"] == np.count_nonzero(ref["raw_vote"])
    assert (st["n_fallback_votes"] > 0) or name != "non_unit"


def test_empty_and_all_non_finite(ctx):
    prm = dict(K.BASE)
    got = D.gauss_sphere_segment(np.zeros((0, 3), f32), np.zeros((0, 3), f32), prm, ctx=ctx,
                                 debug=True)
    assert list(got["plane_offsets"]) == [0] and got["plane_ids"].size == 0
    assert got["sink_cells"].size == 0 and not got["raw_vote"].any()
    assert not got["filtered_vote"].any() and (got["sink"] == -1).all()
    pts, _ = K.box_corner(n=100)
    nrm = np.full(pts.shape, np.nan, f32)
    nrm[::2] = np.inf
    got = D.gauss_sphere_segment(pts, nrm, prm, ctx=ctx, debug=True)
    assert (got["cell_of_point"] == -1).all() and not got["raw_vote"].any()
    assert list(got["plane_offsets"]) == [0] and got["sink_cells"].size == 0
    cell, votes = D.gauss_sphere_vote(np.zeros((0, 3), f32), prm, ctx=ctx)
    assert cell.size == 0 and not votes.any()


def test_cloud_call_equals_the_host_call(ctx):
    """dlg_cloud_gs_segment over the device copy and the estimated normals = dlg_gs_segment over
    the same points and the normals read back"""
    pts, _, prm = K.cases()["box_corner"]
    cloud = D.Cloud(ctx, pts)
    nrm = cloud.estimate_normals(k=12, copy_out=True)
    a = D.cloud_gauss_sphere_segment(cloud, prm, debug=True)
    b = D.gauss_sphere_segment(pts, nrm[:, :3], prm, ctx=ctx, debug=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert len(a["plane_offsets"]) - 1 >= 1 and a["plane_ids"].size > 1000
    bare = D.Cloud(ctx, pts)
    with pytest.raises(D.DialogError):
        D.cloud_gauss_sphere_segment(bare, prm)
    bare.close()
    cloud.close()


def test_capacity_errors_report_sizes(ctx):
    pts, nrm, prm = K.cases()["coplanar_gap"]
    ref = K.reference("coplanar_gap")
    L = _lib.load()
    n = len(pts)
    a, P = D.sac._points(pts)
    nr = np.ascontiguousarray(nrm, f32)
    p = D.gauss_sphere_params(**prm)
    i32p, i64p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)

    def run(planes_cap, ids_cap, sinks_cap):
        off = np.full(n + 1, -7, np.int64)
        ids = np.full(n, -7, np.int32)
        sc = np.full(8, -7, np.int32)
        sv = np.full(8, -7, np.int64)
        r = _lib.GsResult()
        r.plane_offsets, r.planes_cap = off.ctypes.data_as(i64p), planes_cap
        r.plane_ids, r.ids_cap = ids.ctypes.data_as(i32p), ids_cap
        r.sink_cells, r.sink_votes = sc.ctypes.data_as(i32p), sv.ctypes.data_as(i64p)
        r.sinks_cap = sinks_cap
        s = L.dlg_gs_segment(ctx.h, C.byref(P), nr.ctypes.data_as(fp), 12, C.byref(p),
                             C.byref(r), None)
        return s, r, off, ids, sc

    n_pl, n_ids = len(ref["plane_offsets"]) - 1, len(ref["plane_ids"])
    for caps in ((n_pl - 1, n, 8), (n, n_ids - 1, 8), (n, n, 1)):
        s, r, off, ids, sc = run(*caps)
        assert s == _lib.DLG_ERR_CAPACITY
        assert (r.n_planes, r.n_ids, r.n_sinks) == (n_pl, n_ids, 2)
        assert (ids == -7).all() and (off == -7).all()
        assert b"need" in L.dlg_last_error(ctx.h)
    s, r, off, ids, sc = run(n_pl, n_ids, 2)
    assert s == _lib.DLG_OK
    assert np.array_equal(off[:n_pl + 1], ref["plane_offsets"])
    assert np.array_equal(ids[:n_ids], ref["plane_ids"])
    bad = D.gauss_sphere_params(**dict(prm, delta_radius=0.0))
    r = _lib.GsResult()
    off = np.zeros(2, np.int64)
    r.plane_offsets = off.ctypes.data_as(i64p)
    assert L.dlg_gs_segment(ctx.h, C.byref(P), nr.ctypes.data_as(fp), 12, C.byref(bad),
                            C.byref(r), None) == _lib.DLG_ERR_INVALID


def test_several_ranks_are_refused():
    """a context of a 2-rank communicator holds a shard: DLG_ERR_INVALID, as FPFH and ICP answer"""
    pts, nrm, prm = K.cases()["size_equal_T"]
    ctxs = D.Context.loopback_group(2, 0)
    try:
        with pytest.raises(D.DialogError) as ei:
            D.gauss_sphere_segment(pts, nrm, prm, ctx=ctxs[0])
        assert ei.value.status == _lib.DLG_ERR_INVALID and "world > 1" in str(ei.value)
        with pytest.raises(D.DialogError) as ei:
            D.gauss_sphere_vote(nrm, prm, ctx=ctxs[1])
        assert ei.value.status == _lib.DLG_ERR_INVALID and "world > 1" in str(ei.value)
    finally:
        for c in ctxs:
            c.close()


def test_cpp_shim(ctx, tmp_path):
    """dialog::segmentPlanesGaussSphere fills the reference's std::vector<Plane>"""
    src = os.path.join(ROOT, "tests", "cpp", "shim_gauss_sphere.cpp")
    exe = tmp_path / "shim_gauss_sphere"
    lib = os.path.dirname(_lib.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o",
                        str(exe), "-L", lib, "-ldialog_amd", f"-Wl,-rpath,{lib}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
