"""GPU: postProcessPlanes' point-in-polygon kernels and clusterFilt at their edges, bit for bit
against the oracle.

* the ten ray parities of every candidate (dlg_debug_pip_masks, the vote out of the way) against
  orc_pip_parities on the scenes of tests/pp_cases.py: axis-aligned and rotated borders with
  collinear, duplicate and near-duplicate vertices, points on edges and vertices, borders 4000
  long, far from the origin, off their plane, of 1, 2, 3, 16, 17 and 1000 vertices;
* the full entry against orc_post_process_planes where the task split, the compact plane index,
  the candidate blocks and the 1-NN marking take their other paths;
* clusterFilt against orc_cluster_filter on chains, components at the size threshold, pairs at the
  radius, duplicates, sizes around a wave and a workgroup.

tests/test_postprocess_edges.py asserts (CPU) that each scene reaches its case.
"""
import ctypes as C

import numpy as np
import pytest

import pp_cases as PC
from oracle import oracle as O
from test_postprocess import assert_same, gpu_run, oracle_run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(PC.MASK_SCENES))
def test_gpu_ray_parities_bit_exact(gpu_ctx, name):
    import dialog_amd as D
    s = PC.mask_scene(name)
    want = PC.oracle_masks(name)
    got = D.debug_pip_masks(s["cloud"], s["planes"], s["t_dist"], s["seed"], ctx=gpu_ctx)
    assert len(got) == len(want)
    for k, ((gi, gm), (wi, wm)) in enumerate(zip(got, want)):
        assert np.array_equal(gi, wi), (name, k)
        bad = np.nonzero(gm != wm)[0]
        assert bad.size == 0, (name, k, bad.size, [(int(wi[j]), s["cloud"][wi[j]].tolist(),
                                                    bin(int(gm[j])), bin(int(wm[j])))
                                                   for j in bad[:5]])


def test_gpu_ray_parities_entry(gpu_ctx):
    """the debug entry itself: a non-finite plane has an empty range (and the planes after it
    keep theirs), t_dist gates the candidates, an empty border is refused, capacity is reported"""
    import dialog_amd as D
    from dialog_amd import _lib
    from dialog_amd.postprocess import _PlaneArrays
    from dialog_amd.sac import _points
    s = PC.mask_scene("short_edges")
    want = PC.oracle_masks("short_edges")
    nan = dict(coeff=np.array([0, np.nan, 1, 0], np.float32), border=s["planes"][0]["border"])
    inf = dict(coeff=np.array([0, 0, 1, np.inf], np.float32), border=s["planes"][0]["border"])
    planes = [s["planes"][0], nan, s["planes"][1], inf]
    got = D.debug_pip_masks(s["cloud"], planes, s["t_dist"], s["seed"], ctx=gpu_ctx)
    assert got[1][0].size == 0 and got[3][0].size == 0
    for g, w in ((got[0], want[0]), (got[2], want[1])):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])
    # a gate that cuts the noisy copy of the cloud
    cand, m = O.pip_parities(s["cloud"], planes[2]["coeff"], planes[2]["border"], 0.002, 7)
    ids = np.nonzero(cand)[0]
    assert 100 < ids.size < len(s["cloud"]) - 100
    gi, gm = D.debug_pip_masks(s["cloud"], planes[2:3], 0.002, 7, ctx=gpu_ctx)[0]
    assert np.array_equal(gi, ids) and np.array_equal(gm, m[ids])
    assert D.debug_pip_masks(np.zeros((0, 3), np.float32), planes, 0.1, 7, ctx=gpu_ctx)[0][0].size == 0
    with pytest.raises(D.DialogError):
        D.debug_pip_masks(s["cloud"], [dict(coeff=[0, 0, 1, 0], border=np.zeros((0, 3), np.float32))],
                          0.1, 7, ctx=gpu_ctx)
    # capacity: DLG_ERR_CAPACITY and the size needed
    A = _PlaneArrays([dict(coeff=p["coeff"], points=(), border=p["border"]) for p in planes])
    a, pts = _points(s["cloud"])
    off = np.zeros(5, np.int64)
    ids1 = np.full(1, -7, np.int32)
    m1 = np.zeros(1, np.uint32)
    need = C.c_int64(0)
    st = _lib.load().dlg_debug_pip_masks(
        gpu_ctx.h, C.byref(pts), C.byref(A.s), 0.1, 12345, off.ctypes.data_as(C.POINTER(C.c_int64)),
        ids1.ctypes.data_as(C.POINTER(C.c_int32)), m1.ctypes.data_as(C.POINTER(C.c_uint32)), 1,
        C.byref(need))
    assert st == _lib.DLG_ERR_CAPACITY
    assert need.value == off[-1] == want[0][0].size + want[1][0].size and ids1[0] == -7
    assert off.tolist() == [0, want[0][0].size, want[0][0].size, need.value, need.value]


# ---- the full entry ------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [2100, 1100])
def test_gpu_identical_planes(gpu_ctx, count):
    """one candidate block per plane: split 1 (one task per border) and split 2 (chunks of 20
    edges); more than 64 absorbing planes"""
    cloud, planes = PC.identical_planes(count)
    g = gpu_run(gpu_ctx, cloud, planes, radius=0.5, tnum=0)
    o = oracle_run(cloud, planes, radius=0.5, tnum=0)
    assert_same(g, o)
    assert all(np.array_equal(a, g[1][0]) for a in g[1]) and g[1][0].size > 0


@pytest.mark.parametrize("start", [0, 1])
def test_gpu_nan_plane_in_the_middle(gpu_ctx, start):
    cloud, planes = PC.nan_middle()
    g = gpu_run(gpu_ctx, cloud, planes, start=start)
    assert_same(g, oracle_run(cloud, planes, start=start))
    assert np.isnan(g[0][1]).all() and g[1][1].size == 0 and g[1][3].size > 0


@pytest.mark.parametrize("k", [1, 256, 257])
def test_gpu_exact_candidate_counts(gpu_ctx, k):
    cloud, planes = PC.exact_candidates(k)
    assert_same(gpu_run(gpu_ctx, cloud, planes), oracle_run(cloud, planes))


def test_gpu_overlapping_planes(gpu_ctx):
    cloud, planes = PC.overlapping()
    g = gpu_run(gpu_ctx, cloud, planes)
    assert_same(g, oracle_run(cloud, planes))
    assert np.intersect1d(g[1][0], g[1][1]).size > 50


def test_gpu_degenerate_clouds(gpu_ctx):
    for cloud, planes, tnum in [(*PC.one_spot(50), 0), (*PC.one_spot(50, inside=False), 48),
                                (*PC.one_spot(50, inside=False), 49), (*PC.one_spot(1), 0),
                                (PC.one_spot(1)[0], [], 0)]:
        assert_same(gpu_run(gpu_ctx, cloud, planes, tnum=tnum),
                    oracle_run(cloud, planes, tnum=tnum))


def test_gpu_nearest_marking_ties(gpu_ctx):
    cloud, planes, _ = PC.nn_ties()
    assert_same(gpu_run(gpu_ctx, cloud, planes, tnum=0), oracle_run(cloud, planes, tnum=0))


# ---- clusterFilt ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PC.cluster_cases()))
def test_gpu_cluster_filter_edges(gpu_ctx, name):
    import dialog_amd as D
    p, r, T, kept = PC.cluster_cases()[name]
    got = D.cluster_filter(p, r, T, ctx=gpu_ctx)
    want = np.nonzero(O.cluster_filter(p, r, T))[0]
    assert np.array_equal(got, want)
    assert got.size == kept
