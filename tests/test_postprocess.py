"""postProcessPlanes (Dialog/PlaneDetect.h:1454-1579): refit, leftover absorption by the border
polygons (isPointInPoly, :1891-1964), clusterFilt (:1582-1655).

The oracle (oracle/pcl_oracle.c, orc_post_process_planes & co.) restates the reference's float
arithmetic literally; the reference has no tests or fixtures for this stage, so the oracle is
pinned here by (a) the MSVC rand() known answers, (b) agreement of its 10-ray majority vote with
an exact even-odd containment test away from the border, and (c) agreement of its BFS clusters
with scipy's connected components.  The GPU path must match the oracle bit for bit.

The scenes here are synth.postprocess_scene's stars.  The edges are elsewhere: the early outs of
the crossing test on the host in tests/test_pp_math.py; the device's ray parities, the task
split, the 1-NN ties and clusterFilt's thresholds in tests/test_postprocess_edges_gpu.py, on the
scenes of tests/pp_cases.py, which tests/test_postprocess_edges.py checks on the CPU.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O


def star_scene(n=20000, planes=4, seed=None, n_border=40, keep=0.7):
    from dialog_amd.synth import SEED_BASE, postprocess_scene
    return postprocess_scene(n, planes, keep_frac=keep, n_border=n_border,
                             seed=SEED_BASE + 6 if seed is None else seed)


def oracle_run(cloud, planes, t_dist=0.1, start=0, seed=12345, radius=0.5, tnum=20):
    co = np.array([np.r_[np.asarray(p["coeff"], np.float32)[:3], 0.0] for p in planes],
                  np.float32).reshape(-1, 4)
    return O.post_process_planes(cloud, co, [p["points"] for p in planes],
                                 [p["border"] for p in planes], t_dist, start, seed, radius, tnum)


def even_odd_inside(q2, poly2):
    """exact 2-D crossing-number containment (numpy, float64)"""
    x, y = q2[:, 0:1], q2[:, 1:2]
    a, b = poly2, np.roll(poly2, -1, axis=0)
    cond = (a[:, 1] > y) != (b[:, 1] > y)
    xi = a[:, 0] + (y - a[:, 1]) * (b[:, 0] - a[:, 0]) / np.where(b[:, 1] != a[:, 1],
                                                                   b[:, 1] - a[:, 1], 1.0)
    return (np.sum(cond & (x < xi), axis=1) % 2) == 1


def seg_dist2d(q2, poly2):
    a, b = poly2, np.roll(poly2, -1, axis=0)
    ab = b - a
    t = np.clip(((q2[:, None, :] - a) * ab).sum(-1) / (ab * ab).sum(-1), 0, 1)
    d = q2[:, None, :] - (a + t[..., None] * ab)
    return np.sqrt((d * d).sum(-1)).min(axis=1)


# ---------------------------------------------------------------------------------------------
# oracle pinning (CPU)

def test_msvc_rand_kat():
    # MSVC CRT rand() after srand(1) (also the sequence without srand) and after srand(0)
    assert O.msvc_rand(5, 1) == [41, 18467, 6334, 26500, 19169]
    assert O.msvc_rand(1, 0) == [38]


def test_oracle_point_in_poly_matches_containment():
    rng = np.random.default_rng(3)
    cloud, planes = star_scene(4000, 2, n_border=30)
    for pl in planes:
        nrm = np.asarray(pl["coeff"], np.float64)
        b = pl["border"].astype(np.float64)
        c0 = b.mean(axis=0)
        u = (b[0] - c0) / np.linalg.norm(b[0] - c0)
        v = np.cross(nrm, u)
        st = rng.uniform(-5.5, 5.5, size=(400, 2))
        q = (c0 + st[:, :1] * u + st[:, 1:] * v + rng.normal(0, 0.01, (400, 1)) * nrm)
        q = q.astype(np.float32)
        d = -float(np.dot(nrm, c0))
        coeff = np.r_[nrm, d].astype(np.float32)
        b2 = np.c_[(b - c0) @ u, (b - c0) @ v]
        q2 = np.c_[(q - c0) @ u, (q - c0) @ v]
        inside = even_odd_inside(q2, b2)
        far = seg_dist2d(q2, b2) > 0.01
        got = np.array([O.is_point_in_poly(x, coeff, pl["border"], 0.1, 777) for x in q])
        assert np.array_equal(got[far], inside[far])
        # the distance gate
        off = q + 0.2 * nrm.astype(np.float32)
        assert not any(O.is_point_in_poly(x, coeff, pl["border"], 0.1, 777) for x in off[:50])


def test_oracle_cluster_filter_matches_components():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(5)
    centers = rng.uniform(-10, 10, size=(40, 3))
    sizes = rng.integers(1, 60, size=40)
    p = np.concatenate([c + rng.normal(0, 0.15, size=(s, 3)) for c, s in zip(centers, sizes)])
    p = np.concatenate([p, rng.uniform(-10, 10, size=(300, 3))]).astype(np.float32)
    r, T = 0.3, 12
    pairs = cKDTree(p.astype(np.float64)).query_pairs(r * 1.001, output_type="ndarray")
    d = p[pairs[:, 0]] - p[pairs[:, 1]]
    d2 = ((np.float32(0) + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    pairs = pairs[d2 < np.float32(r * r)]
    g = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(len(p), len(p)))
    _, lab = connected_components(g, directed=False)
    want = np.bincount(lab)[lab] > T
    assert np.array_equal(O.cluster_filter(p, r, T), want)
    # size_t comparison: a negative T_cluster_num drops every cluster
    assert not O.cluster_filter(p, r, -1).any()


def test_oracle_post_process_consistency():
    cloud, planes = star_scene()
    co, ab, rem = oracle_run(cloud, planes)
    n = cloud.shape[0]
    taken = np.zeros(n, bool)
    for pl in planes:  # plane points are cloud points: their 1-NN is themselves
        d = np.abs(cloud[:, None, :] - pl["points"][None, :50, :]).sum(-1)
        assert (d.min(axis=0) == 0).all()
    for a in ab:
        assert np.all(np.diff(a) > 0) and a.size > 100
        taken[a] = True
    assert not taken[rem].any() and np.all(np.diff(rem) > 0)
    for k, pl in enumerate(planes):  # refit normal keeps the given orientation
        assert np.dot(co[k, :3], pl["coeff"][:3]) > 0.99


def test_refit_planes_host_bit_exact():
    """dlg_refit_planes is host arithmetic (no device): compared with the oracle here."""
    import dialog_amd as D
    cloud, planes = star_scene(8000, 3)
    planes = planes + [dict(coeff=[0, 0, 1, 0], points=cloud[:2], border=cloud[:3]),
                       dict(coeff=[0, 0, -1], points=cloud[100:2100], border=cloud[:3])]
    got = D.refit_planes(planes)
    co = np.array([np.r_[np.asarray(p["coeff"], np.float32)[:3], 0] for p in planes], np.float32)
    want = O.refit_planes(co, [p["points"] for p in planes])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(got[3]).all()


# ---------------------------------------------------------------------------------------------
# GPU parity

def gpu_run(ctx, cloud, planes, t_dist=0.1, start=0, seed=12345, radius=0.5, tnum=20):
    import dialog_amd as D
    prm = D.PostProcessParams(t_dist, radius, tnum, start, seed)
    return D.post_process_planes(cloud, planes, prm, ctx=ctx)


def assert_same(g, o):
    gco, gab, grem = g
    oco, oab, orem = o
    assert np.array_equal(gco.view(np.uint32), oco.view(np.uint32))
    assert len(gab) == len(oab)
    for a, b in zip(gab, oab):
        assert np.array_equal(a, b)
    assert np.array_equal(grem, orem)


@pytest.mark.gpu
@pytest.mark.parametrize("seed_scene,start,seed,radius,tnum,nb", [
    (None, 0, 12345, 0.5, 20, 40),
    (11, 0, 1, 0.3, 5, 17),
    (12, 2, 1700000000, 0.8, 100, 64),
    (13, 0, 0, 0.0, 0, 9),
])
def test_gpu_post_process_bit_exact(gpu_ctx, seed_scene, start, seed, radius, tnum, nb):
    cloud, planes = star_scene(20000, 4, seed=seed_scene, n_border=nb)
    g = gpu_run(gpu_ctx, cloud, planes, start=start, seed=seed, radius=radius, tnum=tnum)
    o = oracle_run(cloud, planes, start=start, seed=seed, radius=radius, tnum=tnum)
    assert_same(g, o)
    assert sum(a.size for a in g[1][start:]) > 0


@pytest.mark.gpu
def test_gpu_post_process_edges(gpu_ctx):
    import dialog_amd as D
    cloud, planes = star_scene(6000, 3, seed=21)
    # a plane with < 3 points refits to NaN and absorbs nothing; pcl::PointXYZ records
    planes2 = planes + [dict(coeff=[1, 0, 0], points=cloud[:2], border=planes[0]["border"])]
    c4 = np.c_[cloud, np.ones(len(cloud), np.float32)]
    g = gpu_run(gpu_ctx, c4, planes2)
    assert_same(g, oracle_run(cloud, planes2))
    assert np.isnan(g[0][3]).all() and g[1][3].size == 0
    # plane_start beyond the list: no absorption, clusterFilt only
    g = gpu_run(gpu_ctx, cloud, planes, start=3)
    assert all(a.size == 0 for a in g[1])
    assert_same(g, oracle_run(cloud, planes, start=3))
    # no planes at all
    g = gpu_run(gpu_ctx, cloud, [])
    assert_same(g, oracle_run(cloud, []))
    # empty cloud
    g = gpu_run(gpu_ctx, np.zeros((0, 3), np.float32), planes)
    assert all(a.size == 0 for a in g[1]) and g[2].size == 0
    # a participating plane without border is refused
    bad = planes + [dict(coeff=[1, 0, 0], points=cloud[:10], border=np.zeros((0, 3), np.float32))]
    with pytest.raises(D.DialogError):
        gpu_run(gpu_ctx, cloud, bad)
    # capacity: report the sizes, DLG_ERR_CAPACITY
    from dialog_amd import _lib
    from dialog_amd.postprocess import _PlaneArrays
    from dialog_amd.sac import _points
    A = _PlaneArrays(planes)
    a, pts = _points(cloud)
    prm = _lib.PostProcessParams(0.1, 0.5, 20, 0, 12345)
    co = np.zeros((3, 4), np.float32)
    off = np.zeros(4, np.int64)
    ids = np.zeros(1, np.int32)
    rem = np.zeros(1, np.int32)
    nrem = C.c_int64(0)
    st = _lib.load().dlg_post_process_planes(
        gpu_ctx.h, C.byref(pts), C.byref(A.s), C.byref(prm),
        co.ctypes.data_as(C.POINTER(C.c_float)), off.ctypes.data_as(C.POINTER(C.c_int64)),
        ids.ctypes.data_as(C.POINTER(C.c_int32)), 1, rem.ctypes.data_as(C.POINTER(C.c_int32)),
        1, C.byref(nrem))
    assert st == _lib.DLG_ERR_CAPACITY
    o = oracle_run(cloud, planes)
    assert off[-1] == sum(x.size for x in o[1]) and nrem.value == o[2].size


@pytest.mark.gpu
def test_gpu_post_process_nearest_fallback(gpu_ctx):
    """plane points that are not cloud points (nudged copies, points with a zero coordinate, a
    point far away): their nearest cloud point comes from the grid search, not the exact table"""
    cloud, planes = star_scene(12000, 3, seed=41)
    rng = np.random.default_rng(2)
    for pl in planes:
        p = pl["points"].copy()
        sel = rng.random(len(p)) < 0.5
        p[sel] = np.nextafter(p[sel], np.float32(np.inf))
        p[:3, 0] = 0.0
        p[3] = [50.0, -50.0, 50.0]
        pl["points"] = p
    g = gpu_run(gpu_ctx, cloud, planes)
    assert_same(g, oracle_run(cloud, planes))


@pytest.mark.gpu
@pytest.mark.parametrize("n,r,T", [(5000, 0.3, 10), (30000, 0.2, 3), (2000, 0.0, 0)])
def test_gpu_cluster_filter_bit_exact(gpu_ctx, n, r, T):
    import dialog_amd as D
    rng = np.random.default_rng(n)
    centers = rng.uniform(-10, 10, size=(60, 3))
    p = np.concatenate([c + rng.normal(0, 0.2, size=(n // 120, 3)) for c in centers])
    p = np.concatenate([p, rng.uniform(-10, 10, size=(n - len(p), 3))]).astype(np.float32)
    got = D.cluster_filter(p, r, T, ctx=gpu_ctx)
    want = np.nonzero(O.cluster_filter(p, r, T))[0]
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.slow
def test_gpu_post_process_large_properties(gpu_ctx):
    """1M points, 20 planes, 200-vertex borders: refit bit-exact against the oracle; absorption
    of a random sample of leftover points re-decided by the oracle's isPointInPoly; clusterFilt of
    the leftovers against the oracle's BFS."""
    import dialog_amd as D
    cloud, planes = star_scene(1_000_000, 20, seed=31, n_border=200)
    seed = 4242
    co, ab, rem = gpu_run(gpu_ctx, cloud, planes, seed=seed, radius=0.1, tnum=5)
    co_in = np.array([np.r_[p["coeff"][:3], 0] for p in planes], np.float32)
    want = O.refit_planes(co_in, [p["points"] for p in planes])
    assert np.array_equal(co.view(np.uint32), want.view(np.uint32))
    n = cloud.shape[0]
    proc = np.zeros(n, bool)
    # plane points are cloud points (1-NN = themselves)
    lut = {tuple(x): i for i, x in enumerate(map(tuple, cloud))}
    for p in planes:
        proc[[lut[tuple(x)] for x in map(tuple, p["points"])]] = True
    member = np.zeros((len(planes), n), bool)
    for k, a in enumerate(ab):
        assert np.all(np.diff(a) > 0)
        member[k, a] = True
    assert not (member.any(axis=0) & proc).any()
    rng = np.random.default_rng(7)
    cand = np.nonzero(~proc)[0]
    for i in rng.choice(cand, size=300, replace=False):
        for k, p in enumerate(planes):
            assert O.is_point_in_poly(cloud[i], co[k], p["border"], 0.1, seed) == member[k, i]
    rest = np.nonzero(~proc & ~member.any(axis=0))[0]
    keep = O.cluster_filter(cloud[rest], 0.1, 5)
    assert np.array_equal(rem, rest[keep])
