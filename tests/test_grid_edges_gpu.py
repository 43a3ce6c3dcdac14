"""GPU: every search that goes through the uniform grid (make_grid / cell_of / the k-NN bound,
dialog_amd/csrc/grid_model.hpp) on clouds that drive the grid to wide, thin shapes, against plain
references.  All comparisons are exact.

The inputs are tests/golden/grid_edges.npz (tests/golden/make_grid_edges.py): a z = 0 sheet and a
line whose radius grids have 30,000 and 2^21 requested cells per axis, with pairs aimed at the cell
faces; a box whose grid has to grow to fit the key space; a cloud whose cells are chosen by their
hash so that the cell table's probe wraps; and two k-NN clouds of 2^17 points (collinear, and a thin
strip) whose level-0 grids are some 18,000 to 37,000 cells wide.  tests/test_grid_model.py asserts
that these clouds break the arithmetic that shrank inv_cell by 1e-3 and allowed 1e-4 of a cell at
every width: there 546 of the sheet's and 2,082 of the line's pairs within r lie two cells apart,
and 24 queries of the collinear k-NN cloud are placed so that the outlier filter's K-th distance
falls between a neighbour's distance and the violated bound of that neighbour's cell.

What a build with those fixed allowances gave on an MI355X: 1,092 of 19,802 (sheet) and 4,164 of
19,502 (line) MLS neighbour counts wrong, 257 and 274 radius-normal rows wrong on either path, the
BFS stopped after 1 of 12 (sheet) and 1 of 3 (line) points, and the 24 aimed distances of the
outlier filter wrong.  The grown grid, the table's wrap, the k-NN normals and the registration's
correspondences equalled their references there too: those tests characterise.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

import dialog_amd as D
import icp_ref as R
import mls_ref as M
import sor_ref as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location(
        "make_grid_edges", os.path.join(ROOT, "tests", "golden", "make_grid_edges.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "grid_edges.npz"))
    return z, json.loads(str(z["meta"]))


def assert_same_floats(got, want):
    """bit for bit, a NaN matching any NaN"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), int((np.isnan(got) != np.isnan(want)).sum())
    ok = ~np.isnan(want)
    bad = (bits(got) != bits(want)) & ok
    assert not bad.any(), int(bad.any(axis=-1).sum())


# ---- the radius searches: the sheet, the line, the grown grid --------------------------------------
@pytest.mark.parametrize("name", ["sheet", "line", "grown"])
def test_mls_neighbour_counts_and_stats(gpu_ctx, golden, name):
    z, meta = golden
    m = meta[name]
    xyz, nrm, src, nb, st = D.moving_least_squares(z[name + "/points"], m["radius"], ctx=gpu_ctx,
                                                   return_stats=True)
    wrong = int((nb != z[name + "/nb"]).sum())
    print(f"{name}: {wrong} of {len(nb)} neighbour counts differ")
    assert wrong == 0
    assert np.array_equal(src, z[name + "/src"])
    assert {q: st[q] for q in M.STAT_KEYS} == m["stats"]


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", ["sheet", "line", "grown"])
def test_radius_normals_bit_exact(golden, name, fused):
    """PCL-float radius normals against the oracle's, by the fused pass and the chunked pipeline"""
    z, meta = golden
    ctx = D.Context(0)
    try:
        ctx.set_option(D.DLG_OPT_NORMALS_FUSED, fused)
        g = D.estimate_normals(z[name + "/points"], radius=meta[name]["radius"], ctx=ctx)
    finally:
        ctx.close()
    want = z[name + "/normals"]
    print(f"{name}: {int(((bits(g) != bits(want)) & ~np.isnan(want)).any(1).sum())} rows differ, "
          f"{int((np.isnan(g) != np.isnan(want)).any(1).sum())} NaN rows differ")
    assert_same_floats(g, want)


@pytest.mark.parametrize("name", ["sheet", "line"])
def test_regulate_walks_the_chains(gpu_ctx, golden, name):
    """RegulateNormal's BFS from the first point of chains of links nearly r long: the processed
    set and the queue length are the oracle's (test_normals.py's BFS oracle)"""
    z, meta = golden
    pts, r = z[name + "/points"], meta[name]["radius"]
    for seed, size in zip(meta[name]["regulate_seeds"], meta[name]["regulate_component_sizes"]):
        nrm = np.zeros((len(pts), 4), f32)
        nrm[:, 2] = np.where(np.random.RandomState(seed).uniform(size=len(pts)) < 0.5, -1.0, 1.0)
        o_reg, o_proc, o_cnt = O.regulate_normals(pts, nrm, seed, True, r)
        assert o_cnt == size == int(o_proc.sum())
        g_reg, g_proc, g_cnt = D.regulate_normals(pts, nrm, seed, True, r, ctx=gpu_ctx)
        print(f"{name} seed {seed}: processed {g_cnt} of {o_cnt}")
        assert g_cnt == o_cnt
        assert np.array_equal(g_proc, o_proc)
        np.testing.assert_array_equal(g_reg, o_reg)


# ---- the cell table's wrap ---------------------------------------------------------------------------
def hash_key(k):
    """grid_dev.hpp's hash_key"""
    k &= 0xffffffff
    k ^= k >> 16
    k = (k * 0x7feb352d) & 0xffffffff
    k ^= k >> 15
    k = (k * 0x846ca68b) & 0xffffffff
    k ^= k >> 16
    return k


def test_table_probe_wraps_and_collides(gpu_ctx, golden, gen):
    z, meta = golden
    pts, r = z["wrap/points"], meta["wrap"]["radius"]
    # the occupied cells (every point lies 0.2 of a cell or more from a face: float64 suffices)
    lo = pts.min(0).astype(f64)
    c = np.floor((pts.astype(f64) - lo) / (r / (1.0 - 1e-3))).astype(np.int64)
    assert c[:, :2].max() == gen.WRAP_G - 1 and c[:, 2].max() == 0
    keys = sorted(set(int(v) for v in c[:, 1] * gen.WRAP_G + c[:, 0]))
    assert len(keys) <= 512  # (the table keeps its smallest size: 1,024 entries)
    slots = [hash_key(k) & 1023 for k in keys]
    assert slots.count(1023) >= 3  # the second and third of them probe on at slot 0
    assert slots.count(500) >= 4
    ref = M.mls_ref(pts, r)
    xyz, nrm, src, nb, st = D.moving_least_squares(pts, r, ctx=gpu_ctx, return_stats=True)
    assert np.array_equal(nb, ref["neighbours"]) and np.array_equal(nb, z["wrap/nb"])
    assert np.array_equal(src, ref["src_index"])
    assert {q: st[q] for q in M.STAT_KEYS} == ref["stats"]


# ---- the k-NN grids ------------------------------------------------------------------------------------
def sorted_knn_d2(pts, queries, k, reach=64, chunk=16384):
    """sor_ref.knn_d2 for clouds that are thin across x: the k smallest float32 flann_d2 of every
    query, ascending, among the `reach` points on either side of it in x order.  Exact: the
    nearest point outside that window is farther in x alone than the k-th distance found."""
    order = np.argsort(pts[:, 0], kind="stable")
    s = pts[order]
    x = s[:, 0].astype(f64)
    n = len(s)
    out = np.empty((len(queries), k), f32)
    for a in range(0, len(queries), chunk):
        q = queries[a:a + chunk]
        pos = np.searchsorted(x, q[:, 0].astype(f64))
        idx = pos[:, None] + np.arange(-reach, reach)[None, :]
        inside = (idx >= 0) & (idx < n)
        cand = s[np.clip(idx, 0, n - 1)]
        d = np.zeros(idx.shape, f32)
        for ax in range(3):
            e = (q[:, None, ax] - cand[:, :, ax]).astype(f32)
            d = (d + (e * e).astype(f32)).astype(f32)
        d[~inside] = np.inf
        best = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1)
        qx = q[:, 0].astype(f64)
        left = np.where(pos - reach - 1 >= 0, qx - x[np.clip(pos - reach - 1, 0, n - 1)], np.inf)
        right = np.where(pos + reach < n, x[np.clip(pos + reach, 0, n - 1)] - qx, np.inf)
        assert (np.minimum(left, right) ** 2 > best[:, -1].astype(f64) * (1.0 + 1e-5)).all()
        out[a:a + chunk] = best
    return out


@pytest.fixture(scope="module", params=["knn_line", "knn_strip"])
def knn_cloud(request, gen, golden):
    pts, aimed = gen.CLOUDS[request.param]()
    assert gen.digest(pts) == golden[1][request.param]["sha256"]
    if aimed is not None:  # (knn_line: queries placed so that a violated bound costs a neighbour)
        assert [int(v) for v in aimed] == golden[1][request.param]["aimed_queries"]
        assert len(aimed) >= 8
    assert pts[:, 0].min() < -31.0 and pts[:, 0].max() > 28.0  # straddles the origin
    return request.param, pts


def test_knn_normals_bit_exact(gpu_ctx, knn_cloud, gen):
    name, pts = knn_cloud
    o = O.estimate_normals_knn(pts, gen.KNN_K)
    g = D.estimate_normals(pts, k=gen.KNN_K, ctx=gpu_ctx)
    print(f"{name}: {int(((bits(g) != bits(o)) & ~np.isnan(o)).any(1).sum())} rows differ")
    assert_same_floats(g, o)
    if name == "knn_strip":
        assert np.isfinite(o).all(1).mean() > 0.99  # (the strip's normals are proper ones)


def test_sor_kept_set(gpu_ctx, knn_cloud, gen, monkeypatch):
    name, pts = knn_cloud
    monkeypatch.setattr(S, "knn_d2", lambda cloud, queries, k, chunk=512: sorted_knn_d2(cloud, queries, k))
    ref = S.sor_ref(pts, gen.KNN_K, 1.0)
    kept, removed, dist = D.statistical_outlier_removal(pts, gen.KNN_K, 1.0, ctx=gpu_ctx)
    print(f"{name}: {int((bits(dist) != bits(ref['distances'])).sum())} distances differ, "
          f"kept {len(kept)} of {len(ref['kept'])}")
    assert np.array_equal(bits(dist), bits(ref["distances"]))
    assert np.array_equal(kept, ref["kept"]) and np.array_equal(removed, ref["removed"])
    assert 0 < len(removed) < len(pts)


def test_icp_correspondences(gpu_ctx, knn_cloud):
    """2^15 queries beside the cloud (moved by a fraction of the point spacing) against all 2^17"""
    name, pts = knn_cloud
    rng = np.random.RandomState(77)
    src = pts[rng.permutation(len(pts))[:1 << 15]].astype(f64)
    src += rng.normal(0.0, 1e-4, src.shape) * (pts.max(0) > pts.min(0))
    src = src.astype(f32)
    info = {}
    rn, rd = R.correspondences_fast(src, pts, info=info)
    nn, d2 = D.icp_correspondences(src, pts, ctx=gpu_ctx)
    print(f"{name}: {int((nn != rn).sum())} of {len(nn)} correspondences differ "
          f"({info['uncertified']} by brute force)")
    assert np.array_equal(nn, rn) and np.array_equal(bits(d2), bits(rd))
