"""The neighbour-search grid's arithmetic (dialog_amd/csrc/grid_model.hpp: make_grid, cell_of, the
k-NN kernels' distance bound) on the host, at the grid shapes the fixture clouds never reach: up to
2^20 cells on an axis, sheets and lines, boxes at zero, straddling zero and far from it.

tests/cpp/grid_model_host.cpp (built with ASan + UBSan, never loaded into Python) builds the grid
and aims directed samples with the map; the verdicts here use plain float32 / float64 numpy:

* adjacency: whenever flann_d2(q, p) < r2 (the radius searches) or < G.cell^2 (the k-NN levels'
  guaranteed radius), the cell indices of q and p differ by at most 1 on every axis: the 27-cell
  scan visits p;
* the k-NN bound: the lower bound md that the kernels compute for a neighbouring cell never
  exceeds the flann_d2 of a point of that cell: a cell is never skipped wrongly;
* make_grid's outputs, and that degenerate boxes terminate.

The fixture's conditions (tests/golden/grid_edges.npz) are asserted here too: its clouds must
break the previous arithmetic (inv_cell shrunk by 1e-3 and an allowance of 1e-4 at every width),
else the GPU tests in tests/test_grid_edges_gpu.py could not fail.
"""
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
f32, f64 = np.float32, np.float64
REC = np.dtype([("q", f32, 3), ("p", f32, 3), ("cq", np.int32, 3), ("cp", np.int32, 3),
                ("md", f32), ("kind", np.int32)])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("grid") / "grid_model_host")
    subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "dialog_amd/csrc"),
                    os.path.join(ROOT, "tests/cpp/grid_model_host.cpp"), "-o", out], check=True)
    return out


def hx(v):
    return float(v).hex()


def run(exe, lo, hi, cell, n_adj=0, n_knn=0, seed=1, any_=True):
    """one request -> (the GridDesc as a dict, the sample records)"""
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    req = " ".join([*(hx(v) for v in lo), *(hx(v) for v in hi), str(int(any_)), hx(cell),
                    str(n_adj), str(n_knn), str(seed)]) + "\n"
    r = subprocess.run([exe], input=req.encode(), capture_output=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:].decode()
    head, _, rest = r.stdout.partition(b"\n")
    t = head.split()
    G = dict(g=[int(x) for x in t[:3]], ncells=int(t[3]), key_bits=int(t[4]),
             lo=[float.fromhex(x.decode()) for x in t[5:8]], cell=float.fromhex(t[8].decode()),
             inv_cell=float.fromhex(t[9].decode()), slack=float.fromhex(t[10].decode()))
    cnt = int(np.frombuffer(rest[:4], np.uint32)[0])
    rec = np.frombuffer(rest[4:], REC)
    assert len(rec) == cnt
    return G, rec


def flann_d2(q, p):
    """rows of q and p (n, 3) float32 -> ((0 + dx^2) + dy^2) + dz^2, every operation in float32"""
    acc = np.zeros(len(q), f32)
    for a in range(3):
        e = (q[:, a] - p[:, a]).astype(f32)
        acc = (acc + (e * e).astype(f32)).astype(f32)
    return acc


# ---- the grids -------------------------------------------------------------------------------------
EXT = 30.0
WIDTHS = [64, 1024, 4096, 16384, 30000, 1 << 16, 1 << 20]
# lo at 0, straddling zero (-15.3 of extent 30) and far from zero
LOS = [0.0, -15.3, 1000.0]


def shapes(w):
    """(name, cells per axis) with the product under 2^30"""
    out = [("line", (w, 1, 1))]
    second = min(w, (1 << 30) // w // 2)
    if second >= 3:
        out.append(("sheet", (w, second, 1)))
    return out


def box_for(cells, lo0, cell):
    """a box with exactly `cells` cells per axis at cell edge `cell`, its x axis starting at lo0"""
    lo = np.array([lo0, lo0 * 0.5 - 1.0, 2.0], f32)
    hi = (lo.astype(f64) + (np.array(cells, f64) - 0.5) * cell).astype(f32)
    return lo, hi


CASES = [(w, name, cells, lo0) for w in WIDTHS for name, cells in shapes(w) for lo0 in LOS]


@pytest.mark.parametrize("w,name,cells,lo0", CASES,
                         ids=[f"{n}-{w}-lo{lo0:g}" for w, n, _, lo0 in CASES])
def test_adjacency_and_knn_bound(exe, w, name, cells, lo0):
    cell = EXT / (w - 0.5)
    lo, hi = box_for(cells, lo0, cell)
    G, rec = run(exe, lo, hi, cell, n_adj=40000, n_knn=40000, seed=w + int(lo0))
    # the grid is the requested one (no axis above the cap, the product below 2^30), up to the
    # rounding of the box's corners to float
    assert all(abs(a - b) <= 1 + b * 1e-5 for a, b in zip(G["g"], cells)), (G["g"], cells)
    assert len(rec) == 80000
    q, p = rec["q"], rec["p"]
    d2 = flann_d2(q, p)
    step = np.abs(rec["cq"] - rec["cp"]).max(1)
    adj = rec["kind"] == 0
    r2 = f32(f64(f32(cell)) * f64(f32(cell)))     # the drivers' r2 of a float radius `cell`
    lim = f32(f32(G["cell"]) * f32(G["cell"]))    # the k-NN levels' guaranteed radius
    for name_, bound in (("r2", r2), ("G.cell^2", lim)):
        inside = adj & (d2 < bound)
        # the samples are aimed: a share of the partners is inside the radius (few where the
        # floats of the box are as coarse as the 0.002 r band, none where they are coarser than r)
        assert inside.sum() > 100 or lo0 == 1000.0 and w > 30000, (name_, int(inside.sum()))
        bad = inside & (step > 1)
        assert not bad.any(), (name_, int(bad.sum()), int(inside.sum()), rec[bad][:3])
    knn = (rec["kind"] == 1) & (step == 1)
    # (at 2^20 cells the map's own error moves a share of the aimed queries to the next cell)
    assert knn.sum() > 1000
    # float64 says the same of the true distance, to the (1 - 1e-5) the bound is scaled by
    d2_64 = ((q.astype(f64) - p.astype(f64)) ** 2).sum(1)
    bad = knn & ((rec["md"] > d2) | (rec["md"].astype(f64) > d2_64))
    assert not bad.any(), (int(bad.sum()), int(knn.sum()), rec[bad][:3], d2[bad][:3])
    # and the bound is not vacuous: most neighbour cells get a positive one
    assert (rec["md"][knn] > 0).mean() > 0.5


@pytest.mark.parametrize("lo0", LOS)
def test_grown_grids(exe, lo0):
    """a box whose product exceeds 2^30 (the cell grows by 1.25 until it fits) and a line of 2^24
    requested cells (grown to the per-axis cap): the same invariants, against the grown cell"""
    for cells in ((4096, 4096, 4096), (1 << 24, 1, 1)):
        cell = EXT / (cells[0] - 0.5)
        lo, hi = box_for(cells, lo0, cell)
        G, rec = run(exe, lo, hi, cell, n_adj=20000, n_knn=20000, seed=7)
        assert max(G["g"]) <= 1 << 20 and G["g"][0] * G["g"][1] * G["g"][2] <= 1 << 30
        assert max(G["g"]) < cells[0]
        # the samples step by the requested cell, a fraction of the grown one: all inside
        d2 = flann_d2(rec["q"], rec["p"])
        step = np.abs(rec["cq"] - rec["cp"]).max(1)
        adj = rec["kind"] == 0
        assert not (adj & (step > 1)).any()
        knn = (rec["kind"] == 1) & (step == 1)
        assert knn.sum() > 1000 and not (knn & (rec["md"] > d2)).any()


def check_desc(G, lo, hi, cell, any_=True):
    ext = (np.asarray(hi, f32).astype(f64) - np.asarray(lo, f32).astype(f64)) if any_ else np.zeros(3)
    assert all(g >= 1 for g in G["g"])
    prod = G["g"][0] * G["g"][1] * G["g"][2]
    assert prod == G["ncells"] <= 1 << 30 and max(G["g"]) <= 1 << 20
    # key ncells itself (a non-finite point) fits the sorted bits
    assert (1 << G["key_bits"]) > G["ncells"] and G["key_bits"] <= 31
    assert G["lo"] == ([float(v) for v in np.asarray(lo, f32)] if any_ else [0.0, 0.0, 0.0])
    # the effective cell edge of the map is at least the requested cell, and so is the coverage
    # radius the k-NN levels rely on, to its 1e-6
    assert 1.0 / G["inv_cell"] >= cell
    assert G["cell"] >= cell * (1 - 2e-6)
    # every point of the box maps inside the grid: (hi - lo) * inv_cell < g
    assert all(e * G["inv_cell"] < g for e, g in zip(ext, G["g"]))
    assert float(f32(1e-4)) <= G["slack"] < 0.3
    return prod


def test_make_grid_outputs(exe):
    for w, name, cells, lo0 in CASES:
        cell = EXT / (w - 0.5)
        lo, hi = box_for(cells, lo0, cell)
        G, _ = run(exe, lo, hi, cell)
        check_desc(G, lo, hi, cell)
    # up to 1,024 cells per axis the descriptor is the one of the 1e-3 shrink and the 1e-4 / E(g)
    # allowance, bit for bit
    lo, hi = box_for((1024, 700, 3), -15.3, 0.03)
    G, _ = run(exe, lo, hi, 0.03)
    assert G["g"] == [1024, 700, 3]
    assert G["inv_cell"] == float(f32((1.0 / 0.03) * (1.0 - 1e-3)))
    assert G["cell"] == float(f32(0.03 * (1.0 - 1e-6)))
    lo, hi = box_for((300, 300, 300), 0.0, 0.1)
    assert run(exe, lo, hi, 0.1)[0]["slack"] == float(f32(1e-4))


def test_degenerate_boxes_terminate(exe):
    one = np.array([1.5, -2.0, 3.0], f32)
    G, rec = run(exe, one, one, 0.01, n_adj=10, n_knn=10)
    assert G["g"] == [1, 1, 1] and G["ncells"] == 1 and G["key_bits"] == 1 and len(rec) == 0
    check_desc(G, one, one, 0.01)
    G, _ = run(exe, [np.inf] * 3, [-np.inf] * 3, 0.01, any_=False)
    assert G["g"] == [1, 1, 1] and G["lo"] == [0.0, 0.0, 0.0]
    check_desc(G, [0] * 3, [0] * 3, 0.01, any_=False)
    for cell in (1e-3, 1.0, 1e25):
        lo, hi = [-1e30] * 3, [1e30] * 3
        G, rec = run(exe, lo, hi, cell, n_adj=1000, n_knn=1000)
        check_desc(G, lo, hi, cell)
        assert np.isfinite(G["inv_cell"]) and G["inv_cell"] > 0
        step = np.abs(rec["cq"] - rec["cp"]).max(1)
        assert not ((rec["kind"] == 0) & (step > 1)).any()


# ---- the fixture of the GPU tests --------------------------------------------------------------
@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location(
        "make_grid_edges", os.path.join(ROOT, "tests", "golden", "make_grid_edges.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_generator_restates_the_model(exe, gen):
    """make_grid and cell_of as tests/golden/make_grid_edges.py restates them in numpy, against the
    header: the descriptor's bits, and the cells of the samples"""
    for w, name, cells, lo0 in CASES[::3] + [(0, "grown", (4096, 4096, 4096), -15.3)]:
        cell = EXT / (cells[0] - 0.5)
        lo, hi = box_for(cells, lo0, cell)
        G, rec = run(exe, lo, hi, cell, n_adj=2000, n_knn=2000, seed=3)
        P = gen.make_grid(lo, hi, cell)
        assert [int(v) for v in P["g"]] == G["g"]
        assert (float(P["inv_cell"]), float(P["cell"]), float(P["slack"])) == \
            (G["inv_cell"], G["cell"], G["slack"])
        assert np.array_equal(gen.cells_of(rec["q"], P), rec["cq"])
        assert np.array_equal(gen.cells_of(rec["p"], P), rec["cp"])


def test_fixture_breaks_the_previous_arithmetic(gen):
    """the stored clouds are the generator's, and under the emulation of the previous map (float32
    numpy) they hold what the GPU tests need in order to be able to fail"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "grid_edges.npz"))
    meta = json.loads(str(z["meta"]))
    for name in ("sheet", "line"):
        pts = z[name + "/points"]
        r = meta[name]["radius"]
        assert np.array_equal(pts.view(np.uint32), gen.CLOUDS[name]()[0].view(np.uint32))
        far = gen.count_two_apart(pts, r, gen.previous_grid(pts, r))
        assert far == meta[name]["pairs_two_cells_apart_previous_map"]
        assert far >= 100, (name, far)
        now = gen.count_two_apart(pts, r, gen.model_grid(pts, r))
        assert now == 0, (name, now)
    for name in ("knn_line", "knn_strip"):
        pts = gen.CLOUDS[name]()[0]
        assert gen.digest(pts) == meta[name]["sha256"]
        assert meta[name]["bound_violations_previous_map"] > 0
