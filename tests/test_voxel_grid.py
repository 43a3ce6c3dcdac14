"""CPU: the voxel-grid filter's reference (tests/voxel_ref.py) against an independent
characterisation, voxel_model.hpp's host side under ASan + UBSan against the reference, the C++
shim, and the ABI structs.  The device path is tests/test_voxel_grid_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import voxel_ref as V
from dialog_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

FIXTURES = {
    "uniform": (V.uniform_cloud(), (0.25, 0.25, 0.25)),
    "quantised": (V.quantised_cloud(), (0.1, 0.1, 0.1)),
    "anisotropic": (V.uniform_cloud(3000, seed=5), (0.5, 0.125, 2.0)),
    "ladder": (V.ladder_cloud(), (1.0, 1.0, 1.0)),
}


@pytest.fixture(scope="module")
def refs():
    return {k: V.voxel_ref(p, leaf) for k, (p, leaf) in FIXTURES.items()}


def test_issue_fixture_figures(refs):
    """the figures the fixtures were chosen for: 4067 voxels of 1..17 points; reversing the order
    inside a voxel changes centroid bits; a double-precision key changes the partition"""
    r = refs["uniform"]
    assert len(r["xyz"]) == 4067 and r["counts"].min() == 1 and r["counts"].max() == 17
    p, leaf = FIXTURES["uniform"]
    d = V.voxel_ref(p, leaf, order="desc")
    differ = (d["xyz"].view(np.uint32) != r["xyz"].view(np.uint32)).any(1)
    assert differ.sum() > 1000
    assert not differ[r["counts"] <= 2].any()  # (sums of at most 2 points: any order)
    q, leaf = FIXTURES["quantised"]
    k = V.voxel_ref(q, leaf, key_double=True)
    a = refs["quantised"]
    assert len(k["xyz"]) != len(a["xyz"]) or (k["voe"] != a["voe"]).any()


@pytest.mark.parametrize("name", list(FIXTURES))
def test_reference_against_characterisation(refs, name):
    p, leaf = FIXTURES[name]
    r = refs[name]
    lf = np.asarray(leaf, np.float32)
    inv = (np.float32(1) / lf).astype(np.float32)
    # the partition: np.unique over the integer cell triples (float32 floor, as the semantics say)
    cell = np.floor((p * inv).astype(np.float32)).astype(np.int64)
    _, inverse, counts = np.unique(cell, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    voe = r["voe"]
    assert (voe >= 0).all() and len(r["xyz"]) == len(counts)
    # same partition: entries share an output row exactly when they share a cell triple
    pair = np.unique(np.stack([voe, inverse], 1), axis=0)
    assert len(pair) == len(counts) == len(np.unique(pair[:, 0])) == len(np.unique(pair[:, 1]))
    # voxel_of_entry is consistent with counts
    assert np.array_equal(np.bincount(voe, minlength=len(r["xyz"])), r["counts"])
    # ordered by key, strictly
    assert (np.diff(r["keys"].astype(np.int64)) > 0).all()
    # every centroid within count * 2^-23 * max|p| of the float64 mean
    mean = np.zeros((len(counts), 3))
    np.add.at(mean, voe, p.astype(np.float64))
    mean /= r["counts"][:, None]
    bound = r["counts"] * 2.0**-23 * np.abs(p).max()
    assert (np.abs(r["xyz"] - mean).max(1) <= bound).all()


def test_reference_min_points_indices_and_nonfinite():
    p = V.uniform_cloud(4000, seed=11)
    p[::37, 0] = np.nan
    p[5::37 * 3, 1] = np.inf
    p[9::37 * 5, 2] = -np.inf
    rng = np.random.default_rng(2)
    idx = rng.integers(0, len(p), 5000)
    full = V.voxel_ref(p, 0.5, idx=idx)
    fin = np.isfinite(p[idx]).all(1)
    assert (full["voe"][~fin] == -1).all() and (full["voe"][fin] >= 0).all()
    assert full["n_finite"] == fin.sum()
    for mp in (1, 2, 5):
        r = V.voxel_ref(p, 0.5, idx=idx, min_points=mp)
        keep = full["counts"] >= mp
        assert np.array_equal(r["xyz"].view(np.uint32), full["xyz"][keep].view(np.uint32))
        assert np.array_equal(r["counts"], full["counts"][keep])
        dropped = fin & ~keep[np.where(fin, full["voe"], 0)]
        assert (r["voe"][dropped] == -1).all() and (r["voe"][fin & ~dropped] >= 0).all()
    allnan = V.voxel_ref(np.full((10, 3), np.nan, np.float32), 1.0)
    assert len(allnan["xyz"]) == 0 and (allnan["voe"] == -1).all()


# ---- voxel_model.hpp on the host, under the sanitizers ------------------------------------------
@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vsan") / "voxel_model_san")
    subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "dialog_amd/csrc"),
                    os.path.join(ROOT, "tests/cpp/voxel_model_san.cpp"), "-o", exe], check=True)
    return exe


def run_model(exe, p, leaf):
    lf = np.broadcast_to(np.asarray(leaf, np.float32), (3,))
    lines = [" ".join(float(v).hex() for v in lf) + f" {len(p)}"]
    lines += [" ".join(float(v).hex() for v in row) for row in p]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       env=ENV, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        w = line.split()
        out[w[0]] = w[1:]
    return out


@pytest.mark.parametrize("name", list(FIXTURES))
def test_model_header_keys_equal_reference(model_exe, name):
    p, leaf = FIXTURES[name]
    if name == "uniform":  # (non-finite entries are skipped, negative zero and exact multiples stay)
        p = p.copy()
        p[::37, 1] = np.nan
        p[1::37, 0] = -0.0
        p[2::37, 2] = np.float32(0.25) * np.round(p[2::37, 2] * 4)
    out = run_model(model_exe, p, leaf)
    assert out["verdict"] == ["0"]
    fin = np.isfinite(p).all(1)
    q = p[fin]
    inv, min_b, div = V.grid(q.min(0), q.max(0), leaf)
    assert [int(v) for v in out["div"]] == list(div)
    assert [int(v) for v in out["min_b"]] == list(min_b)
    keys = np.array([int(v) for v in out["keys"]], np.uint32)
    assert np.array_equal(keys, V.keys_of(q, inv, min_b, div))
    total = int(div[0]) * int(div[1]) * int(div[2])
    assert int(keys.max()) < total <= 2 ** int(out["bits"][0])


def test_model_header_verdicts(model_exe):
    p = V.uniform_cloud()
    for leaf, want, exc in ((1e-4, "1", V.LeafTooSmall), (5e-3, "0", None), (0.25, "0", None)):
        assert run_model(model_exe, p[:500], leaf)["verdict"] == [want]
        if exc:
            with pytest.raises(exc):
                V.voxel_ref(p[:500], leaf)
    # one voxel along y and z, 2^31 along x: too small; huge coordinates over a small extent:
    # the cell index leaves the int range
    line = np.zeros((2, 3), np.float32)
    line[1, 0] = 3e9
    assert run_model(model_exe, line, 1.0)["verdict"] == ["1"]
    far = np.array([[3e12, 0, 0], [3e12, 1, 1]], np.float32)
    assert run_model(model_exe, far, 1.0)["verdict"] == ["2"]
    with pytest.raises(V.OutOfIntRange):
        V.voxel_ref(far, 1.0)
    huge = np.array([[-3e38, 0, 0], [3e38, 0, 0]], np.float32)  # max - min overflows to inf
    assert run_model(model_exe, huge, 1.0)["verdict"] == ["1"]
    with pytest.raises(V.LeafTooSmall):
        V.voxel_ref(huge, 1.0)
    assert "empty" in run_model(model_exe, np.full((3, 3), np.nan, np.float32), 1.0)
    # a cloud straddling 0 falls into 8 voxels, a positive one into 1
    q = (p[:5000] * np.float32(0.25)).astype(np.float32)
    assert len(set(run_model(model_exe, q, 100.0)["keys"])) == 8
    assert len(set(run_model(model_exe, q + np.float32(3), 100.0)["keys"])) == 1


# ---- shim, ABI ---------------------------------------------------------------------------------
def test_cpp_voxel_shim_compiles_and_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "shim_voxel.cpp")
    exe = tmp_path / "shim_voxel"
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", str(exe),
           "-L", os.path.dirname(_lib.LIB_PATH), "-ldialog_amd",
           f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_voxel_struct_layouts_match_the_header():
    L = _lib.load()
    assert L.dlg_abi_struct_size(6) == C.sizeof(_lib.VoxelParams) == 16
    assert L.dlg_abi_struct_size(7) == C.sizeof(_lib.VoxelStats) == 48
    assert _lib.DLG_OPT_VOXEL_LONG_RUN == 24
    assert "dlg_voxel_grid" in _lib.SYMBOLS and "dlg_voxel_grid_cloud" in _lib.SYMBOLS
    assert hasattr(L, "dlg_voxel_grid") and hasattr(L, "dlg_voxel_grid_cloud")
