"""CPU: the numpy restatement of pcl::FPFHEstimation (tests/fpfh_ref.py) -- the fixture
tests/golden/fpfh_small.npz against a recomputation, the cap on unstable rows, the neighbour order
really showing in the bits -- fpfh_model.hpp's host side under ASan + UBSan against the reference,
the C++ shim, and the ABI.  The device path is tests/test_fpfh_gpu.py.

The parity rule: neighbour counts, NaN rows, zero rows and the integer stats are exact; the SPFH
counts equal the reference's at its stable points; the descriptors are bit-equal at its stable
rows (given equal counts everything after them is IEEE + * / in a fixed order: no ulp allowance).
"""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import fpfh_ref as F
from dialog_amd import _lib, pcd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
f32 = np.float32
STEP = 8  # tests/golden/make_fpfh.py keeps every STEP-th row of the tables
CASES = ("shadow", "planes", "sphere", "dense", "near_dup", "dups_nan", "indices", "thin")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fpfh_small.npz"))
    return z, json.loads(str(z["meta"]))


@pytest.fixture(scope="module")
def refs(golden):
    """the reference rerun on the fixture's inputs, once per case"""
    z, meta = golden
    out = {}

    def get(name):
        if name not in out:
            idx = z[name + "/idx"] if name + "/idx" in z.files else None
            out[name] = F.fpfh_ref(z[name + "/points"], z[name + "/normals"], meta[name]["radius"],
                                   idx)
        return out[name]
    return get


def unpack(z, key, n):
    return np.unpackbits(z[key])[:n].astype(bool)


# ---- the fixture --------------------------------------------------------------------------------
def test_fixture_inputs_are_the_cases(golden):
    z, meta = golden
    shadow = np.ascontiguousarray(
        pcd.read_pcd(os.path.join(ROOT, "tests", "golden", "double_shadow.pcd"))[:, :3], f32)
    cs = F.cases(shadow)
    assert set(cs) == set(CASES) == set(meta)
    for name, (pts, r_normals, radius, idx) in cs.items():
        assert np.array_equal(bits(pts), bits(z[name + "/points"])), name
        assert meta[name]["radius"] == radius and meta[name]["r_normals"] == r_normals
        assert (idx is None) == (name + "/idx" not in z.files)
        assert len(pts) < 3000
    nrm = F.pca_normals(cs["planes"][0], cs["planes"][1])
    assert np.array_equal(bits(nrm), bits(z["planes/normals"]))
    assert int(np.isnan(nrm).any(1).sum()) == 89  # the case's NaN normals


@pytest.mark.parametrize("name", CASES)
def test_fixture_equals_the_reference(golden, refs, name):
    z, meta = golden
    ref = refs(name)
    n, m = len(z[name + "/points"]), len(ref["hist"])
    assert np.array_equal(ref["neighbours"], z[name + "/nb"].astype(np.int32))
    assert np.array_equal(ref["stable"], unpack(z, name + "/stable", m))
    assert np.array_equal(ref["stable_spfh"], unpack(z, name + "/stable_spfh", n))
    assert ref["stats"] == meta[name]["stats"]
    assert np.array_equal(bits(ref["hist"][::STEP]), bits(z[name + "/hist"]))
    assert np.array_equal(ref["counts"][::STEP], z[name + "/counts"].astype(np.int32))
    assert digest(ref["hist"]) == meta[name]["hist_sha"]
    assert digest(ref["counts"]) == meta[name]["counts_sha"]


@pytest.mark.parametrize("name", CASES)
def test_unstable_rows_within_the_cap(golden, name):
    """at most 1 % of a case's rows (and of its points' SPFHs) may be unstable: a condition of
    the cases, not a measurement"""
    z, _ = golden
    n = len(z[name + "/points"])
    m = len(z[name + "/nb"])
    assert (~unpack(z, name + "/stable", m)).sum() <= 0.01 * m
    assert (~unpack(z, name + "/stable_spfh", n)).sum() <= 0.01 * n


def test_the_cases_reach_their_paths(golden, refs):
    z, meta = golden
    nb = z["shadow/nb"]
    assert (nb.min(), int(np.median(nb)), nb.max()) == (50, 168, 282)
    st = {k: meta[k]["stats"] for k in meta}
    assert st["planes"]["n_zero_rows"] > 0 and st["planes"]["n_pairs_failed"] > 0
    assert 100 <= st["dense"]["n_lds_overflow"] <= 500 and st["dense"]["max_neighbours"] > F.CAP
    assert st["near_dup"]["n_sum_literal"] > 0 and st["shadow"]["n_sum_literal"] == 0
    assert st["dups_nan"]["n_nan_rows"] == 4 and st["dups_nan"]["n_finite"] == 346
    # NaN entries are NaN rows, every other row is finite
    h = refs("dups_nan")
    assert np.isnan(h["hist"][[5, 77, 120, 301]]).all() and (h["neighbours"][[5, 77]] == -1).all()
    assert np.isfinite(np.delete(h["hist"], [5, 77, 120, 301], 0)).all()
    # the sphere fills all 33 bins and takes both branches of the swap
    assert (refs("sphere")["counts"].sum(0) > 0).all()


def test_histograms_sum_to_100(refs):
    ref = refs("shadow")
    sums = ref["hist"].astype(np.float64).reshape(-1, 3, 11).sum(2)
    assert np.abs(sums - 100.0).max() < 1e-3


def test_index_list_rows_are_the_full_run_s(golden, refs):
    z, _ = golden
    idx = z["indices/idx"]
    assert len(set(idx.tolist())) < len(idx)  # (repeats)
    assert np.array_equal(bits(refs("indices")["hist"]), bits(refs("shadow")["hist"][idx]))
    assert np.array_equal(refs("indices")["neighbours"], refs("shadow")["neighbours"][idx])


def test_the_neighbour_order_shows_in_the_bits(golden, refs):
    """summing in index order instead of (d2, index) order changes the float sums' bits"""
    z, meta = golden
    wrong = F.fpfh_ref(z["shadow/points"], z["shadow/normals"], meta["shadow"]["radius"],
                       order="index")
    changed = (bits(wrong["hist"]) != bits(refs("shadow")["hist"])).any(1)
    assert changed.mean() > 0.9
    assert np.array_equal(wrong["counts"], refs("shadow")["counts"])  # (not the integer part)


# ---- fpfh_model.hpp on the host, under the sanitizers ------------------------------------------
@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fsan") / "fpfh_model_san")
    subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "dialog_amd/csrc"),
                    os.path.join(ROOT, "tests/cpp/fpfh_model_san.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("name", CASES)
def test_model_header_against_the_reference(model_exe, golden, refs, tmp_path, name):
    z, meta = golden
    pts, nrm = z[name + "/points"], z[name + "/normals"]
    n = len(pts)
    lst = z[name + "/idx"] if name + "/idx" in z.files else np.arange(n, dtype=np.int32)
    m = len(lst)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([n, m], np.int32).tobytes())
        f.write(f32(meta[name]["radius"]).tobytes())
        f.write(np.ascontiguousarray(pts, f32).tobytes())
        f.write(np.ascontiguousarray(nrm[:, :3], f32).tobytes())
        f.write(np.ascontiguousarray(lst, np.int32).tobytes())
    r = subprocess.run([model_exe, src, dst], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(dst, "rb").read()
    assert len(raw) == 4 * 33 * (n + m) + 5 * m
    cnt = np.frombuffer(raw, np.int32, n * 33).reshape(n, 33)
    hist = np.frombuffer(raw, f32, m * 33, 4 * 33 * n).reshape(m, 33)
    nb = np.frombuffer(raw, np.int32, m, 4 * 33 * (n + m))
    lit = np.frombuffer(raw, np.uint8, m, 4 * 33 * (n + m) + 4 * m)
    ref = refs(name)
    assert np.array_equal(nb, ref["neighbours"])
    sp, st = ref["stable_spfh"], ref["stable"]
    assert np.array_equal(cnt[sp], ref["counts"][sp])
    assert np.array_equal(bits(hist[st]), bits(ref["hist"][st]))
    assert int(lit.sum()) == ref["stats"]["n_sum_literal"]


# ---- shim, ABI ---------------------------------------------------------------------------------
def test_cpp_fpfh_shim_compiles_and_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "shim_fpfh.cpp")
    exe = tmp_path / "shim_fpfh"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o",
           str(exe), "-L", os.path.dirname(_lib.LIB_PATH), "-ldialog_amd",
           f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_fpfh_struct_layouts_match_the_header():
    L = _lib.load()
    assert L.dlg_abi_struct_size(17) == C.sizeof(_lib.FpfhParams) == 4
    assert L.dlg_abi_struct_size(18) == C.sizeof(_lib.FpfhStats) == 96
    for which in (12, 16, 99):
        assert L.dlg_abi_struct_size(which) == -1
    assert L.dlg_abi_version() == 5 == _lib.ABI_VERSION
    for s in ("dlg_fpfh_estimate", "dlg_cloud_fpfh"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    import dialog_amd as D
    assert callable(D.fpfh_estimation) and callable(D.cloud_fpfh)


def test_null_handles_are_invalid_without_a_device():
    """the argument checks that need no context (the rest: tests/test_fpfh_gpu.py)"""
    L = _lib.load()
    prm = _lib.FpfhParams(0.1)
    assert L.dlg_fpfh_estimate(None, None, None, 12, None, 0, C.byref(prm), None, 132, None, None,
                               None) == _lib.DLG_ERR_INVALID
    assert L.dlg_cloud_fpfh(None, None, C.byref(prm), None, 132, None, None) == _lib.DLG_ERR_INVALID
