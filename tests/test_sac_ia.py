"""CPU: the numpy restatement of pcl::SampleConsensusInitialAlignment (tests/sac_ia_ref.py) -- the
two rand() generators' known answers, the fixture tests/golden/sac_ia_small.npz against a
recomputation, the cases reaching their paths -- sacia_model.hpp's host side under ASan + UBSan
against the fixture, the C++ shim, and the ABI.  The device path is tests/test_sac_ia_gpu.py.

The parity rule: every integer (draws, samples, matches, ranks, counts, both error words) and every
float's bits (T, final, aligned, the error, the fitness) are equal; nothing has a tolerance.
"""
import ctypes as C
import ctypes.util
import json
import os
import subprocess

import numpy as np
import pytest

import sac_ia_ref as S
from dialog_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]  # (test_fpfh.py's)
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
f32 = np.float32
SCALARS = ("converged", "best_iteration", "n_valid", "n_invalid", "draws", "relaxations",
           "n_queries", "error", "fitness")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_floats(a, b):
    """bit-equal where finite, non-finite in the same places (a NaN's payload is not pinned)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    fin = np.isfinite(a)
    return a.shape == b.shape and np.array_equal(fin, np.isfinite(b)) and \
        np.array_equal(bits(a)[fin], bits(b)[fin]) and np.array_equal(np.isnan(a), np.isnan(b))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "sac_ia_small.npz"))
    return z, json.loads(str(z["meta"]))


def load_case(golden, name):
    z, meta = golden
    m = meta[name]
    case = {k: z[key] for k, key in m["inputs"].items()}
    if "guess" in case:
        case["guess"] = case["guess"].reshape(4, 4)
    case.update(m["args"])
    return case


@pytest.fixture(scope="module")
def reruns(golden):
    """the restatement run now on the fixture's inputs, once per case"""
    out = {}

    def get(name):
        if name not in out:
            out[name] = S.run_case(load_case(golden, name))
        return out[name]
    return get


# ---- rand() -------------------------------------------------------------------------------------
def test_generators_known_answers():
    g = S.Rand(S.RNG_GLIBC, 1)
    assert [g.next() for _ in range(5)] == [1804289383, 846930886, 1681692777, 1714636915,
                                            1957747793]
    m = S.Rand(S.RNG_MSVC, 1)
    assert [m.next() for _ in range(5)] == [41, 18467, 6334, 26500, 19169]
    assert S.Rand(S.RNG_GLIBC, 0).next() == 1804289383  # (seed 0 is seed 1)


def test_glibc_generator_against_libc():
    name = ctypes.util.find_library("c")
    if not name:
        pytest.skip("no libc to load")
    libc = C.CDLL(name)
    if not hasattr(libc, "srand") or not hasattr(libc, "rand") or "musl" in name:
        pytest.skip("not glibc")
    libc.rand.restype = C.c_int
    for seed in (1, 12345, 2 ** 31 - 1):
        libc.srand(C.c_uint(seed))
        want = [libc.rand() for _ in range(1000)]
        g = S.Rand(S.RNG_GLIBC, seed)
        assert [g.next() for _ in range(1000)] == want, seed


def test_get_random_index_is_in_range():
    for kind in (S.RNG_GLIBC, S.RNG_MSVC):
        g = S.Rand(kind, 7)
        v = [g.index(446) for _ in range(5000)]
        assert min(v) >= 0 and max(v) <= 445 and len(set(v)) > 400


def test_default_threshold_is_infinite():
    with np.errstate(over="ignore"):
        assert np.float32(np.sqrt(np.finfo(np.float64).max)) == np.inf
    assert S.threshold(np.sqrt(S.DBL_MAX)) == np.inf and S.threshold(0.25) == f32(0.25)


def test_identity_tolerance_of_the_guess():
    g = np.eye(4, dtype=f32)
    assert S.guess_is_identity(g)
    g[0, 3] = 0.019
    assert S.guess_is_identity(g)      # 0.019^2 <= 1e-4 * 4
    g[0, 3] = 0.021
    assert not S.guess_is_identity(g)


# ---- the fixture --------------------------------------------------------------------------------
def test_fixture_inputs_are_the_cases(golden):
    z, meta = golden
    assert list(meta) == S.CASE_NAMES
    base = load_case(golden, "default")
    cases = S.build_cases(base["fs"], base["ft"])  # (the descriptors: fpfh_ref's, kept as inputs)
    for name, case in cases.items():
        got = load_case(golden, name)
        for k in ("src", "fs", "tgt", "ft", "guess"):
            assert (k in case) == (k in got), (name, k)
            if k in case:
                a, b = np.asarray(case[k], f32), np.asarray(got[k], f32)
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), (name, k)
        assert {k: case[k] for k in S.ALIGN_KEYS if k in case} == meta[name]["args"], name
    assert len(base["src"]) == 446 and len(base["tgt"]) == 545
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "sac_ia_small.npz")) < 1 << 20


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_fixture_equals_the_restatement(golden, reruns, name):
    z, meta = golden
    r = reruns(name)
    assert same_floats(r["final"], z[name + "/final"])
    assert same_floats(r["aligned"], z[name + "/aligned"])
    for k, v in S.hypothesis_arrays(r).items():
        want = z[f"{name}/{k}"]
        assert same_floats(v, want) if k == "T" else np.array_equal(v, want), (name, k)
    for k in SCALARS:
        assert r[k] == meta[name][k], (name, k)
    assert str(r["E"]) == meta[name]["E"]


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_the_cases_reach_their_paths(golden, reruns, name):
    S.check_paths(name, load_case(golden, name), reruns(name))


def test_the_draws_do_not_depend_on_the_descriptors(golden):
    """every iteration's samples and ranks replay from the source coordinates alone"""
    case = load_case(golden, "finite_threshold")
    r = S.run_case(dict(case, fs=case["fs"][::-1].copy(), max_iterations=25))
    z, _ = golden
    for k in ("sample", "rank", "draws"):
        assert np.array_equal(S.hypothesis_arrays(r)[k], z[f"finite_threshold/{k}"][:25])


def test_error_is_an_exact_integer_of_any_order(golden):
    case = load_case(golden, "finite_threshold")
    z, _ = golden
    T = z["finite_threshold/T"][65].reshape(4, 4)
    tv = case["tgt"][S.valid_target(case["tgt"], case["ft"])]
    thr = S.threshold(case["max_correspondence_distance"])
    E, far, used = S.error_metric(T, case["src"], tv, thr)
    E2, far2, used2 = S.error_metric(T, case["src"][::-1], tv[::-1], thr)
    assert (E, far, used) == (E2, far2, used2)
    assert E == (int(z["finite_threshold/err_hi"][65]) << 24) + int(z["finite_threshold/err_lo"][65])


# ---- sacia_model.hpp on the host, under the sanitizers -----------------------------------------
@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ssan") / "sacia_model_san")
    subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "dialog_amd/csrc"), "-I",
                    os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests/cpp/sacia_model_san.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_model_header_against_the_fixture(model_exe, golden, tmp_path, name):
    z, meta = golden
    case = load_case(golden, name)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    guess = np.asarray(case.get("guess", np.eye(4)), f32)
    with open(src, "wb") as f:
        f.write(np.array([len(case["src"]), len(case["tgt"]), case["max_iterations"],
                          case.get("nr_samples", 3), case.get("k_correspondences", 10),
                          case.get("rng", 0), case.get("seed", 1), int("guess" in case)],
                         np.int32).tobytes())
        f.write(f32(case.get("min_sample_distance", 0.0)).tobytes())
        f.write(np.float64(case.get("max_correspondence_distance", np.sqrt(S.DBL_MAX))).tobytes())
        for k in ("src", "fs", "tgt", "ft"):
            f.write(np.ascontiguousarray(case[k], f32).tobytes())
        f.write(guess.tobytes())
    r = subprocess.run([model_exe, src, dst], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(dst, "rb").read()
    n_rec, converged, best = np.frombuffer(raw, np.int32, 3)
    final = np.frombuffer(raw, f32, 16, 12)
    hi, lo = (int(v) for v in np.frombuffer(raw, np.uint64, 2, 76))
    err = float(np.frombuffer(raw, np.float64, 1, 92)[0])
    m = meta[name]
    assert n_rec == len(z[name + "/valid"])
    assert (converged, best) == (m["converged"], m["best_iteration"])
    assert same_floats(final, z[name + "/final"].reshape(16))
    assert (hi << 24) + lo == int(m["E"]) and err == m["error"]
    size = C.sizeof(_lib.SacIaHypothesis)
    assert len(raw) == 100 + size * n_rec
    for it in range(n_rec):
        h = _lib.SacIaHypothesis.from_buffer_copy(raw, 100 + size * it)
        for k in ("sample", "match", "rank"):
            assert list(getattr(h, k)) == z[f"{name}/{k}"][it].tolist(), (name, it, k)
        for k in ("valid", "relaxations", "draws", "n_far", "n_used", "err_hi", "err_lo"):
            assert int(getattr(h, k)) == int(z[f"{name}/{k}"][it]), (name, it, k)
        assert same_floats(np.array(h.T, f32), z[name + "/T"][it]), (name, it)


# ---- shim, ABI ---------------------------------------------------------------------------------
def test_cpp_sac_ia_shim_compiles_and_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "shim_sac_ia.cpp")
    exe = tmp_path / "shim_sac_ia"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o",
           str(exe), "-L", os.path.dirname(_lib.LIB_PATH), "-ldialog_amd",
           f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_sac_ia_struct_layouts_match_the_header():
    L = _lib.load()
    assert L.dlg_abi_struct_size(19) == C.sizeof(_lib.SacIaParams) == 56
    assert L.dlg_abi_struct_size(20) == C.sizeof(_lib.SacIaHypothesis) == 208
    assert L.dlg_abi_struct_size(21) == C.sizeof(_lib.SacIaStats) == 112
    assert L.dlg_abi_struct_size(22) == -1
    assert L.dlg_abi_version() == 5 == _lib.ABI_VERSION
    for s in ("dlg_sac_ia_params_default", "dlg_fpfh_knn", "dlg_sac_ia_score", "dlg_sac_ia_align"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    import dialog_amd as D
    assert callable(D.sac_ia_align) and callable(D.sac_ia_score) and callable(D.fpfh_knn)


def test_params_default_is_pcl_s():
    p = _lib.SacIaParams()
    _lib.load().dlg_sac_ia_params_default(C.byref(p))
    assert (p.max_iterations, p.nr_samples, p.k_correspondences, p.rng, p.seed) == (1000, 3, 10, 0, 1)
    assert (p.compute_fitness, p.batch, p.max_blocks, p.min_sample_distance) == (0, 0, 0, 0.0)
    assert p.max_correspondence_distance == np.sqrt(S.DBL_MAX) and p.fitness_max_range == S.DBL_MAX


def test_null_handles_are_invalid_without_a_device():
    """the argument checks that need no context (the rest: tests/test_sac_ia_gpu.py)"""
    L = _lib.load()
    p = _lib.SacIaParams()
    L.dlg_sac_ia_params_default(C.byref(p))
    assert L.dlg_fpfh_knn(None, None, 132, 0, None, 132, 0, 1, None, None) == _lib.DLG_ERR_INVALID
    assert L.dlg_sac_ia_score(None, None, None, None, 0, 1.0, 0, 0, None) == _lib.DLG_ERR_INVALID
    assert L.dlg_sac_ia_align(None, None, None, 132, None, None, 132, C.byref(p), None, None, None,
                              12, None, 0, None) == _lib.DLG_ERR_INVALID
