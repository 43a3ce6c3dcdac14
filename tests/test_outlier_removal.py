"""CPU: the statistical outlier filter's reference (tests/sor_ref.py) on the fixtures' figures and
edge cases, sor_model.hpp's host side under ASan + UBSan against the reference, the C++ shim, and
the ABI structs.  The device path is tests/test_outlier_removal_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sor_ref as S
from dialog_amd import _lib, pcd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
f32 = np.float32


@pytest.fixture(scope="module")
def shadow():
    return np.ascontiguousarray(
        pcd.read_pcd(os.path.join(ROOT, "tests", "golden", "double_shadow.pcd"))[:, :3], f32)


@pytest.fixture(scope="module")
def cluster():
    A = S.cluster_cloud()
    return A, {k: S.sor_ref(A, k, 1.0) for k in (20, 100)}


# ---- the fixtures' figures ------------------------------------------------------------------------
@pytest.mark.parametrize("mean_k,mul,removed,threshold", [
    (8, 1.0, 148, 0.01019383551886305), (50, 1.0, 133, 0.021751963317590422),
    (63, 0.5, 190, None), (150, 1.0, 122, None), (255, 1.0, 116, None)])
def test_double_shadow_figures(shadow, mean_k, mul, removed, threshold):
    assert len(shadow) == 991
    r = S.sor_ref(shadow, mean_k, mul)
    assert len(r["removed"]) == removed and len(r["kept"]) == 991 - removed
    assert r["n_finite"] == r["n_valid"] == 991
    if threshold is not None:
        assert r["threshold"] == threshold


def test_cluster_figures(cluster):
    """mean_k 20: both statistics certificates fail; mean_k 100: 36 per-query certificates fail,
    the statistics certify, and the descending sequential chain changes 29 of the double sums, all
    among the 36, but none of the float distances.  (The issue's prototype counted 14: that is
    what numpy's pairwise np.sum over the reversed terms gives against the ascending chain, not a
    descending chain)"""
    A, refs = cluster
    assert len(refs[20]["removed"]) == 864 and len(refs[100]["removed"]) == 730
    d = refs[20]["distances"]
    assert not S.certificate(d)[0] and not S.certificate((d * d).astype(f32))[0]
    t20 = np.sqrt(refs[20]["d2"]).astype(f32)
    assert all(S.certificate(t)[0] for t in t20)
    d = refs[100]["distances"]
    assert S.certificate(d)[0] and S.certificate((d * d).astype(f32))[0]
    terms = np.sqrt(refs[100]["d2"]).astype(f32)
    fails = np.array([not S.certificate(t)[0] for t in terms])
    assert fails.sum() == 36
    asc, desc = S.seq_sum(terms), S.seq_sum(terms, "desc")
    differ = asc.view(np.uint64) != desc.view(np.uint64)
    assert differ.sum() == 29 and not differ[~fails].any()
    w = S.sor_ref(A, 100, 1.0, order="desc")
    assert np.array_equal(w["distances"].view(np.uint32), d.view(np.uint32))
    # where the certificate holds the order cannot matter, and the sum is the exact one
    for t, a, b in zip(terms, asc, desc):
        ok, exact = S.certificate(t)
        if ok:
            assert a == b == exact
    # sqrt in double is a different filter
    w = S.sor_ref(A, 100, 1.0, sqrt_double=True)
    assert (w["distances"].view(np.uint32) != d.view(np.uint32)).any()


def test_reference_against_characterisation(shadow):
    """distances within float rounding of a float64 evaluation; the partition is the threshold's"""
    r = S.sor_ref(shadow, 8, 1.0)
    p = shadow.astype(np.float64)
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(2))
    want = np.sort(d, axis=1)[:, 1:9].mean(1)
    assert np.abs(r["distances"] - want).max() <= 4 * 2.0**-23 * want.max()
    assert np.array_equal(r["removed"], np.nonzero(r["distances"].astype(np.float64) > r["threshold"])[0])
    assert np.array_equal(np.sort(np.concatenate([r["kept"], r["removed"]])), np.arange(991))


# ---- edge cases of the reference --------------------------------------------------------------
def test_identical_points():
    p = np.full((300, 3), 1.25, f32)
    r = S.sor_ref(p, 10, 1.0)
    assert r["threshold"] == 0.0 and len(r["removed"]) == 0 and (r["distances"] == 0).all()


def test_one_entry_list(shadow):
    r = S.sor_ref(shadow, 8, 1.0, idx=[17])
    assert not np.isfinite(r["threshold"])
    assert list(r["kept"]) == [17] and len(r["removed"]) == 0 and r["n_valid"] == 1


def test_nan_point_kept_or_removed(shadow):
    p = shadow.copy()
    p[5, 1] = np.nan
    r = S.sor_ref(p, 8, 1.0)
    assert r["n_finite"] == 990 and r["n_valid"] == 990 and r["distances"][5] == 0
    assert 5 in r["kept"]
    r = S.sor_ref(p, 8, -100.0)
    assert r["threshold"] < 0 and 5 in r["removed"]


def test_negative_and_index_lists(shadow):
    a = S.sor_ref(shadow, 8, 1.0)
    b = S.sor_ref(shadow, 8, 1.0, negative=True)
    assert np.array_equal(a["kept"], b["removed"]) and np.array_equal(a["removed"], b["kept"])
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 991, 1500)  # (duplicated and permuted)
    r = S.sor_ref(shadow, 8, 1.0, idx=idx)
    # the distances do not depend on the list: the search is over the whole cloud
    assert np.array_equal(r["distances"].view(np.uint32), a["distances"][idx].view(np.uint32))
    assert np.array_equal(np.sort(np.concatenate([r["kept"], r["removed"]])), np.sort(idx))
    rm = r["distances"].astype(np.float64) > r["threshold"]
    assert np.array_equal(r["removed"], idx[rm]) and np.array_equal(r["kept"], idx[~rm])
    with pytest.raises(S.TooFewPoints):
        S.sor_ref(shadow[:8], 8, 1.0)


# ---- sor_model.hpp on the host, under the sanitizers ------------------------------------------
@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ssan") / "sor_model_san")
    subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "dialog_amd/csrc"),
                    os.path.join(ROOT, "tests/cpp/sor_model_san.cpp"), "-o", exe], check=True)
    return exe


def run_model(exe, lists, mul=1.0):
    lines = [f"{len(t)} {float(mul).hex()} " + " ".join(float(v).hex() for v in t) for t in lists]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       env=ENV, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 3 * len(lists)
    return [(rows[3 * i], rows[3 * i + 1], rows[3 * i + 2]) for i in range(len(lists))]


def bits(x):
    return np.float64(x).view(np.uint64)


def check_lists(exe, lists, mul=1.0):
    verdicts = []
    for t, (cert, sums, stats) in zip(lists, run_model(exe, lists, mul)):
        t = np.asarray(t, f32)
        ok, exact = S.certificate(t)
        assert cert[0] == "cert" and int(cert[1]) == int(ok)
        lit = np.cumsum(t.astype(np.float64))[-1] if len(t) else np.float64(0)
        assert bits(float.fromhex(sums[1])) == bits(lit)
        if ok:  # the tree sum and units * 2^q are the literal sum's bits
            assert bits(float.fromhex(sums[2])) == bits(lit) == bits(exact)
            assert bits(float.fromhex(sums[3])) == bits(lit)
            assert float(int(cert[3])) * 2.0 ** int(cert[2]) == exact
        # the statistics and the threshold, as sor_ref computes them
        with np.errstate(all="ignore"):
            sq = (t * t).astype(f32)
            sq_sum = np.cumsum(sq.astype(np.float64))[-1] if len(t) else np.float64(0)
            nv = np.float64(len(t))
            mean = lit / nv
            sd = np.sqrt((sq_sum - lit * lit / nv) / (nv - np.float64(1)))
            thr = mean + np.float64(mul) * sd
        got = [float.fromhex(v) for v in stats[1:]]
        for g, wnt in zip(got, (lit, sq_sum, mean, sd, thr)):
            assert bits(g) == bits(wnt) or (np.isnan(g) and np.isnan(wnt))
        verdicts.append(ok)
    return verdicts


def test_model_header_certificate_and_sums(model_exe, cluster):
    A, refs = cluster
    terms = np.sqrt(refs[100]["d2"]).astype(f32)
    v = check_lists(model_exe, list(terms))
    assert sum(not x for x in v) == 36
    # the two statistics lists of both settings
    for k, want in ((20, False), (100, True)):
        d = refs[k]["distances"]
        assert check_lists(model_exe, [d], mul=1.0) == [want]


def test_model_header_built_lists(model_exe):
    rng = np.random.default_rng(7)
    # terms spanning 2^-30 .. 1, the two extremes with their lowest bits set: the unit is
    # 2^-53, in which the term near 1 alone is 2^53 - 2^29... and the rest lift the sum past 2^53
    ends = [np.float32(1 - 2.0**-24), np.float32((1 + 2.0**-23) * 2.0**-30), np.float32(0.75)]
    wide = [np.concatenate([(rng.uniform(0.5, 1, 50) * 2.0 ** rng.integers(-30, 1, 50)), ends])
            .astype(f32)[rng.permutation(53)] for _ in range(20)]
    v = check_lists(model_exe, wide, mul=0.5)
    assert not any(v)
    narrow = [rng.uniform(0.5, 1, 200).astype(f32) for _ in range(5)]
    assert all(check_lists(model_exe, narrow, mul=-2.0))
    zeros = [np.zeros(k, f32) for k in (1, 2, 50)]
    assert all(check_lists(model_exe, zeros))
    assert all(check_lists(model_exe, [np.array([0, 0, 3e-41, 0, 1e-39], f32)]))  # denormals
    assert check_lists(model_exe, [np.array([1, np.inf], f32)]) == [False]
    assert check_lists(model_exe, [np.array([], f32), np.array([0.75], f32)]) == [True, True]
    # the boundary: 2^29 + ... units of 2^-23 stay below 2^53; one more power of two does not
    assert check_lists(model_exe, [np.array([2.0**28, 1 + 2.0**-23], f32)]) == [True]
    assert check_lists(model_exe, [np.array([2.0**30, 1 + 2.0**-23], f32)]) == [False]
    # odd parts of several bits shifted far: term / unit must be refused at 2^53 by its bit
    # length, not after a 64-bit shift that has already dropped the high bits (4097 * 2^52 and
    # 0x8007ff * 2^41 both wrap to a value below 2^53)
    assert check_lists(model_exe, [np.array([4097 * 2.0**40, 2.0**-12], f32)]) == [False]
    assert check_lists(model_exe, [np.array([0x8007ff, 2.0**-41, 0x8007ff], f32)]) == [False]
    assert check_lists(model_exe, [np.array([3 * 2.0**49, 0.5], f32)]) == [True]   # 3 * 2^50 + 1
    assert check_lists(model_exe, [np.array([7 * 2.0**50, 0.5], f32)]) == [False]  # 7 * 2^51
    assert check_lists(model_exe, [np.array([(2**24 - 1) * 2.0**5, 2.0**-24], f32)]) == [True]
    assert check_lists(model_exe, [np.array([(2**24 - 1) * 2.0**6, 2.0**-24], f32)]) == [False]
    # a sweep: random odd 24-bit significands at every shift 2..37 against the unit 1.0 (term /
    # unit reaches 2^53 from shift 30)
    sweep = [np.array([float(int(s) | 1 | 2**23) * 2.0**int(k), 1.0], f32)
             for k in range(2, 38) for s in rng.integers(2**23, 2**24, 4)]
    v = check_lists(model_exe, sweep)
    assert any(v) and not all(v)


# ---- shim, ABI ---------------------------------------------------------------------------------
def test_cpp_sor_shim_compiles_and_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "shim_sor.cpp")
    exe = tmp_path / "shim_sor"
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", str(exe),
           "-L", os.path.dirname(_lib.LIB_PATH), "-ldialog_amd",
           f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_sor_struct_layouts_match_the_header():
    L = _lib.load()
    assert L.dlg_abi_struct_size(8) == C.sizeof(_lib.SorParams) == 16
    assert L.dlg_abi_struct_size(9) == C.sizeof(_lib.SorStats) == 80
    assert _lib.DLG_OPT_SOR_LITERAL == 25
    for s in ("dlg_statistical_outlier_removal", "dlg_statistical_outlier_removal_cloud"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
