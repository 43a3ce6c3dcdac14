"""The rigid registration without a GPU: tests/golden/icp_small.npz against a recomputation by
tests/icp_ref.py, the host side of dialog_amd/csrc/icp_model.hpp (a stand-alone program under
-fsanitize=address,undefined) bit-equal to the restatement on every case's moments -> T -> criteria
chain, the Horn solve against a float64 SVD, the order-independence of the sums, the recovered
motion, the ABI and the C++ shim; the fast exact reference (icp_ref.correspondences_fast) against
the brute force, and what each generated input of the device tests (scatter, the scale ladder, the
degenerate clouds, the contract cases) is for."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import icp_ref as R
from dialog_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
f32 = np.float32

# Measured with the restatement on every iteration of every case (test_horn_against_svd prints it):
# the worst entry difference between the solve's R | t in double and a float64 np.linalg.svd
# Umeyama is 2.55e-11 (the `big` case, coordinates near 8192); the bound is 100 x that, and has to
# stay below 1e-6, the resolution of the float output.
HORN_SVD_MEASURED = 2.6e-11
HORN_SVD_BOUND = 100 * HORN_SVD_MEASURED
# Measured with the restatement on `shadow_moved` (5 degrees about z plus (0.01, 0, 0)):
# final . motion differs from the identity by 6.44e-8 rad and 2.66e-8 in translation; the bounds
# are twice those.
MOTION_ROT_MEASURED, MOTION_TRANS_MEASURED = 6.44e-8, 2.66e-8


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def dbits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "icp_small.npz"))
    return z, json.loads(str(z["meta"]))


@pytest.fixture(scope="module")
def cases():
    return R.build_cases()


@pytest.fixture(scope="module")
def results(cases):
    """every case through the restatement, computed once (with each iteration's pairs)"""
    return {name: R.run_case(c, keep_pairs=True) for name, c in cases.items()}


# ---- the fixture -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_fixture_equals_the_recomputation(golden, cases, results, name):
    z, meta = golden
    c, r = cases[name], results[name]
    assert np.array_equal(bits(z[f"{name}/src"]), bits(c["src"]))
    assert np.array_equal(bits(z[f"{name}/tgt"]), bits(c["tgt"]))
    n_corr, mse, ee, T = R.history_arrays(r)
    assert (meta[name]["state"], meta[name]["iterations"], meta[name]["converged"]) == \
        (r["state"], r["iterations"], r["converged"])
    assert np.array_equal(z[f"{name}/n_corr"], n_corr) and np.array_equal(z[f"{name}/e"], ee)
    assert np.array_equal(dbits(z[f"{name}/mse"]), dbits(mse))
    assert np.array_equal(bits(z[f"{name}/T"]), bits(T))
    assert np.array_equal(bits(z[f"{name}/final"]), bits(r["final"]))
    assert np.array_equal(bits(z[f"{name}/aligned"]), bits(r["aligned"]))
    assert dbits(z[f"{name}/fitness"])[0] == dbits(r["fitness"])[0]


def test_the_cases_cover_what_they_are_for(golden, cases, results):
    z, meta = golden
    assert len(cases["shadow"]["src"]) == 446 and len(cases["shadow"]["tgt"]) == 545
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "icp_small.npz")) < (1 << 20)
    # shadow_maxdist drops part of the first iteration's pairs: between 20 % and 80 % kept
    k = results["shadow_maxdist"]["history"][0]["n_corr"]
    assert 0.2 * 446 <= k <= 0.8 * 446
    assert results["planes_mse"]["state"] in (R.ABS_MSE, R.REL_MSE)
    assert results["planes_iter"]["state"] == R.ITERATIONS
    assert len(cases["planes_iter"]["src"]) == 5000 and len(cases["planes_iter"]["tgt"]) == 7000
    # far: every source point outside the target's box
    s, t = cases["far"]["src"], cases["far"]["tgt"]
    assert (s.min(axis=0) > t.max(axis=0)).all()
    # ties: the first iteration pairs every centre with the lowest of its 8 equidistant corners
    nn, d2 = R.correspondences(cases["ties"]["src"], cases["ties"]["tgt"])
    corner = (cases["ties"]["src"] - f32(0.5)).astype(np.int64)
    assert np.array_equal(nn, (corner[:, 0] * 6 + corner[:, 1]) * 6 + corner[:, 2])
    assert (d2 == f32(0.75)).all()
    # big: e changes between iterations
    assert len({h["e"] for h in results["big"]["history"]}) > 1
    idx = cases["shadow_dups"]["indices"]
    assert len(np.unique(idx)) < len(idx)
    assert not np.isfinite(cases["nonfinite"]["src"]).all()
    assert not np.isfinite(cases["nonfinite"]["tgt"]).all()
    assert results["nonfinite"]["history"][0]["n_corr"] == 446 - 3
    assert results["shadow_guess"]["iterations"] > 0 and "guess" in cases["shadow_guess"]


def test_recovered_motion(golden):
    """shadow_moved is shadow's source moved by a known rigid motion: the registration undoes it"""
    z, _ = golden
    rot, trans = R.motion_error(z["shadow_moved/final"], R.rigid(**R.SHADOW_MOTION))
    print("recovered motion: rotation error", rot, "rad, translation error", trans)
    assert rot <= 2 * MOTION_ROT_MEASURED and trans <= 2 * MOTION_TRANS_MEASURED


def test_horn_against_svd(results):
    worst = 0.0
    for name, r in results.items():
        for (w, t, d2), h in zip(r["pairs"], r["history"]):
            mo = R.moments(w, t, d2, h["e"], h["e2"])
            d = float(np.abs(R.solve_double(mo, h["e"]) - R.umeyama_svd(w, t)).max())
            worst = max(worst, d)
            assert d <= HORN_SVD_BOUND, (name, d)
    print("Horn against SVD: worst entry difference", worst)
    assert HORN_SVD_BOUND <= 1e-6
    # the solve always yields a proper rotation, also for a reflected and for a degenerate set
    for M in ([[1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0]], [[0.0] * 3] * 3, [[2.0, 0, 0], [0, 0, 0], [0, 0, 0]]):
        Rm = np.array(R.horn(M))
        assert abs(np.linalg.det(Rm) - 1.0) < 1e-12 and np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-12)


# ---- the fast reference and the generated inputs ------------------------------------------------------
@pytest.fixture(scope="module")
def scatter():
    c = R.scatter_case()
    c["nn"], c["d2"] = R.correspondences(c["src"], c["tgt"])
    return c


def same_pairs(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def test_fast_reference_equals_brute_force(cases, scatter):
    """correspondences_fast against correspondences, bit for bit in nn and d2, on every golden case,
    on the scatter case (with and without a max_dist) and on the ties lattice, which has to come out
    through the fallback"""
    for name, c in cases.items():
        W = c["src"] if "indices" not in c else c["src"][c["indices"]]
        md = c.get("max_dist", R.DBL_MAX ** 0.5)
        info = {}
        assert same_pairs(R.correspondences_fast(W, c["tgt"], md, info=info),
                          R.correspondences(W, c["tgt"], md)), name
        assert info["queries"] == int(np.isfinite(W).all(axis=1).sum())
        if name == "ties":  # 8 equidistant corners: the 4th candidate is no farther than the 1st
            assert info["uncertified"] == info["queries"] == 125
        else:
            assert info["uncertified"] <= 0.01 * info["queries"], name
    md = float(np.median(scatter["d2"][scatter["nn"] >= 0].astype(np.float64))) ** 0.5
    for m in (R.DBL_MAX ** 0.5, md):
        info = {}
        assert same_pairs(R.correspondences_fast(scatter["src"], scatter["tgt"], m, info=info),
                          R.correspondences(scatter["src"], scatter["tgt"], m))
        assert info["uncertified"] <= 0.01 * info["queries"]
    # fewer target points than candidates, and subnormal d2 (below the certificate's floor)
    few = cases["shadow"]["tgt"][:3]
    assert same_pairs(R.correspondences_fast(cases["shadow"]["src"], few),
                      R.correspondences(cases["shadow"]["src"], few))
    tiny = R.scaled_case(cases["shadow_moved"], -60)
    info = {}
    assert same_pairs(R.correspondences_fast(tiny["src"], tiny["tgt"], info=info),
                      R.correspondences(tiny["src"], tiny["tgt"]))
    assert info["uncertified"] == info["queries"]
    # the loop on the fast function: the same bits as the loop on the brute force
    a = R.run_case(cases["shadow_maxdist"], fast=True)
    b = R.run_case(cases["shadow_maxdist"])
    assert np.array_equal(bits(a["final"]), bits(b["final"])) and a["fitness"] == b["fitness"]
    assert np.array_equal(bits(a["aligned"]), bits(b["aligned"]))


def test_scatter_is_what_it_is_for(scatter):
    src, nn, d2 = scatter["src"], scatter["nn"], scatter["d2"]
    assert len(src) % 256 != 0 and 2900 <= len(src) <= 3100 and 2900 <= len(scatter["tgt"]) <= 3100
    fin = np.isfinite(src).all(axis=1)
    assert 0 < (~fin).sum() <= 16 and np.array_equal(nn >= 0, fin)
    # every workgroup of 256 holds entries of every part of the ladder (and so of every level)
    d = np.sqrt(d2.astype(np.float64)) / scatter["spacing"]
    for a in range(0, len(src), 256):
        blk = d[a:a + 256][fin[a:a + 256]]
        assert (blk < 2).any() and ((blk > 8) & (blk < 64)).any() and (blk > 256).any(), a
    md = float(np.median(d2[fin].astype(np.float64))) ** 0.5
    kn, kd = R.correspondences(src, scatter["tgt"], md)
    kept = kd[kn >= 0].astype(np.float64)
    assert 0.2 * len(src) <= len(kept) <= 0.8 * len(src)
    lo, hi = np.percentile(kept, 10), np.percentile(kept, 90)
    print("scatter: kept", len(kept), "of", len(src), "d2 p90 / p10 = 2^%.2f" % np.log2(hi / lo))
    assert hi >= lo * 2.0 ** 16


def test_transformation_epsilon_ends_by_transform(cases):
    c = cases["shadow_moved"]
    r = R.align(c["src"], c["tgt"], transformation_epsilon=1e-5)
    assert (r["state"], r["iterations"], r["converged"]) == (R.TRANSFORM, 5, 1)
    assert R.align(c["src"], c["tgt"])["iterations"] == 7


def test_fitness_range(cases, results):
    """getFitnessScore keeps d2 <= max_range: a NaN or a negative range keeps nothing (DBL_MAX), the
    median of the final pass's d2 keeps between 20 % and 80 %"""
    c, r = cases["shadow_moved"], results["shadow_moved"]
    W, tgt = r["aligned"], c["tgt"]
    assert R.fitness_score(W, tgt, float("nan")) == R.DBL_MAX
    assert R.fitness_score(W, tgt, -1.0) == R.DBL_MAX
    assert R.fitness_score(W, tgt, R.DBL_MAX) == r["fitness"] < 1e-3
    nn, d2 = R.correspondences(W, tgt)
    mr = float(np.median(d2.astype(np.float64)))
    k = d2.astype(np.float64) <= mr
    assert 0.2 * len(W) <= k.sum() <= 0.8 * len(W)
    f = R.fitness_score(W, tgt, mr)
    assert 0.0 < f < r["fitness"]
    assert f == R.align(c["src"], tgt, fitness_max_range=mr)["fitness"]
    # the sum as the mse's: exact integers of the kept d2 at their own exponent
    e2 = R.qexp(d2[k].max())
    assert f == float(int(R.quantise(d2[k], e2).sum())) / float(int(k.sum())) * 2.0 ** (e2 - 48)


def test_scale_ladder_is_what_it_is_for(cases):
    base = cases["shadow_moved"]
    tiny = float(np.finfo(f32).tiny)
    for k in R.SCALE_RUNGS:
        c = R.scaled_case(base, k)
        assert np.array_equal(np.ldexp(c["src"].astype(np.float64), -k), base["src"])  # exact
        nn, d2 = R.correspondences(c["src"], c["tgt"])
        assert (nn >= 0).all() and np.isfinite(d2).all()
        if k == -70:
            assert (d2 == 0).all()
        if k == -60:
            assert ((d2 > 0) & (d2 < tiny)).any()
        if k == 60:
            assert d2.max() < np.finfo(f32).max and d2.min() > 0
    # upward the runs are the unscaled run scaled exactly
    r0, r60 = R.align(base["src"], base["tgt"], max_iterations=4), \
        R.align(**R.scaled_case(base, 60), max_iterations=4)
    assert np.array_equal(bits(np.ldexp(r0["aligned"], 60)), bits(r60["aligned"]))
    assert np.array_equal(bits(r0["final"][:3, :3]), bits(r60["final"][:3, :3]))


def test_degenerate_clouds_are_degenerate():
    d = R.degenerate_cases()
    p, ln = d["plane"], d["line"]
    assert (bits(p["tgt"][:, 2]) == bits(f32(0.25))).all() and (bits(p["src"][:, 2]) == bits(f32(0.26))).all()
    assert (bits(ln["tgt"][:, 1:]) == 0).all() and np.abs(ln["src"][:, 1:]).max() > 0
    for c in (p, ln):
        assert 200 <= len(c["src"]) <= 500 and 200 <= len(c["tgt"]) <= 500
    # the plane pair: a rank-deficient M (every pair has the same z on each side)
    r = R.align(p["src"], p["tgt"], max_iterations=1, keep_pairs=True)
    (w, t, d2), h = r["pairs"][0], r["history"][0]
    M = np.array(R.rounded_moments(R.moments(w, t, d2, h["e"], h["e2"])))
    assert (M[2] == 0).all() and (M[:, 2] == 0).all()


# ---- the model header --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("isan") / "icp_model_san")
    subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "dialog_amd/csrc"),
                    os.path.join(ROOT, "tests", "cpp", "icp_model_san.cpp"), "-o", exe], check=True)
    return exe


def run_model(exe, blocks):
    """blocks: ("C", max_iterations, teps, feps) or ("I", w, t, d2, e, e2, group, reverse) ->
    per iteration dict(ints, T (uint32 [16]), mse (uint64), state)"""
    lines = []
    for b in blocks:
        if b[0] == "C":
            lines.append(f"C {b[1]} {b[2]!r} {b[3]!r}")
            continue
        _, w, t, d2, e, e2, group, reverse = b
        lines.append(f"I {len(w)} {e} {e2} {group} {reverse}")
        rows = np.concatenate([w, t, d2[:, None]], axis=1).astype(f32).view(np.uint32)
        lines += [" ".join("%x" % v for v in row) for row in rows]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       env=ENV, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    o = r.stdout.splitlines()
    out = []
    for k in range(0, len(o), 4):
        ints = o[k].split()[1:]
        big = [int(x, 16) for x in ints[1:]]
        out.append(dict(ints=[int(ints[0])] + [v - (1 << 192) if v >> 191 else v for v in big],
                        T=np.array([int(x, 16) for x in o[k + 1].split()[1:]], np.uint32),
                        mse=int(o[k + 2].split()[1], 16), state=int(o[k + 3].split()[1])))
    return out


def expected_ints(mo):
    return [mo["m"]] + mo["S"] + mo["T"] + [mo["P"][a][b] for a in range(3) for b in range(3)] + \
        [mo["D"]]


def test_model_header_against_the_restatement(model_exe, cases, results):
    """every case's chain: the pairs' exact integers, T, mse and the criteria's state"""
    blocks, want = [], []
    for name in R.CASE_NAMES:
        c, r = cases[name], results[name]
        blocks.append(("C", c.get("max_iterations", 10), c.get("transformation_epsilon", 0.0),
                       c.get("euclidean_fitness_epsilon", -R.DBL_MAX)))
        for k, ((w, t, d2), h) in enumerate(zip(r["pairs"], r["history"])):
            blocks.append(("I", w, t, d2, h["e"], h["e2"], R_FLUSH, 0))
            last = k == len(r["history"]) - 1
            want.append((name, k, expected_ints(R.moments(w, t, d2, h["e"], h["e2"])), h,
                         r["state"] if last else R.NOT_CONVERGED))
    got = run_model(model_exe, blocks)
    assert len(got) == len(want)
    for g, (name, k, ints, h, state) in zip(got, want):
        assert g["ints"] == ints, (name, k)
        assert np.array_equal(g["T"], bits(h["T"]).reshape(16)), (name, k)
        assert g["mse"] == int(dbits(h["mse"])[0]) and g["state"] == state, (name, k)


R_FLUSH = 16  # kIcpFlush


def test_sums_do_not_depend_on_order_or_grouping(model_exe, results):
    r = results["planes_iter"]
    (w, t, d2), h = r["pairs"][0], r["history"][0]
    ints = expected_ints(R.moments(w, t, d2, h["e"], h["e2"]))
    perm = np.random.default_rng(5).permutation(len(w))
    assert expected_ints(R.moments(w[perm], t[perm], d2[perm], h["e"], h["e2"])) == ints
    blocks = [("C", 10, 0.0, -R.DBL_MAX)]
    for group, reverse, order in ((1, 0, None), (7, 0, None), (16, 1, None), (16, 0, perm),
                                  (3, 1, perm)):
        o = slice(None) if order is None else order
        blocks.append(("I", w[o], t[o], d2[o], h["e"], h["e2"], group, reverse))
    got = run_model(model_exe, blocks)
    for g in got:
        assert g["ints"] == ints
        assert np.array_equal(g["T"], bits(h["T"]).reshape(16)) and g["mse"] == int(dbits(h["mse"])[0])


# ---- shim, ABI ---------------------------------------------------------------------------------------
def test_cpp_icp_shim_compiles_and_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "shim_icp.cpp")
    exe = tmp_path / "shim_icp"
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", str(exe),
           "-L", os.path.dirname(_lib.LIB_PATH), "-ldialog_amd",
           f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_icp_struct_layouts_match_the_header():
    L = _lib.load()
    assert L.dlg_abi_struct_size(13) == C.sizeof(_lib.IcpParams) == 40
    assert L.dlg_abi_struct_size(14) == C.sizeof(_lib.IcpStats) == 80
    assert L.dlg_abi_struct_size(15) == C.sizeof(_lib.IcpIteration) == 88
    assert L.dlg_abi_struct_size(16) == -1 and L.dlg_abi_version() == 5
    assert _lib.DLG_OPT_ICP_REVERSED == 26 and _lib.DLG_OPT_ICP_MAX_BLOCKS == 27
    for s in ("dlg_icp_align", "dlg_icp_correspondences", "dlg_icp_params_default"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    p = _lib.IcpParams()
    L.dlg_icp_params_default(C.byref(p))
    assert (p.max_iterations, p.compute_fitness, p.transformation_epsilon) == (10, 0, 0.0)
    assert p.max_correspondence_distance == R.DBL_MAX ** 0.5
    assert p.euclidean_fitness_epsilon == -R.DBL_MAX and p.fitness_max_range == R.DBL_MAX
