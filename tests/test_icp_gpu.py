"""dlg_icp_align / dlg_icp_correspondences on the GPU against tests/icp_ref.py: every bit of the
final transformation, of each iteration's record (n_corr, mse, e, e2, T), of the aligned cloud, the
state, the iteration count and the fitness score (tests/golden/icp_small.npz), the correspondence
kernel on its own, the small sizes around the thresholds (fewer than 3 pairs, the wave), the
refusals, the Python mirror, the C++ shim and the determinism of the sums; under
DLG_OPT_ICP_MAX_BLOCKS the several-entries-per-thread paths of a huge cloud at small shapes (the
in-loop flush, the block-stride trips of every kernel, the deferral queues), the degenerate and the
extremely scaled clouds, the rest of the header's contract, and one run at a production launch
shape against the fast exact reference."""
import ctypes as C
import json
import math
import os
import subprocess
import sys
from contextlib import contextmanager

import numpy as np
import pytest

import dialog_amd as D
import icp_ref as R
from dialog_amd import _lib
from dialog_amd.sac import _f32p, _i32p

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def dbits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "icp_small.npz"))
    return z, json.loads(str(z["meta"]))


def strided(p, stride):
    """the points as records of `stride` bytes (the padding filled with a marker)"""
    p = np.ascontiguousarray(p, f32).reshape(-1, 3)
    a = np.full((max(len(p), 1), stride // 4), 7.5, f32)
    a[:len(p), :3] = p
    return a, _lib.Points(_f32p(a), len(p), stride)


def raw_align(ctx, src, tgt, indices=None, guess=None, max_iterations=10,
              max_dist=math.sqrt(R.DBL_MAX), transformation_epsilon=0.0,
              euclidean_fitness_epsilon=-R.DBL_MAX, fitness_max_range=R.DBL_MAX, fitness=True,
              stride=12, tstride=12, out_stride=12, want_aligned=True, history_cap=None,
              history_len=None, want_history=True, want_stats=True):
    """history_cap: the capacity passed (default: max_iterations); history_len: the records
    allocated (every one prefilled with NaN and n_corr = -1; the whole buffer comes back as
    `hist`); want_history / want_stats False: NULL is passed"""
    L = _lib.load()
    a, ps = strided(src, stride)
    b, pt = strided(tgt, tstride)
    idx = None if indices is None else np.ascontiguousarray(indices, np.int32)
    m = len(src) if idx is None else len(idx)
    prm = _lib.IcpParams()
    L.dlg_icp_params_default(C.byref(prm))
    prm.max_iterations = int(max_iterations)
    prm.compute_fitness = int(fitness)
    prm.max_correspondence_distance = float(max_dist)
    prm.transformation_epsilon = float(transformation_epsilon)
    prm.euclidean_fitness_epsilon = float(euclidean_fitness_epsilon)
    prm.fitness_max_range = float(fitness_max_range)
    g = None if guess is None else np.ascontiguousarray(guess, f32).reshape(16)
    final = np.full(16, np.nan, f32)
    out = np.full((max(m, 1), out_stride // 4), np.nan, f32)
    cap = max(int(max_iterations), 1) if history_cap is None else int(history_cap)
    hist = (_lib.IcpIteration * max(cap, history_len or 0, 1))()
    for h in hist:
        h.n_corr, h.mse, h.e, h.e2 = -1, math.nan, -1, -1
        for k in range(16):
            h.T[k] = math.nan
    st = _lib.IcpStats()
    status = L.dlg_icp_align(ctx.h, C.byref(ps), None if idx is None else _i32p(idx),
                             m if idx is not None else 0, C.byref(pt), C.byref(prm),
                             None if g is None else _f32p(g), _f32p(final),
                             _f32p(out) if want_aligned else None, out_stride,
                             hist if want_history else None, cap,
                             C.byref(st) if want_stats else None)
    k = min(st.iterations, cap) if status == 0 and want_history else 0
    return dict(status=status, final=final.reshape(4, 4), out=out[:m], aligned=out[:m, :3], stats=st,
                hist=hist,
                n_corr=np.array([hist[i].n_corr for i in range(k)], np.int64),
                mse=np.array([hist[i].mse for i in range(k)], np.float64),
                e=np.array([[hist[i].e, hist[i].e2] for i in range(k)], np.int32).reshape(-1, 2),
                T=np.array([list(hist[i].T) for i in range(k)], f32).reshape(-1, 16))


def assert_equals_reference(r, ref):
    """the device call r against icp_ref.align's dict"""
    n_corr, mse, ee, T = R.history_arrays(ref)
    st = r["stats"]
    assert r["status"] == 0
    assert (st.state, st.iterations, st.converged) == (ref["state"], ref["iterations"],
                                                       ref["converged"])
    assert np.array_equal(r["n_corr"], n_corr) and np.array_equal(r["e"], ee)
    assert np.array_equal(bits(r["T"]), bits(T))
    assert np.array_equal(dbits(r["mse"]), dbits(mse))
    assert np.array_equal(bits(r["final"]), bits(ref["final"]))
    assert np.array_equal(bits(r["aligned"]), bits(ref["aligned"]))
    assert dbits(st.fitness)[0] == dbits(ref["fitness"])[0]
    assert st.n_corr == ref["n_corr"]


def golden_ref(z, meta, name):
    h = [dict(n_corr=int(n), mse=float(m), e=int(e[0]), e2=int(e[1]), T=T.reshape(4, 4))
         for n, m, e, T in zip(z[f"{name}/n_corr"], z[f"{name}/mse"], z[f"{name}/e"], z[f"{name}/T"])]
    return dict(final=z[f"{name}/final"], history=h, aligned=z[f"{name}/aligned"],
                fitness=float(z[f"{name}/fitness"]), n_corr=h[-1]["n_corr"] if h else 0,
                **{k: meta[name][k] for k in ("state", "iterations", "converged")})


def golden_args(z, meta, name):
    kw = dict(meta[name]["args"])
    for k in ("indices", "guess"):
        if f"{name}/{k}" in z.files:
            kw[k] = z[f"{name}/{k}"]
    return kw


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_bit_equal_with_the_golden(gpu_ctx, golden, name):
    z, meta = golden
    r = raw_align(gpu_ctx, z[f"{name}/src"], z[f"{name}/tgt"], **golden_args(z, meta, name))
    assert_equals_reference(r, golden_ref(z, meta, name))
    st = r["stats"]
    src = z[f"{name}/src"] if "indices" not in golden_args(z, meta, name) else \
        z[f"{name}/src"][z[f"{name}/indices"]]
    assert st.n_src_finite == int(np.isfinite(src).all(axis=1).sum())
    assert st.n_tgt_finite == int(np.isfinite(z[f"{name}/tgt"]).all(axis=1).sum())
    # one stream synchronisation per correspondence pass of the loop
    assert st.host_syncs == st.iterations
    assert 1 <= st.levels <= 12


def test_far_queries_reach_coarser_levels(gpu_ctx, golden):
    z, meta = golden
    near = raw_align(gpu_ctx, z["shadow/src"], z["shadow/tgt"])["stats"].levels
    far = raw_align(gpu_ctx, z["far/src"], z["far/tgt"], max_iterations=3)["stats"].levels
    assert far > near


@pytest.mark.parametrize("name", ["shadow", "shadow_maxdist", "planes_iter", "far", "ties",
                                  "nonfinite"])
def test_correspondences_equal_the_restatement(gpu_ctx, golden, name):
    z, meta = golden
    src, tgt = z[f"{name}/src"], z[f"{name}/tgt"]
    md = meta[name]["args"].get("max_dist", math.sqrt(R.DBL_MAX))
    T = R.rigid((0.1, 0.3, 1.0), 3.0, (0.01, -0.02, 0.005))
    for xf in (None, R.IDENTITY, T):
        nn, d2 = D.icp_correspondences(src, tgt, transform=xf, max_dist=md, ctx=gpu_ctx)
        W = src if xf is None or xf is R.IDENTITY else R.transform_points(xf, src)
        rn, rd = R.correspondences(W, tgt, md)
        assert np.array_equal(nn, rn) and np.array_equal(bits(d2), bits(rd))
        if name == "shadow_maxdist" and xf is None:  # (part of the pairs is dropped)
            assert 0.2 * len(src) <= (rn >= 0).sum() <= 0.8 * len(src)


@pytest.mark.parametrize("nt", [1, 545])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 15, 16, 17, 63, 64, 65])
def test_small_sources(gpu_ctx, golden, n, nt):
    """fewer than 3 pairs, and the sizes around a wave"""
    z, _ = golden
    src, tgt = z["shadow_moved/src"][:n], z["shadow/tgt"][:nt]
    ref = R.align(src, tgt, max_iterations=4)
    r = raw_align(gpu_ctx, src, tgt, max_iterations=4)
    assert_equals_reference(r, ref)
    if n < 3:
        assert r["stats"].state == R.NO_CORRESPONDENCES and r["stats"].converged == 0
        assert np.array_equal(bits(r["final"]), bits(R.IDENTITY))
        assert np.array_equal(bits(r["aligned"]), bits(src))


def test_all_pairs_dropped(gpu_ctx, golden):
    z, _ = golden
    src, tgt = z["far/src"], z["far/tgt"]
    g = R.rigid((0, 0, 1), 1.0, (0.001, 0, 0))
    r = raw_align(gpu_ctx, src, tgt, guess=g, max_dist=1e-3)
    st = r["stats"]
    assert r["status"] == 0 and st.state == R.NO_CORRESPONDENCES and st.converged == 0
    assert st.iterations == 0 and st.n_corr == 0
    assert np.array_equal(bits(r["final"]), bits(g))
    assert np.array_equal(bits(r["aligned"]), bits(R.transform_points(g, src)))
    assert_equals_reference(r, R.align(src, tgt, guess=g, max_dist=1e-3))


def test_identity_guess_equals_null(gpu_ctx, golden):
    z, _ = golden
    src, tgt = z["shadow_moved/src"], z["shadow_moved/tgt"]
    a = raw_align(gpu_ctx, src, tgt)
    b = raw_align(gpu_ctx, src, tgt, guess=R.IDENTITY)
    for k in ("final", "aligned", "T"):
        assert np.array_equal(bits(a[k]), bits(b[k]))
    assert np.array_equal(dbits(a["mse"]), dbits(b["mse"]))


def test_strides(gpu_ctx, golden):
    z, meta = golden
    ref = golden_ref(z, meta, "nonfinite")
    src, tgt = z["nonfinite/src"], z["nonfinite/tgt"]
    for s, t in ((16, 12), (32, 16), (12, 32)):
        assert_equals_reference(raw_align(gpu_ctx, src, tgt, stride=s, tstride=t), ref)
    r = raw_align(gpu_ctx, src, tgt, out_stride=16)
    assert_equals_reference(r, ref)
    assert (r["out"][:, 3] == 1.0).all()
    assert raw_align(gpu_ctx, src, tgt, out_stride=32)["status"] == _lib.DLG_ERR_INVALID
    r = raw_align(gpu_ctx, src, tgt, want_aligned=False)
    assert np.array_equal(bits(r["final"]), bits(ref["final"]))


def test_status_codes(gpu_ctx, golden):
    z, _ = golden
    L = _lib.load()
    src, tgt = z["shadow/src"], z["shadow/tgt"]
    inv = _lib.DLG_ERR_INVALID
    assert raw_align(gpu_ctx, src, tgt, max_iterations=0)["status"] == inv
    assert b"max_iterations" in L.dlg_last_error(gpu_ctx.h)
    for md in (0.0, -1.0, math.nan):
        assert raw_align(gpu_ctx, src, tgt, max_dist=md)["status"] == inv
    assert b"max_correspondence_distance" in L.dlg_last_error(gpu_ctx.h)
    for bad in ([-1], [len(src)]):
        assert raw_align(gpu_ctx, src, tgt, indices=bad)["status"] == inv
    g = R.IDENTITY.copy()
    g[1, 2] = np.inf
    assert raw_align(gpu_ctx, src, tgt, guess=g)["status"] == inv
    assert b"guess" in L.dlg_last_error(gpu_ctx.h)
    assert raw_align(gpu_ctx, src, np.full((4, 3), np.nan, f32))["status"] == inv
    assert b"no finite point" in L.dlg_last_error(gpu_ctx.h)
    assert raw_align(gpu_ctx, src, np.zeros((0, 3), f32))["status"] == inv
    assert raw_align(gpu_ctx, src, tgt)["status"] == 0


def test_several_ranks_are_refused(golden):
    """a context of a 2-rank communicator holds a shard: DLG_ERR_INVALID, and no collective runs"""
    z, _ = golden
    ctxs = D.Context.loopback_group(2, 0)
    try:
        r = raw_align(ctxs[0], z["shadow/src"], z["shadow/tgt"])
        assert r["status"] == _lib.DLG_ERR_INVALID
        assert b"world > 1" in _lib.load().dlg_last_error(ctxs[0].h)
        with pytest.raises(D.DialogError):
            D.icp_correspondences(z["shadow/src"], z["shadow/tgt"], ctx=ctxs[1])
    finally:
        for c in ctxs:
            c.close()


def test_python_mirror_and_stats(gpu_ctx, golden):
    z, meta = golden
    src, tgt = z["shadow_moved/src"], z["shadow_moved/tgt"]
    ref = golden_ref(z, meta, "shadow_moved")
    final, aligned, hist, st = D.icp_align(src, tgt, fitness_max_range=R.DBL_MAX, ctx=gpu_ctx,
                                           return_history=True, return_stats=True)
    assert np.array_equal(bits(final), bits(ref["final"]))
    assert np.array_equal(bits(aligned), bits(ref["aligned"]))
    assert len(hist) == ref["iterations"] == st["iterations"]
    for h, g in zip(hist, ref["history"]):
        assert (h["n_corr"], h["e"], h["e2"]) == (g["n_corr"], g["e"], g["e2"])
        assert dbits(h["mse"])[0] == dbits(g["mse"])[0] and np.array_equal(bits(h["T"]), bits(g["T"]))
    assert st["state_name"] == "ABS_MSE" and st["converged"] == 1
    assert dbits(st["fitness"])[0] == dbits(ref["fitness"])[0] and st["device_ms"] >= 0
    assert st["n_src_finite"] == 446 and st["n_tgt_finite"] == 545
    plain = D.icp_align(src, tgt, ctx=gpu_ctx)
    assert len(plain) == 2 and np.array_equal(bits(plain[0]), bits(final))
    with pytest.raises(D.DialogError):
        D.icp_align(src, tgt, max_iterations=0, ctx=gpu_ctx)


def test_same_bits_twice_and_in_reversed_order(gpu_ctx, golden):
    """the sums are exact integers: neither a second run nor the visiting order shows in any bit"""
    z, meta = golden
    ref = golden_ref(z, meta, "planes_iter")
    src, tgt = z["planes_iter/src"], z["planes_iter/tgt"]
    assert gpu_ctx.get_option(D.DLG_OPT_ICP_REVERSED) == 0
    try:
        for opt in (0, 0, 1):
            gpu_ctx.set_option(D.DLG_OPT_ICP_REVERSED, opt)
            assert_equals_reference(raw_align(gpu_ctx, src, tgt, max_iterations=4), ref)
    finally:
        gpu_ctx.set_option(D.DLG_OPT_ICP_REVERSED, 0)


def test_cpp_icp_shim_runs_on_gpu(tmp_path, gpu_ctx, golden):
    """tests/cpp/shim_icp.cpp: on_registrationICPAction_triggered's calls on double_shadow's halves"""
    z, meta = golden
    src, tgt = z["shadow_moved/src"], z["shadow_moved/tgt"]
    exe = tmp_path / "shim_icp"
    lib = os.path.dirname(D.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_icp.cpp"), "-o", str(exe), "-L", lib,
                    "-ldialog_amd", f"-Wl,-rpath,{lib}"], check=True)
    files = []
    for k, a in enumerate((src, tgt, z["shadow_guess/src"], z["shadow_guess/guess"])):
        files.append(str(tmp_path / f"in{k}.f32"))
        np.ascontiguousarray(a, f32).tofile(files[-1])
    out = subprocess.run([str(exe), *files], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.strip().splitlines()}
    ref = golden_ref(z, meta, "shadow_moved")
    assert lines["converged"] == ["1"]
    assert lines["final"] == [str(int(b)) for b in bits(ref["final"]).reshape(16)]
    assert lines["fitness"] == [str(int(dbits(ref["fitness"])[0]))]
    u = bits(ref["aligned"])
    chk = sum((i * 3 + j + 1) * int(u[i, j]) for i in range(len(u)) for j in range(3)) % 2**64
    assert lines["aligned"] == [str(len(u)), str(chk)]
    g = golden_ref(z, meta, "shadow_guess")
    assert lines["guess"] == [str(int(b)) for b in bits(g["final"]).reshape(16)]


# ---- the paths of a huge cloud at small shapes (DLG_OPT_ICP_MAX_BLOCKS) --------------------------------
@contextmanager
def launch_options(ctx, max_blocks=0, reversed_=0):
    assert ctx.get_option(D.DLG_OPT_ICP_MAX_BLOCKS) == 0
    assert ctx.get_option(D.DLG_OPT_ICP_REVERSED) == 0
    try:
        ctx.set_option(D.DLG_OPT_ICP_MAX_BLOCKS, max_blocks)
        ctx.set_option(D.DLG_OPT_ICP_REVERSED, reversed_)
        yield
    finally:
        ctx.set_option(D.DLG_OPT_ICP_MAX_BLOCKS, 0)
        ctx.set_option(D.DLG_OPT_ICP_REVERSED, 0)


def test_max_blocks_option(gpu_ctx):
    assert _lib.DLG_OPT_ICP_MAX_BLOCKS == D.DLG_OPT_ICP_MAX_BLOCKS == 27
    assert gpu_ctx.get_option(D.DLG_OPT_ICP_MAX_BLOCKS) == 0
    try:
        for v in (1, 65536, 0):
            gpu_ctx.set_option(D.DLG_OPT_ICP_MAX_BLOCKS, v)
            assert gpu_ctx.get_option(D.DLG_OPT_ICP_MAX_BLOCKS) == v
        for bad in (-1, 65537, 1 << 40):
            with pytest.raises(D.DialogError) as ei:
                gpu_ctx.set_option(D.DLG_OPT_ICP_MAX_BLOCKS, bad)
            assert ei.value.status == _lib.DLG_ERR_INVALID and "0..65536" in str(ei.value)
            assert gpu_ctx.get_option(D.DLG_OPT_ICP_MAX_BLOCKS) == 0
    finally:
        gpu_ctx.set_option(D.DLG_OPT_ICP_MAX_BLOCKS, 0)


@pytest.mark.parametrize("cap", [1, 2, 3, 7])
def test_golden_under_a_block_cap(gpu_ctx, golden, cap):
    """planes_iter's 5,000 entries on `cap` workgroups: cap 1 gives a thread 19 or 20 entries (one
    flush inside k_icp_finish's loop, then a remainder of 3 or 4), cap 7 gives some threads 3 and
    others 2; every kernel takes several trips of its block-stride loop, the last one with a partial
    workgroup, in both visiting orders"""
    z, meta = golden
    ref = golden_ref(z, meta, "planes_iter")
    src, tgt = z["planes_iter/src"], z["planes_iter/tgt"]
    assert len(src) == 5000 and -(-5000 // 256) == 20 and 5000 - 19 * 256 == 136
    for rev in (0, 1):
        with launch_options(gpu_ctx, cap, rev):
            assert_equals_reference(raw_align(gpu_ctx, src, tgt, max_iterations=4), ref)


@pytest.fixture(scope="module")
def tiled(golden):
    z, _ = golden
    return R.tiled_source(z["shadow_moved/src"], 8193)


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8192, 8193])
def test_sizes_around_a_full_flush(gpu_ctx, golden, tiled, n):
    """one workgroup: 4096 entries are exactly kIcpFlush = 16 a thread (the flush inside the loop,
    then an empty last flush), 4097 give one thread a 17th, 8192 two full flushes"""
    z, _ = golden
    src, tgt = tiled[:n], z["shadow/tgt"]
    assert len(np.unique(src, axis=0)) == n and len(tgt) == 545
    ref = R.align(src, tgt, max_iterations=3)
    with launch_options(gpu_ctx, 1):
        assert_equals_reference(raw_align(gpu_ctx, src, tgt, max_iterations=3), ref)


@pytest.mark.parametrize("name", ["nonfinite", "shadow_dups"])
def test_nonfinite_and_index_list_inside_the_stride_loops(gpu_ctx, golden, name):
    z, meta = golden
    with launch_options(gpu_ctx, 1):
        r = raw_align(gpu_ctx, z[f"{name}/src"], z[f"{name}/tgt"], **golden_args(z, meta, name))
    assert_equals_reference(r, golden_ref(z, meta, name))


@pytest.fixture(scope="module")
def scatter():
    c = R.scatter_case()
    nn, d2 = R.correspondences(c["src"], c["tgt"])
    unlimited = math.sqrt(R.DBL_MAX)
    median = math.sqrt(float(np.median(d2[nn >= 0].astype(np.float64))))
    # (a third limit, below the coarser levels' radii: their empty queries are dropped there)
    c["limits"] = dict(unlimited=unlimited, median=median, near=3.0 * c["spacing"])
    c["pairs"] = {k: R.correspondences(c["src"], c["tgt"], md) for k, md in c["limits"].items()}
    c["align"] = {k: R.align(c["src"], c["tgt"], max_iterations=3, max_dist=md)
                  for k, md in c["limits"].items()}
    return c


@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("limit", ["unlimited", "median", "near"])
def test_scatter_fills_the_deferral_queues(gpu_ctx, scatter, limit, cap):
    """every workgroup holds queries that settle at every level: several workgroups append to the
    same queue, the queues shrink level by level, and under a max_dist part of each is dropped"""
    src, tgt, md = scatter["src"], scatter["tgt"], scatter["limits"][limit]
    rn, rd = scatter["pairs"][limit]
    if limit != "unlimited":
        assert (0.2 if limit == "median" else 0.05) * len(src) <= (rn >= 0).sum() <= 0.8 * len(src)
    with launch_options(gpu_ctx, cap):
        nn, d2 = D.icp_correspondences(src, tgt, max_dist=md, ctx=gpu_ctx)
        r = raw_align(gpu_ctx, src, tgt, max_iterations=3, max_dist=md)
    assert np.array_equal(nn, rn) and np.array_equal(bits(d2), bits(rd))
    assert_equals_reference(r, scatter["align"][limit])
    assert r["stats"].levels >= 3
    assert r["stats"].n_src_finite == int(np.isfinite(src).all(axis=1).sum()) < len(src)


@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("name", ["plane", "line"])
def test_degenerate_geometry(gpu_ctx, name, cap):
    """a hierarchy one cell thick on one axis (the plane z = 0.25) or on two (the x axis), and a
    rank-deficient M"""
    c = R.degenerate_cases()[name]
    ref = R.align(c["src"], c["tgt"])
    with launch_options(gpu_ctx, cap):
        assert_equals_reference(raw_align(gpu_ctx, c["src"], c["tgt"]), ref)
        nn, d2 = D.icp_correspondences(c["src"], c["tgt"], ctx=gpu_ctx)
    rn, rd = R.correspondences(c["src"], c["tgt"])
    assert np.array_equal(nn, rn) and np.array_equal(bits(d2), bits(rd))


@pytest.mark.parametrize("k", R.SCALE_RUNGS)
def test_scale_ladder(gpu_ctx, golden, k):
    """shadow_moved times 2^k.  -70: every first-pass d2 is 0 (d2max = 0: e2 = 0, no atomicMax);
    -60: they are subnormal, and so is a level radius's square; -40: normal d2 under the absolute
    1e-12 mse threshold; +40, +60: coordinates up to about 2^57, d2 up to about 2^107"""
    z, _ = golden
    c = R.scaled_case(dict(src=z["shadow_moved/src"], tgt=z["shadow_moved/tgt"]), k)
    rn, rd = R.correspondences(c["src"], c["tgt"])
    tiny = float(np.finfo(f32).tiny)
    if k == -70:
        assert (rd == 0).all()
    if k == -60:
        assert ((rd > 0) & (rd < tiny)).any()
    if k == 60:
        assert np.isfinite(rd).all() and rd.min() > 0
    ref = R.align(c["src"], c["tgt"], max_iterations=4)
    for cap in (0, 1):
        with launch_options(gpu_ctx, cap):
            nn, d2 = D.icp_correspondences(c["src"], c["tgt"], ctx=gpu_ctx)
            r = raw_align(gpu_ctx, c["src"], c["tgt"], max_iterations=4)
        assert np.array_equal(nn, rn) and np.array_equal(bits(d2), bits(rd))
        assert_equals_reference(r, ref)


# ---- the rest of the header's contract ----------------------------------------------------------------
def test_transformation_epsilon_ends_by_transform(gpu_ctx, golden):
    z, _ = golden
    src, tgt = z["shadow_moved/src"], z["shadow_moved/tgt"]
    ref = R.align(src, tgt, transformation_epsilon=1e-5)
    assert (ref["state"], ref["iterations"]) == (R.TRANSFORM, 5)
    r = raw_align(gpu_ctx, src, tgt, transformation_epsilon=1e-5)
    assert_equals_reference(r, ref)
    assert r["stats"].state == _lib.DLG_ICP_TRANSFORM == 2 and r["stats"].converged == 1


def test_history_cap_below_the_iteration_count(gpu_ctx, golden):
    z, meta = golden
    ref = golden_ref(z, meta, "shadow_moved")
    assert ref["iterations"] == 7
    r = raw_align(gpu_ctx, z["shadow_moved/src"], z["shadow_moved/tgt"], history_cap=2,
                  history_len=3)
    st = r["stats"]
    assert r["status"] == 0 and st.iterations == 7 and st.state == ref["state"]
    n_corr, mse, ee, T = R.history_arrays(ref)
    assert len(r["n_corr"]) == 2
    assert np.array_equal(r["n_corr"], n_corr[:2]) and np.array_equal(r["e"], ee[:2])
    assert np.array_equal(bits(r["T"]), bits(T[:2])) and np.array_equal(dbits(r["mse"]), dbits(mse[:2]))
    h = r["hist"][2]  # (the third record of the buffer is beyond the capacity passed: untouched)
    assert h.n_corr == -1 and math.isnan(h.mse) and (h.e, h.e2) == (-1, -1)
    assert all(math.isnan(v) for v in h.T)
    assert np.array_equal(bits(r["final"]), bits(ref["final"]))
    assert np.array_equal(bits(r["aligned"]), bits(ref["aligned"]))
    assert dbits(st.fitness)[0] == dbits(ref["fitness"])[0]
    # a capacity of 0 writes nothing
    r = raw_align(gpu_ctx, z["shadow_moved/src"], z["shadow_moved/tgt"], history_cap=0,
                  history_len=1)
    assert r["status"] == 0 and r["stats"].iterations == 7 and r["hist"][0].n_corr == -1
    assert np.array_equal(bits(r["final"]), bits(ref["final"]))


def test_null_history_and_null_stats(gpu_ctx, golden):
    z, meta = golden
    ref = golden_ref(z, meta, "shadow_moved")
    for hist, stats in ((False, True), (True, False), (False, False)):
        r = raw_align(gpu_ctx, z["shadow_moved/src"], z["shadow_moved/tgt"], want_history=hist,
                      want_stats=stats)
        assert r["status"] == 0
        assert np.array_equal(bits(r["final"]), bits(ref["final"]))
        assert np.array_equal(bits(r["aligned"]), bits(ref["aligned"]))
        if stats:
            assert r["stats"].iterations == 7
            assert dbits(r["stats"].fitness)[0] == dbits(ref["fitness"])[0]
        if not hist:
            assert r["hist"][0].n_corr == -1 and math.isnan(r["hist"][0].mse)


def test_fitness_max_range(gpu_ctx, golden):
    """getFitnessScore keeps d2 <= max_range: the median of the final pass's d2 keeps about half,
    a NaN or a negative range keeps nothing"""
    z, meta = golden
    src, tgt = z["shadow_moved/src"], z["shadow_moved/tgt"]
    ref = golden_ref(z, meta, "shadow_moved")
    _, d2 = R.correspondences(ref["aligned"], tgt)
    mr = float(np.median(d2.astype(np.float64)))
    kept = int((d2.astype(np.float64) <= mr).sum())
    assert 0.2 * len(src) <= kept <= 0.8 * len(src)
    want = R.fitness_score(ref["aligned"], tgt, mr)
    assert 0.0 < want < ref["fitness"]
    for cap in (0, 1):
        with launch_options(gpu_ctx, cap):
            r = raw_align(gpu_ctx, src, tgt, fitness_max_range=mr)
        assert_equals_reference(r, dict(ref, fitness=want))
    for none in (math.nan, -1.0, -math.inf):
        assert R.fitness_score(ref["aligned"], tgt, none) == R.DBL_MAX
        r = raw_align(gpu_ctx, src, tgt, fitness_max_range=none)
        assert r["stats"].fitness == R.DBL_MAX
        assert_equals_reference(r, dict(ref, fitness=R.DBL_MAX))
    # a range of exactly the largest d2 keeps every pair, one just below it drops that pair
    top = float(d2.max())
    assert_equals_reference(raw_align(gpu_ctx, src, tgt, fitness_max_range=top), ref)
    below = float(np.nextafter(d2.max(), f32(0)))
    r = raw_align(gpu_ctx, src, tgt, fitness_max_range=below)
    assert dbits(r["stats"].fitness)[0] == dbits(R.fitness_score(ref["aligned"], tgt, below))[0]
    assert r["stats"].fitness < ref["fitness"]


# ---- a production launch shape, no hook set -------------------------------------------------------------
def device_cu_count():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a child process: torch
    brings a HIP runtime of its own, which finds no device in a process where the library's runtime
    already holds it"""
    out = subprocess.run([sys.executable, "-c", "import torch; "
                          "print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return int(out.stdout.split()[-1])


def test_production_launch_shape(gpu_ctx):
    """600,000 entries against 50,000 points with the default options: more entries than
    k_icp_level's 8 x 256 x CUs threads (a second trip of its block-stride loop, the last workgroup
    partial), two or three entries a thread in k_icp_finish and the 2,048-workgroup cap of gather,
    apply and pack.  The reference is icp_ref.align on correspondences_fast (k-d tree candidates
    re-evaluated in float32, every uncertified query answered by the brute force).
    Wall time with the device call stubbed out, measured on a CPU-only machine: 6.3 s (0.15 s the
    two clouds, 6.1 s the reference: two k-d tree passes and the Python-integer moments of 600,000
    pairs twice); the child process that asks for the CU count adds torch's import."""
    cus = device_cu_count()
    c = R.large_case()
    src, tgt = c["src"], c["tgt"]
    assert len(src) == 600000 > 8 * 256 * cus and len(tgt) == 50000
    assert gpu_ctx.get_option(D.DLG_OPT_ICP_MAX_BLOCKS) == 0
    assert gpu_ctx.get_option(D.DLG_OPT_ICP_REVERSED) == 0
    info = {}
    ref = R.align(src, tgt, max_iterations=2, compute_fitness=False, fast=True, info=info)
    assert info["queries"] == 2 * len(src) and info["uncertified"] <= 0.01 * info["queries"]
    r = raw_align(gpu_ctx, src, tgt, max_iterations=2, fitness=False)
    assert_equals_reference(r, ref)
    assert r["stats"].host_syncs == 2 and r["stats"].n_corr == len(src)
