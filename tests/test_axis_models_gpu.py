"""GPU (gfx950): SACMODEL_PERPENDICULAR_PLANE / SACMODEL_PARALLEL_PLANE and dlg_score_samples
against the restatement of tests/axis_ref.py (the frozen oracle's primitives + the isModelValid
gate), bit for bit: best sample, iterations, draws, unrefined and refined coefficients, inlier
lists, per-draw counts / good / valid / coefficients -- on every device path (exhaustive and
pruned scorers, both tile scorers, speculative and host pick, lean and full rounds, device and
host PCL refit, the fast refit, point- and hypothesis-sharded ranks).

Scene: a room (floor z = 0 with 60 % of the points, wall x = 0 with 25 %, a 30-degree ramp with
10 %, 5 % noise), threshold 0.02.  With the axis z and eps = 5 degrees the parallel-plane model
must return the wall although the floor has more inliers: that is what fails if validity is
ignored.  Every reference is computed once (lru_cache) and shared.
"""
import functools
import math
import os
import subprocess
import threading
from typing import NamedTuple

import numpy as np
import pytest

import dialog_amd as D
from oracle import oracle as O

import axis_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.02
Z = (0.0, 0.0, 1.0)
OBLIQUE = (0.3, -1.7, 2.0)  # not a unit vector: the library must not assume one
DEG5, DEG30 = math.radians(5.0), math.radians(30.0)


class Case(NamedTuple):
    n: int
    model: int
    axis: tuple
    eps: float
    prob: float
    iters: int


# n in {3, 64, 1000, 4097, 16385} x both models x eps {0, 5, 30 degrees} x p {0.99, 1} x
# iterations {1, 50, 1000}, the oblique axis at two sizes: every value of every dimension occurs,
# each size with both models
CASES = [
    Case(3, R.PERP, Z, DEG5, 0.99, 50), Case(3, R.PAR, Z, DEG5, 1.0, 1),
    Case(64, R.PERP, Z, DEG30, 0.99, 50), Case(64, R.PAR, OBLIQUE, DEG30, 1.0, 50),
    Case(1000, R.PAR, Z, DEG5, 0.99, 1000), Case(1000, R.PERP, Z, 0.0, 0.99, 50),
    Case(4097, R.PAR, Z, DEG5, 1.0, 1000), Case(4097, R.PERP, Z, DEG5, 0.99, 50),
    Case(4097, R.PERP, OBLIQUE, DEG30, 1.0, 50),
    Case(16385, R.PAR, Z, DEG5, 1.0, 1000), Case(16385, R.PERP, Z, DEG30, 0.99, 1000),
    Case(16385, R.PAR, Z, DEG30, 1.0, 1), Case(16385, R.PAR, Z, 0.0, 0.99, 50),
]
WALL_CASES = [c for c in CASES if c.model == R.PAR and c.axis == Z and c.eps == DEG5 and c.n >= 1000]


class Path(NamedTuple):
    """context options of one device path; refit: "pcl" or "fast" """
    prune: int = -1
    spec: int = 1
    lean: int = 1
    pcl_dev: int = 1
    tile: int = D.DLG_TILE_EXACT
    score: int = D.DLG_SCORE_BF16
    refit: str = "pcl"


# DLG_OPT_PRUNE 1 forces the spatial copy (pruned scorer) on every cloud, the 4097- and
# 16385-point ones included; 0 takes the exhaustive scorers
PATHS = {
    "default": Path(),
    "pruned_exact": Path(prune=1),
    "pruned_bf16": Path(prune=1, tile=D.DLG_TILE_BF16),
    "exhaustive_exact_hostpick": Path(prune=0, spec=0, score=D.DLG_SCORE_EXACT),
    "pruned_hostpick_hostrefit": Path(prune=1, spec=0, pcl_dev=0),
    "exhaustive_hostrefit": Path(prune=0, pcl_dev=0),
    "pruned_fast": Path(prune=1, refit="fast"),
    "exhaustive_fast_hostpick": Path(prune=0, spec=0, refit="fast"),
    # (DLG_OPT_PCL_REFIT_DEVICE 3: the host recomputes every refit's tail, uploads its plane and
    # the select is redone with it -- the path an uncertain eigen33 transcendental takes)
    "pruned_host_recheck": Path(prune=1, pcl_dev=3),
    "pruned_full_rounds": Path(prune=1, lean=0),
    "pruned_full_rounds_fast": Path(prune=1, lean=0, refit="fast"),
}


def make_ctx(path, ctx=None):
    ctx = ctx or D.Context(0)
    ctx.set_option(D.DLG_OPT_PRUNE, path.prune)
    ctx.set_option(D.DLG_OPT_SPEC_PICK, path.spec)
    ctx.set_option(D.DLG_OPT_LEAN_ROUNDS, path.lean)
    ctx.set_option(D.DLG_OPT_PCL_REFIT_DEVICE, path.pcl_dev)
    ctx.set_option(D.DLG_OPT_PRUNE_TILE_SCORER, path.tile)
    ctx.set_option(D.DLG_OPT_SCORE_KERNEL, path.score)
    return ctx


def refit_mode(path):
    return D.DLG_REFIT_FAST if path.refit == "fast" else D.DLG_REFIT_PCL


@functools.lru_cache(maxsize=None)
def room(n, second_wall=False, floor=True):
    p = R.room(n, second_wall=second_wall, floor=floor)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def reference(case, refit):
    return R.segment(room(case.n), THR, model=case.model, axis=case.axis, eps=case.eps,
                     max_iterations=case.iters, probability=case.prob, refit_mode=refit)


def gpu_segment(ctx, pts, case, refit, model=None):
    ctx.set_axis(case.axis, case.eps)
    cloud = D.Cloud(ctx, pts)
    try:
        prm = D.make_params(THR, max_iterations=case.iters, probability=case.prob,
                            refit_mode=refit, model=case.model if model is None else model)
        return D.segment_cloud(cloud, prm)
    finally:
        cloud.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, r):
    inl, coeff, st = got
    assert st["has_model"] == r["ok"]
    assert st["iterations"] == r["iterations"], (st["iterations"], r["iterations"])
    assert st["draws"] == r["draws"]
    if not r["ok"]:
        assert inl.size == 0
        return
    assert list(st["best_sample"]) == list(r["best_sample"])
    assert np.array_equal(bits(st["coeff_unrefined"]), bits(r["coeff_unrefined"]))
    assert st["n_unrefined"] == r["n_unrefined"]
    assert np.array_equal(bits(coeff), bits(r["coeff"])), (coeff, r["coeff"])
    assert np.array_equal(inl, r["inliers"])


# ---- 2 + 3: segment() parity on every path ------------------------------------------------------
@pytest.mark.parametrize("path", sorted(k for k in PATHS if "full_rounds" not in k))
def test_segment_equals_restatement(path):
    P = PATHS[path]
    ctx = make_ctx(P)
    try:
        for case in CASES:
            assert_same(gpu_segment(ctx, room(case.n), case, refit_mode(P)), reference(case, P.refit))
    finally:
        ctx.close()


def test_parallel_plane_returns_the_wall_not_the_floor():
    """(restatement side) the cases that fail if validity is ignored: the winner is the wall
    x = 0 although the floor z = 0 holds more points within the threshold"""
    assert len(WALL_CASES) == 3
    for case in WALL_CASES:
        r = reference(case, "pcl")
        assert r["ok"] and r["unrefined_valid"] and r["refined_valid"]
        assert abs(r["coeff"][0]) > 0.99 and abs(r["coeff"][2]) < 0.05
        floor = O.count_within(room(case.n), np.array([0, 0, 1, 0], np.float32), THR)
        assert floor > 2 * r["inliers"].size > 0
        # and the unconstrained model on the same cloud takes the floor
        u = R.segment(room(case.n), THR, model=R.PLANE, max_iterations=case.iters,
                      probability=case.prob)
        assert abs(u["coeff"][2]) > 0.99


@pytest.mark.parametrize("model", [R.PERP, R.PAR])
def test_eps_zero_is_sacmodel_plane(gpu_ctx, model):
    """eps <= 0: both models reduce to SACMODEL_PLANE bit for bit (and to the oracle's)"""
    case = Case(4097, model, Z, 0.0, 0.99, 50)
    got = gpu_segment(gpu_ctx, room(4097), case, D.DLG_REFIT_PCL)
    plain = gpu_segment(gpu_ctx, room(4097), case, D.DLG_REFIT_PCL, model=R.PLANE)
    r = O.sac_segment(room(4097), THR, max_iterations=50, probability=0.99)
    for g in (got, plain):
        assert g[2]["iterations"] == r["iterations"] and g[2]["draws"] == r["draws"]
        assert list(g[2]["best_sample"]) == list(r["best_sample"])
        assert np.array_equal(bits(g[2]["coeff_unrefined"]), bits(r["coeff_unrefined"]))
        assert np.array_equal(bits(g[1]), bits(r["coeff"]))
        assert np.array_equal(g[0], r["inliers"])


def test_python_sac_segmentation_set_axis(gpu_ctx):
    """the PCL-style Python mirror: setModelType(SACMODEL_PARALLEL_PLANE), setAxis, setEpsAngle"""
    case = WALL_CASES[0]
    seg = D.SACSegmentation(gpu_ctx)
    seg.setModelType(D.SACMODEL_PARALLEL_PLANE)
    seg.setMethodType(D.SAC_RANSAC)
    seg.setDistanceThreshold(THR)
    seg.setMaxIterations(case.iters)
    seg.setProbability(case.prob)
    seg.setAxis(case.axis)
    seg.setEpsAngle(case.eps)
    seg.setInputCloud(room(case.n))
    inl, coeff = seg.segment()
    assert np.array_equal(seg.getAxis(), np.array(case.axis, np.float32)) and seg.getEpsAngle() == case.eps
    assert_same((inl, coeff, seg.last_stats), reference(case, "pcl"))
    gpu_ctx.set_axis((0, 0, 0), 0.0)


def test_set_axis_arguments(gpu_ctx):
    gpu_ctx.set_axis(OBLIQUE, 0.25)
    a, e = gpu_ctx.get_axis()
    assert np.array_equal(a, np.array(OBLIQUE, np.float32)) and e == 0.25  # stored as given
    for bad in ((np.nan, 0, 1), (0, np.inf, 1), (0, 0, -np.inf)):
        with pytest.raises(D.DialogError) as ei:
            gpu_ctx.set_axis(bad, 0.1)
        assert ei.value.status == 1
    with pytest.raises(D.DialogError):
        gpu_ctx.set_axis(Z, math.nan)
    a, e = gpu_ctx.get_axis()
    assert np.array_equal(a, np.array(OBLIQUE, np.float32)) and e == 0.25  # unchanged by a failure
    gpu_ctx.set_axis((0, 0, 0), 0.0)


# ---- 4: every hypothesis invalid ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wall_and_ramp():
    """only the wall x = 0 and the 30-degree ramp: neither is within 5 degrees of the z axis (a
    mixed triple can be, by chance: the restatement asserts that none of this cloud's 51 draws is)"""
    p = R.room(1000, floor=False, noise=False, seed=6)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def all_invalid_reference(refit):
    case = Case(1000, R.PERP, Z, DEG5, 0.99, 50)
    return case, R.segment(wall_and_ramp(), THR, model=case.model, axis=case.axis,
                           eps=case.eps, max_iterations=case.iters, probability=case.prob,
                           refit_mode=refit)


@pytest.mark.parametrize("path", ["default", "pruned_exact", "exhaustive_exact_hostpick",
                                  "pruned_hostpick_hostrefit", "pruned_fast"])
def test_all_invalid_first_good_draw_wins_with_no_inliers(path):
    P = PATHS[path]
    case, r = all_invalid_reference(P.refit)
    # (restatement side) no valid hypothesis: the first good draw won with count 0
    assert r["ok"] and not r["unrefined_valid"] and r["n_unrefined"] == 0 and r["inliers"].size == 0
    assert r["iterations"] == case.iters + 1
    assert np.all(np.isfinite(r["coeff"])) and np.array_equal(bits(r["coeff"]), bits(r["coeff_unrefined"]))
    pts = wall_and_ramp()
    ctx = make_ctx(P)
    try:
        got = gpu_segment(ctx, pts, case, refit_mode(P))
        assert got[2]["has_model"] and got[2]["n_unrefined"] == 0 and got[0].size == 0
        assert np.all(np.isfinite(got[1]))
        assert_same(got, r)
        cloud = D.Cloud(ctx, pts)
        prm = D.make_params(THR, max_iterations=case.iters, probability=case.prob,
                            refit_mode=refit_mode(P), model=case.model)
        e = D.extract_planes(cloud, prm, max_planes=3)
        assert e["n_planes"] == 0 and e["inliers"].size == 0 and cloud.n_active == 1000
        cloud.close()
    finally:
        ctx.close()


# ---- 5: a valid winner whose refit tips over the bound ------------------------------------------
TILT = math.radians(2.0)
REFINED_EPS = math.radians(1.9)


@functools.lru_cache(maxsize=None)
def tilted_floor():
    """a floor tilted by 2 degrees with 4 mm noise: single triples scatter around the tilt, so some
    fall within 1.9 degrees of z, but the least-squares refit recovers the 2 degrees"""
    rng = np.random.default_rng(77)
    n = 1000
    u, v, e = rng.uniform(0, 4, n), rng.uniform(0, 4, n), rng.normal(0, 0.004, n)
    p = np.c_[u * math.cos(TILT) - e * math.sin(TILT), v, u * math.sin(TILT) + e * math.cos(TILT)]
    p = np.ascontiguousarray(p, np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def refined_invalid_reference(refit):
    case = Case(1000, R.PERP, Z, REFINED_EPS, 1.0, 1000)
    return case, R.segment(tilted_floor(), THR, model=case.model, axis=case.axis, eps=case.eps,
                           max_iterations=case.iters, probability=case.prob, refit_mode=refit)


@pytest.mark.parametrize("path", ["default", "pruned_exact", "pruned_hostpick_hostrefit",
                                  "exhaustive_hostrefit", "pruned_fast", "exhaustive_fast_hostpick",
                                  "pruned_host_recheck"])
def test_refined_model_invalid_reports_coefficients_and_no_inliers(path):
    P = PATHS[path]
    case, r = refined_invalid_reference(P.refit)
    # (restatement side) the case does what it is built for
    assert r["ok"] and r["unrefined_valid"] and r["n_unrefined"] > 500 and not r["refined_valid"]
    assert r["inliers"].size == 0 and not np.array_equal(bits(r["coeff"]), bits(r["coeff_unrefined"]))
    ctx = make_ctx(P)
    try:
        got = gpu_segment(ctx, tilted_floor(), case, refit_mode(P))
        assert got[0].size == 0 and got[2]["n_unrefined"] == r["n_unrefined"]
        assert_same(got, r)
        cloud = D.Cloud(ctx, tilted_floor())
        prm = D.make_params(THR, max_iterations=case.iters, probability=case.prob,
                            refit_mode=refit_mode(P), model=case.model)
        assert D.extract_planes(cloud, prm, max_planes=3)["n_planes"] == 0
        cloud.close()
    finally:
        ctx.close()


# ---- 6: dlg_extract_planes -------------------------------------------------------------------
EXTRACT = dict(max_planes=5, min_inliers=40)
EXTRACT_KW = dict(max_iterations=300, probability=0.99)


@functools.lru_cache(maxsize=None)
def extract_reference(refit):
    e = R.extract(room(16385, second_wall=True), THR, model=R.PAR, axis=Z, eps=DEG5,
                  refit_mode=refit, **EXTRACT, **EXTRACT_KW)
    # both walls come out first, every plane is vertical, and several rounds run
    assert e["n_planes"] >= 3
    assert abs(e["coeffs"][0][2]) < 0.1 and abs(e["coeffs"][1][2]) < 0.1
    assert {int(np.argmax(np.abs(e["coeffs"][k][:3]))) for k in (0, 1)} == {0, 1}
    return e


def assert_same_extract(e, ref):
    assert e["n_planes"] == ref["n_planes"]
    assert np.array_equal(bits(e["coeffs"]), bits(ref["coeffs"]))
    assert np.array_equal(e["offsets"], ref["offsets"])
    assert np.array_equal(e["inliers"], ref["inliers"])


@pytest.mark.parametrize("path", ["default", "pruned_exact", "pruned_bf16", "pruned_full_rounds",
                                  "pruned_hostpick_hostrefit", "pruned_fast", "pruned_host_recheck",
                                  "pruned_full_rounds_fast", "exhaustive_fast_hostpick"])
def test_extract_planes_equals_restatement(path):
    P = PATHS[path]
    ref = extract_reference(P.refit)
    ctx = make_ctx(P)
    try:
        ctx.set_axis(Z, DEG5)
        cloud = D.Cloud(ctx, room(16385, second_wall=True))
        prm = D.make_params(THR, refit_mode=refit_mode(P), model=R.PAR, **EXTRACT_KW)
        e = D.extract_planes(cloud, prm, **EXTRACT)
        assert_same_extract(e, ref)
        if P.prune == 1 and P.pcl_dev:  # (lean rounds need the spatial copy and a device refit)
            assert (e["stats"]["lean_rounds"] > 0) == bool(P.lean)
        assert cloud.n_active == 16385 - ref["offsets"][-1]
        cloud.close()
    finally:
        ctx.close()


def run_ranks(world, body):
    ctxs = D.Context.loopback_group(world, 0)
    out, errs = [None] * world, []

    def run(r):
        try:
            out[r] = body(ctxs[r], r)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    for c in ctxs:
        c.close()
    assert not errs, errs
    return out


@pytest.mark.parametrize("hyp_shard,refit", [(0, "pcl"), (0, "fast"), (1, "pcl")])
def test_extract_planes_two_ranks(hyp_shard, refit):
    """point shards (each rank its half) and DLG_OPT_HYP_SHARD 1 (each rank the whole cloud) on a
    loopback group of 2 ranks, DLG_OPT_SYNC_CHECK comparing the ranks' axis and eps every round"""
    ref = extract_reference(refit)
    pts = room(16385, second_wall=True)
    half = pts.shape[0] // 2
    mode = D.DLG_REFIT_FAST if refit == "fast" else D.DLG_REFIT_PCL

    def body(ctx, r):
        ctx.set_option(D.DLG_OPT_HYP_SHARD, hyp_shard)
        ctx.set_option(D.DLG_OPT_SYNC_CHECK, 1)
        ctx.set_axis(Z, DEG5)
        if hyp_shard:
            cloud = D.Cloud(ctx, pts)
        else:
            lo, hi = (0, half) if r == 0 else (half, pts.shape[0])
            cloud = D.Cloud(ctx, pts[lo:hi], id_base=lo)
        prm = D.make_params(THR, refit_mode=mode, model=R.PAR, **EXTRACT_KW)
        e = D.extract_planes(cloud, prm, capacity=pts.shape[0], **EXTRACT)
        cloud.close()
        return e

    for e in run_ranks(2, body):
        assert_same_extract(e, ref)


def test_sync_check_catches_ranks_with_different_axes():
    pts = room(4097)
    half = pts.shape[0] // 2
    errs = []

    def body(ctx, r):
        ctx.set_option(D.DLG_OPT_HYP_SHARD, 0)
        ctx.set_option(D.DLG_OPT_SYNC_CHECK, 1)
        ctx.set_axis(Z, DEG30 if r == 0 else math.radians(30.5))
        lo, hi = (0, half) if r == 0 else (half, pts.shape[0])
        cloud = D.Cloud(ctx, pts[lo:hi], id_base=lo)
        prm = D.make_params(THR, model=R.PERP, max_iterations=20, probability=1.0)
        try:
            D.extract_planes(cloud, prm, capacity=pts.shape[0], max_planes=2)
        except D.DialogError as e:
            errs.append(str(e))
        return None

    run_ranks(2, body)
    assert len(errs) == 2 and any("eps_angle" in e for e in errs), errs


# ---- 7: dlg_score_samples ----------------------------------------------------------------------
def draws(n_active, d, seed=12345):
    """the first batch of d draws of dlg_sac_control_next over an n_active-long list"""
    ctl = D.RansacControl(D.make_params(THR, max_iterations=5000, probability=1.0, seed=seed),
                          n_active, max_batch=d)
    pos = ctl.next().copy()
    ctl.close()
    assert pos.shape == (d, 3)
    return pos


@functools.lru_cache(maxsize=None)
def room_normals():
    nrm = O.estimate_normals_knn(room(4097), 12)
    nrm.setflags(write=False)
    return nrm


@functools.lru_cache(maxsize=None)
def indexed():
    idx = np.random.default_rng(3).choice(4097, 3000, replace=False).astype(np.int32)  # unsorted
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def removed_two():
    """the room after two SACMODEL_PLANE extraction rounds (floor and wall gone)"""
    e = R.extract(room(4097), THR, max_planes=2, min_inliers=100, max_iterations=100,
                  probability=0.99)
    assert e["n_planes"] == 2 and 300 < e["remaining"].size < 1200
    return e


# (the parallel model takes the axis as given: with |OBLIQUE| = 2.6 its band is |cos| <= 0.33)
SCORE_MODELS = {R.PLANE: (Z, 0.0), R.PERP: (Z, DEG30), R.PAR: (OBLIQUE, math.radians(60.0)),
                R.NORMAL_PLANE: (Z, 0.0)}


@functools.lru_cache(maxsize=None)
def score_reference(which, model, d):
    axis, eps = SCORE_MODELS[model]
    active = None
    if which == "indexed":
        active = indexed()
    elif which == "removed":
        active = removed_two()["remaining"]
    n_active = 4097 if active is None else active.size
    pos = draws(n_active, d)
    ref = R.score(room(4097), THR, pos, model, axis, eps, active=active,
                  normals=room_normals() if model == R.NORMAL_PLANE else None)
    return pos, ref


def assert_same_score(got, ref):
    assert np.array_equal(got["good"], ref["good"])
    assert np.array_equal(got["valid"], ref["valid"])
    nan = np.isnan(ref["coeffs"])  # (bad samples: all four NaN; any NaN payload)
    assert np.array_equal(np.isnan(got["coeffs"]), nan)
    assert np.array_equal(nan.all(axis=1), ref["good"] == 0) and not nan[ref["good"] == 1].any()
    assert np.array_equal(bits(got["coeffs"])[~nan], bits(ref["coeffs"])[~nan])
    assert np.array_equal(got["counts"], ref["counts"]), np.nonzero(got["counts"] != ref["counts"])


@pytest.mark.parametrize("path", ["default", "pruned_exact", "pruned_bf16", "exhaustive_exact_hostpick"])
@pytest.mark.parametrize("model", sorted(SCORE_MODELS))
def test_score_samples_all_draws(path, model):
    """counts of ALL D draws, good, valid and coefficient bits, D in {1, 63, 64, 65, 4096};
    model 11 with k-NN normals and weight 0.1, exhaustive and pruned-NP"""
    P = PATHS[path]
    axis, eps = SCORE_MODELS[model]
    ctx = make_ctx(P)
    try:
        ctx.set_axis(axis, eps)
        cloud = D.Cloud(ctx, room(4097))
        if model == R.NORMAL_PLANE:
            cloud.set_normals(room_normals())
        prm = D.make_params(THR, model=model, normal_distance_weight=0.1)
        n_invalid = n_good = 0
        for d in (1, 63, 64, 65, 4096):
            pos, ref = score_reference("full", model, d)
            assert_same_score(D.score_samples(cloud, prm, pos), ref)
            assert cloud.n_active == 4097  # the list is left as it was
            n_invalid += int(np.count_nonzero(ref["valid"] == 0))
            n_good += int(np.count_nonzero(ref["good"]))
            if d == 4096:
                assert np.count_nonzero(ref["counts"] > 400) > 20  # (not all near-empty planes)
        if model in (R.PERP, R.PAR):
            # (restatement side) the test cannot pass by having nothing to reject
            assert 0.1 * n_good <= n_invalid <= 0.9 * n_good, (n_invalid, n_good)
        else:
            assert n_invalid == 0
        cloud.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("path", ["default", "pruned_exact"])
def test_score_samples_on_lists(path):
    """the remaining list after two extraction rounds (a lean list on the pruned path), and a
    setIndices cloud"""
    P = PATHS[path]
    ctx = make_ctx(P)
    try:
        for model in (R.PERP, R.PAR):
            axis, eps = SCORE_MODELS[model]
            ctx.set_axis(axis, eps)
            prm = D.make_params(THR, model=model)
            # after two rounds
            cloud = D.Cloud(ctx, room(4097))
            e = D.extract_planes(cloud, D.make_params(THR, max_iterations=100, probability=0.99),
                                 max_planes=2, min_inliers=100)
            assert np.array_equal(e["inliers"], removed_two()["inliers"])
            inv = good = 0
            for d in (65, 1024):
                pos, ref = score_reference("removed", model, d)
                assert_same_score(D.score_samples(cloud, prm, pos), ref)
                inv += int(np.count_nonzero(ref["valid"] == 0))
                good += int(np.count_nonzero(ref["good"]))
            assert 0.1 * good <= inv <= 0.9 * good, (inv, good)  # (restatement side)
            assert cloud.n_active == removed_two()["remaining"].size
            cloud.close()
            # setIndices
            cloud = D.Cloud(ctx, room(4097), indices=indexed())
            pos, ref = score_reference("indexed", model, 65)
            assert_same_score(D.score_samples(cloud, prm, pos), ref)
            cloud.close()
    finally:
        ctx.close()


def test_score_samples_arguments(gpu_ctx):
    cloud = D.Cloud(gpu_ctx, room(64))
    prm = D.make_params(THR, model=R.PAR)
    ok = np.array([[0, 1, 2]], np.int32)
    assert D.score_samples(cloud, prm, ok)["good"].shape == (1,)
    for bad in (np.array([[0, 1, 64]], np.int32), np.array([[-1, 1, 2]], np.int32),
                np.zeros((4097, 3), np.int32)):
        with pytest.raises(D.DialogError) as ei:
            D.score_samples(cloud, prm, bad)
        assert ei.value.status == 1
    with pytest.raises(D.DialogError):  # model 11 without normals, as segment()
        D.score_samples(cloud, D.make_params(THR, model=R.NORMAL_PLANE), ok)
    with pytest.raises(D.DialogError):
        D.score_samples(cloud, D.make_params(THR, model=5), ok)
    cloud.close()


@pytest.mark.parametrize("hyp_shard", [0, 1])
def test_score_samples_two_ranks(hyp_shard):
    """N > 1: the gather allreduce and the count allreduce (point shards), the hypothesis slices"""
    pts = room(4097)
    half = pts.shape[0] // 2
    axis, eps = SCORE_MODELS[R.PAR]
    pos, ref = score_reference("full", R.PAR, 65)

    def body(ctx, r):
        ctx.set_option(D.DLG_OPT_HYP_SHARD, hyp_shard)
        ctx.set_axis(axis, eps)
        if hyp_shard:
            cloud = D.Cloud(ctx, pts)
        else:
            lo, hi = (0, half) if r == 0 else (half, pts.shape[0])
            cloud = D.Cloud(ctx, pts[lo:hi], id_base=lo)
        got = D.score_samples(cloud, D.make_params(THR, model=R.PAR), pos)
        cloud.close()
        return got

    for got in run_ranks(2, body):
        assert_same_score(got, ref)


# ---- 8: the C++ shim -------------------------------------------------------------------------
def test_cpp_shim_axis_models(tmp_path):
    """tests/cpp/shim_axis.cpp: setModelType(pcl::SACMODEL_PARALLEL_PLANE), setAxis, setEpsAngle,
    segment through the PCL-style shim equal the C ABI's result on the same room (and the
    restatement's: the wall)"""
    exe = tmp_path / "shim_axis"
    lib = os.path.dirname(D.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_axis.cpp"), "-o", str(exe), "-L", lib,
                    "-ldialog_amd", f"-Wl,-rpath,{lib}"], check=True)
    pts = room(4097)
    f = tmp_path / "room.bin"
    pts.tofile(f)
    out = subprocess.run([str(exe), str(f), "4097"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = dict(ln.split(" ", 1) for ln in out.stdout.strip().splitlines())
    assert lines["same"].strip() == "1"
    r = reference(Case(4097, R.PAR, Z, DEG5, 0.99, 50), "pcl")
    assert [int(w, 16) for w in lines["coeff"].split()] == [int(v) for v in bits(r["coeff"])]
    assert int(lines["inliers"].split()[0]) == r["inliers"].size
    assert lines["perpendicular_eps0_same_as_plane"].strip() == "1"
    v = lines["vertical_planes"].split()  # "<vertical> of <planes>": both walls, nothing else
    assert v[0] == v[2] and int(v[0]) >= 1
