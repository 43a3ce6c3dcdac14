"""GPU (gfx950): culled scoring of probability-1 rounds (DLG_OPT_CULL; spatial.hpp).

A culled round scores exactly only the hypotheses whose tile bound -- 32 x the tiles whose sphere
test the plane passes -- can still reach the best exact count.  Held against the oracle here:

  * the bound is a bound: dlg_score_benchmark(DLG_SCORE_BOUND) >= countWithinDistance for every
    hypothesis, on clouds with partial last tiles and super-tiles, thick slabs, exact ties,
    non-finite points and index lists;
  * culled scoring (DLG_SCORE_CULLED): every scored hypothesis has the oracle's count, the oracle's
    first strict maximum is scored, and every culled hypothesis counts less than that maximum, for
    K = 2, 64, 4096 first candidates and D = 48, 256, 4096 hypotheses;
  * extraction with DLG_OPT_CULL 0, 1 and 2 is bit-equal to the oracle's chain and to each other,
    in both refit modes, after a reset, on pure noise (where the bound separates nothing and the
    call falls back), and for an axis-constrained model.

Every cloud is uploaded with DLG_OPT_PRUNE 1, so the pruned path runs below the 131072-point
cut-off.  The hypotheses dlg_score_benchmark draws are replayed on the host: position i of 3 D is
(uint32)rnd() % n_active over Mt19937(777) (its contract, include/dialog_ransac.h).
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import dialog_amd as D
from dialog_amd import _lib
from dialog_amd.synth import plane_cloud
from oracle import oracle as O

import axis_ref as R

pytestmark = pytest.mark.gpu
DMAX = 4096
TILE = 32
THR = 0.02


# ---- clouds: name -> (points, indices or None, threshold) ---------------------------------------
def _multi(n, seed):
    return plane_cloud(n, 5, sigma=0.01, seed=seed)[0], None, THR


def _slab():
    # a slab thicker than the threshold (sigma = 5 thresholds): n = 1 (mod 32)
    return plane_cloud(20001, 2, sigma=0.1, seed=72)[0], None, THR


def _coplanar_q():
    # exactly coplanar, quantised: z = 0.5, x and y multiples of 1/8; every good draw is the plane
    # (0, 0, +-1, -+0.5) and counts all n points; n = 31 (mod 32)
    n = 20031
    rng = np.random.default_rng(73)
    p = np.empty((n, 3), np.float32)
    p[:, :2] = rng.integers(-400, 401, size=(n, 2)) * 0.125
    p[:, 2] = 0.5
    return p, None, THR


def _coplanar_full():
    # the same with n = 0 (mod 32): every tile is full, so every tied draw's bound 32 nt equals
    # its count n exactly -- pass B's rule must keep a bound EQUAL to the best count (>=, not >)
    p = _coplanar_q()[0]
    return np.ascontiguousarray(p[:20000]), None, THR


def _wide():
    p = plane_cloud(24000, 6, sigma=0.01, seed=74)[0]
    return (p * np.float32(300.0)).astype(np.float32), None, 6.0


def _nonfinite():
    p = plane_cloud(20003, 4, sigma=0.01, seed=75)[0]
    p[::7, 0] = np.nan
    p[3::11, 2] = np.inf
    return p, None, THR


def _indexed():
    p = plane_cloud(30000, 4, sigma=0.01, seed=76)[0]
    idx = np.random.default_rng(9).choice(30000, 20000, replace=False).astype(np.int32)
    return p, idx, THR


def _collinear():
    t = np.arange(20000, dtype=np.float32) * np.float32(0.001)
    return np.stack([t, 2 * t, -t], axis=1).astype(np.float32), None, THR


CLOUDS = {
    "multi": functools.partial(_multi, 20000, 71),  # n = 0 (mod 32)
    "slab": _slab, "coplanar": _coplanar_q, "coplanar_full": _coplanar_full, "wide": _wide, "nonfinite": _nonfinite,
    "indexed": _indexed, "collinear": _collinear,
    "n513": functools.partial(_multi, 513, 77),     # partial last tile, one partial super-tile
    "n8193": functools.partial(_multi, 8193, 78),   # just over 16 super-tiles, one hyper
}


@functools.lru_cache(maxsize=None)
def _stream():
    return O.rnd_stream(3 * DMAX, seed=777)


@functools.lru_cache(maxsize=None)
def reference(cloud, n_hyp):
    """the oracle's verdict, plane and count of the first n_hyp replayed hypotheses (0 for a
    rejected sample), computed once per cloud at the largest D a test asks for"""
    pts, idx, thr = CLOUDS[cloud]()
    active = np.ascontiguousarray(pts if idx is None else pts[idx], np.float32)
    pos = (_stream()[:3 * n_hyp] % active.shape[0]).reshape(n_hyp, 3)
    ok = np.zeros(n_hyp, bool)
    counts = np.zeros(n_hyp, np.int64)
    for d in range(n_hyp):
        ok[d], coef = O.plane_coefficients(*active[pos[d]])
        if ok[d]:
            counts[d] = O.count_within(active, coef, thr)
    ok.flags.writeable = counts.flags.writeable = False
    return ok, counts


def ref_head(cloud, n_hyp):
    ok, counts = reference(cloud, FULL_D[cloud])  # (a smaller D's draw is a prefix of a larger one's)
    return ok[:n_hyp], counts[:n_hyp]


@pytest.fixture(scope="module")
def pctx():
    """a context of its own whose clouds all get a spatial copy (the option applies at upload)"""
    ctx = D.Context(0)
    ctx.set_option(D.DLG_OPT_PRUNE, 1)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def uploaded(pctx):
    """each cloud uploaded once per module"""
    held = {}

    def get(name):
        if name not in held:
            pts, idx, _ = CLOUDS[name]()
            held[name] = D.Cloud(pctx, pts, indices=idx)
        return held[name]
    yield get
    for c in held.values():
        c.close()


def bench_counts(ctx, cloud, n_hyp, kernel, thr, k=1):
    ms = C.c_double()
    out = np.full(n_hyp, -7, np.int32)
    ctx.set_option(D.DLG_OPT_CULL, k)
    try:
        ctx.check(_lib.load().dlg_score_benchmark(ctx.h, cloud.h, n_hyp, kernel, 1, thr, C.byref(ms),
                                                  out.ctypes.data_as(C.POINTER(C.c_int32))))
    finally:
        ctx.set_option(D.DLG_OPT_CULL, 1)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


CULL_CLOUDS = ("multi", "coplanar", "coplanar_full", "n8193")
# hypotheses of a cloud's bound test; its reference is computed once, for the most any test uses
BOUND_D = {"multi": DMAX, "wide": DMAX}
FULL_D = {name: DMAX if name in CULL_CLOUDS or name in BOUND_D else 256 for name in CLOUDS}


# ---- the bound ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_bound_is_a_bound(pctx, uploaded, name):
    """32 nt_h >= the oracle's count of every hypothesis (bad draws: the oracle counts 0), in
    whole tiles, and it agrees with the exact pruned scorer's counts on the same launch path."""
    n_hyp = BOUND_D.get(name, 256)
    thr = CLOUDS[name]()[2]
    ok, counts = ref_head(name, n_hyp)
    bound = bench_counts(pctx, uploaded(name), n_hyp, D.DLG_SCORE_BOUND, thr)
    assert (bound >= 0).all() and (bound % TILE == 0).all()
    low = np.flatnonzero(bound < counts)
    assert low.size == 0, [(int(i), int(bound[i]), int(counts[i])) for i in low[:4]]
    exact = bench_counts(pctx, uploaded(name), n_hyp, D.DLG_SCORE_PRUNED, thr)
    assert np.array_equal(exact, counts)
    assert name == "collinear" or counts.max() > 0


# ---- culled scoring -------------------------------------------------------------------------------
KS = (2, 64, DMAX)
DS = (48, 256, DMAX)


def set_a(bound, ok, k):
    """the K good hypotheses with the largest bound, ties to the lower index"""
    good = np.flatnonzero(ok)
    order = good[np.lexsort((good, -bound[good].astype(np.int64)))]
    return set(int(i) for i in order[:k])


@pytest.mark.parametrize("n_hyp", DS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", CULL_CLOUDS)
def test_culled_scoring(pctx, uploaded, name, k, n_hyp):
    """DLG_SCORE_CULLED: a scored hypothesis has the oracle's count; the oracle's first strict
    maximum over the good draws is scored; a culled good draw counts less than that maximum; a
    bad draw is never scored.  On the coplanar cloud every good draw ties at n, so all of them must
    be scored (the first wins by index: test_segment_ties_and_bad_draws)."""
    thr = CLOUDS[name]()[2]
    ok, counts = ref_head(name, n_hyp)
    got = bench_counts(pctx, uploaded(name), n_hyp, D.DLG_SCORE_CULLED, thr, k)
    assert ((got >= 0) | (got == -1)).all()
    scored = got >= 0
    assert not (scored & ~ok).any()
    wrong = np.flatnonzero(scored & (got != counts))
    assert wrong.size == 0, [(int(i), int(got[i]), int(counts[i])) for i in wrong[:4]]
    assert ok.any()
    best = int(counts[ok].max())
    first = int(np.flatnonzero(ok & (counts == best))[0])
    assert got[first] == best
    culled = ok & ~scored
    high = np.flatnonzero(culled & (counts >= best))
    assert high.size == 0, [(int(i), int(counts[i]), best) for i in high[:4]]
    if name.startswith("coplanar"):
        assert best == CLOUDS[name]()[0].shape[0] and (got[ok] == best).all()
    if name == "coplanar_full" and n_hyp == 256:
        # the tie of bound and best count is real: pass B keeps it only with >=
        bound = bench_counts(pctx, uploaded(name), n_hyp, D.DLG_SCORE_BOUND, thr)
        assert (bound[ok] == best).all()
    if k >= n_hyp:  # K >= D: every good draw is in the first pass
        assert scored[ok].all()
    if name == "multi" and k == 2 and n_hyp == 256:
        # the winner is not among the two largest bounds: it is found by the second pass
        bound = bench_counts(pctx, uploaded(name), n_hyp, D.DLG_SCORE_BOUND, thr)
        assert first not in set_a(bound, ok, 2)


def test_culled_scoring_collinear(pctx, uploaded):
    """every draw of a collinear cloud is bad: nothing is scored"""
    ok, _ = ref_head("collinear", 256)
    assert not ok.any()
    got = bench_counts(pctx, uploaded("collinear"), 256, D.DLG_SCORE_CULLED, THR, 2)
    assert (got == -1).all()


def segment(ctx, cloud, k, iters=255, thr=THR, model=D.SACMODEL_PLANE, refit=D.DLG_REFIT_PCL):
    ctx.set_option(D.DLG_OPT_CULL, k)
    try:
        prm = D.make_params(thr, max_iterations=iters, probability=1.0, refit_mode=refit, model=model)
        return D.segment_cloud(cloud, prm)
    finally:
        ctx.set_option(D.DLG_OPT_CULL, 1)


@pytest.mark.parametrize("k", (0, 1, 2))
def test_segment_ties_and_bad_draws(pctx, uploaded, k):
    """coplanar cloud: many draws tie at count n and the first wins (all of them reach the second
    pass under K = 2); collinear cloud: no good draw, the pick reports none."""
    pts = CLOUDS["coplanar"]()[0]
    r = O.sac_segment(pts, THR, max_iterations=255, probability=1.0)
    pctx.cull_stats(reset=True)
    inl, coeff, st = segment(pctx, uploaded("coplanar"), k)
    cs = pctx.cull_stats(reset=True)
    assert st["has_model"] and r["ok"]
    assert list(st["best_sample"]) == list(r["best_sample"])
    assert st["n_unrefined"] == r["n_unrefined"] == pts.shape[0]
    assert np.array_equal(bits(coeff), bits(r["coeff"])) and np.array_equal(inl, r["inliers"])
    if k == 2:
        assert cs["rounds"] == 1 and cs["scored_a"] == 2 and cs["scored_b"] > 0 and cs["culled"] == 0
    if k == 0:
        assert not any(cs.values())
    inl, coeff, st = segment(pctx, uploaded("collinear"), k)
    r = O.sac_segment(CLOUDS["collinear"]()[0], THR, max_iterations=255, probability=1.0)
    assert not st["has_model"] and not r["ok"] and inl.size == 0
    cs = pctx.cull_stats(reset=True)
    assert cs["scored_a"] == 0 and cs["scored_b"] == 0


# ---- extraction ---------------------------------------------------------------------------------
def _five_planes():
    return plane_cloud(40000, 5, seed=81)[0]


def _noise():
    return np.random.default_rng(82).uniform(-5.0, 5.0, size=(20000, 3)).astype(np.float32)


EXTRACT = {"planes": (_five_planes, 500), "noise": (_noise, 0)}
# (256 draws: on clouds this small the tiles are coarse, the first round of either setting culls
# about half the batch, scores more than D / 16 and the later rounds run unculled)
EXTRACT_ITERS = {"planes": 255, "noise": 255}


@functools.lru_cache(maxsize=None)
def extract_reference(which, refit):
    make, min_inl = EXTRACT[which]
    return O.extract_planes(make(), THR, max_planes=4, min_inliers=min_inl,
                            max_iterations=EXTRACT_ITERS[which], probability=1.0, refit=refit)


def gpu_extract(ctx, cloud, which, refit, k):
    ctx.set_option(D.DLG_OPT_CULL, k)
    try:
        prm = D.make_params(THR, max_iterations=EXTRACT_ITERS[which], probability=1.0,
                            refit_mode=D.DLG_REFIT_FAST if refit == "fast" else D.DLG_REFIT_PCL)
        return D.extract_planes(cloud, prm, max_planes=4, min_inliers=EXTRACT[which][1])
    finally:
        ctx.set_option(D.DLG_OPT_CULL, 1)


def assert_same_extract(e, ref):
    assert e["n_planes"] == ref["n_planes"]
    assert np.array_equal(bits(e["coeffs"]), bits(ref["coeffs"]))
    assert np.array_equal(e["offsets"], ref["offsets"])
    assert np.array_equal(e["inliers"], ref["inliers"])


@pytest.mark.parametrize("refit", ("pcl", "fast"))
def test_extract_planes_every_setting(pctx, refit):
    """max_planes 4 of a five-plane cloud with DLG_OPT_CULL 0, 1, 2 and 1 again, each after a reset:
    coefficient bits, offsets and inlier ids equal the oracle's chain (hence each other's)."""
    ref = extract_reference("planes", refit)
    assert ref["n_planes"] == 4
    cloud = D.Cloud(pctx, _five_planes())
    try:
        for i, k in enumerate((0, 1, 2, 1)):
            if i:
                cloud.reset()  # (every extraction after the first starts from the reset list)
            pctx.cull_stats(reset=True)
            e = gpu_extract(pctx, cloud, "planes", refit, k)
            cs = pctx.cull_stats(reset=True)
            assert_same_extract(e, ref)
            if k == 0:
                assert not any(cs.values()), cs
            else:
                assert cs["rounds"] >= 1 and cs["culled"] > 0, cs
            if k == 2:
                assert cs["rounds_with_b"] >= 1 and cs["scored_b"] >= 1, cs
    finally:
        cloud.close()


def test_extract_noise_falls_back(pctx):
    """uniform noise: every hypothesis passes about as many tiles, the bound separates nothing,
    the first round scores nearly its whole batch and the rest of the call runs unculled --
    with the oracle's planes."""
    ref = extract_reference("noise", "pcl")
    cloud = D.Cloud(pctx, _noise())
    try:
        for again in (False, True):
            if again:
                cloud.reset()
            pctx.cull_stats(reset=True)
            e = gpu_extract(pctx, cloud, "noise", "pcl", 1)
            cs = pctx.cull_stats(reset=True)
            assert_same_extract(e, ref)
            assert cs["rounds"] == 1 and cs["fallbacks"] == 1, cs
            assert 2 * (cs["scored_a"] + cs["scored_b"]) > 256, cs
    finally:
        cloud.close()


# ---- axis-constrained model -----------------------------------------------------------------------
@pytest.mark.parametrize("k", (0, 1, 2))
def test_perpendicular_plane_mostly_invalid(pctx, k):
    """SACMODEL_PERPENDICULAR_PLANE in a room (floor + walls), axis z, 5 degrees: most good draws
    are wall or mixed planes that isModelValid rejects (NaN planes on the device: they pass no
    sphere test and count nothing)."""
    pts = R.room(16385)
    z, eps = (0.0, 0.0, 1.0), math.radians(5.0)
    ref = R.segment(pts, THR, model=R.PERP, axis=z, eps=eps, max_iterations=255, probability=1.0,
                    refit_mode="pcl")
    pctx.set_axis(z, eps)
    cloud = D.Cloud(pctx, pts)
    try:
        pctx.cull_stats(reset=True)
        inl, coeff, st = segment(pctx, cloud, k, model=R.PERP)
        cs = pctx.cull_stats(reset=True)
    finally:
        cloud.close()
        pctx.set_axis((0, 0, 0), 0.0)
    assert st["has_model"] and ref["ok"]
    assert list(st["best_sample"]) == list(ref["best_sample"])
    assert st["n_unrefined"] == ref["n_unrefined"]
    assert np.array_equal(bits(coeff), bits(ref["coeff"])) and np.array_equal(inl, ref["inliers"])
    if k:
        assert cs["rounds"] == 1 and cs["culled"] > 0, cs
