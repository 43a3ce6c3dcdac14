"""GPU (gfx950): the fused culled scoring (DLG_OPT_CULL_FUSE 1, the default: each selection in the
last workgroup of the launch before it) against the seven-launch sequence it replaces
(DLG_OPT_CULL_FUSE 0) and against the oracle.

The fused sequence must compute the same integers: the tile bound nt of every hypothesis (the
cascade hyper sphere -> super-tile sphere -> tile sphere defines it), the same candidate sets A and
B, the same exact counts and the same pick.  Held here:

  * the bound (DLG_SCORE_BOUND), element for element, on small clouds with partial tiles, partial
    super-tiles, non-finite points, index lists and no good draw, and on a 600100-point cloud whose
    hypers hold two super-tiles (from 1024 super-tiles, 524288 points, up on 256 CUs), the last
    hyper one, and whose bound pass runs more than one super-tile per wave;
  * the scored set (DLG_SCORE_CULLED), element for element with the -1 fills, for K on both sides
    of the wave size, every scored count the oracle's;
  * set A's tie rule (ties in the bound go to the lower index), fewer good draws than K, and
    exactly K;
  * no state left behind in the per-context scratch (stale tile counts, ticket words);
  * extraction: planes bit-equal to the oracle's chain and the counters of dlg_cull_stats equal
    under both settings, on a five-plane cloud, on noise (the fallback) and for an axis-constrained
    model in which most draws are invalid.

Clouds and helpers as in test_cull_gpu.py: every cloud is uploaded with DLG_OPT_PRUNE 1, and the
hypotheses dlg_score_benchmark draws are replayed on the host from Mt19937(777).
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
BIG_N = 600100  # 1173 super-tiles: H = 2, 587 hypers, the last of one super-tile; n = 4 (mod 32)


# ---- clouds: name -> (points, indices or None, threshold) ---------------------------------------
def _multi(n, seed):
    return plane_cloud(n, 5, sigma=0.01, seed=seed)[0], None, THR


def _coplanar_q():
    # exactly coplanar, quantised: every good draw is the same plane and counts all n points
    n = 20031
    rng = np.random.default_rng(73)
    p = np.empty((n, 3), np.float32)
    p[:, :2] = rng.integers(-400, 401, size=(n, 2)) * 0.125
    p[:, 2] = 0.5
    return p, None, THR


def _coplanar_full():
    # the same with every tile full: every tied draw's bound equals its count
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
    "multi": functools.partial(_multi, 20000, 71),
    "coplanar": _coplanar_q, "coplanar_full": _coplanar_full, "wide": _wide,
    "nonfinite": _nonfinite, "indexed": _indexed, "collinear": _collinear,
    "n513": functools.partial(_multi, 513, 77),    # two super-tiles, the second of one point
    "n8193": functools.partial(_multi, 8193, 78),  # just over 16 super-tiles
    "big": functools.partial(_multi, BIG_N, 79),   # GPU against GPU only
}
BOUND_CLOUDS = ("n513", "n8193", "multi", "nonfinite", "indexed", "wide", "collinear", "big")
CULL_CLOUDS = ("multi", "coplanar", "coplanar_full", "n8193")


@functools.lru_cache(maxsize=None)
def _stream():
    return O.rnd_stream(3 * DMAX, seed=777)


@functools.lru_cache(maxsize=None)
def reference(cloud):
    """the oracle's verdict and count of the DMAX replayed hypotheses (0 for a rejected sample),
    once per cloud; a smaller D's draw is a prefix"""
    pts, idx, thr = CLOUDS[cloud]()
    active = np.ascontiguousarray(pts if idx is None else pts[idx], np.float32)
    pos = (_stream()[:3 * DMAX] % active.shape[0]).reshape(DMAX, 3)
    ok = np.zeros(DMAX, bool)
    counts = np.zeros(DMAX, np.int64)
    for d in range(DMAX):
        ok[d], coef = O.plane_coefficients(*active[pos[d]])
        if ok[d]:
            counts[d] = O.count_within(active, coef, thr)
    ok.flags.writeable = counts.flags.writeable = False
    return ok, counts


def ref_head(cloud, n_hyp):
    ok, counts = reference(cloud)
    return ok[:n_hyp], counts[:n_hyp]


def new_ctx():
    ctx = D.Context(0)
    ctx.set_option(D.DLG_OPT_PRUNE, 1)
    return ctx


@pytest.fixture(scope="module")
def pctx():
    ctx = new_ctx()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def uploaded(pctx):
    held = {}

    def get(name):
        if name not in held:
            pts, idx, _ = CLOUDS[name]()
            held[name] = D.Cloud(pctx, pts, indices=idx)
        return held[name]
    yield get
    for c in held.values():
        c.close()


def bench_counts(ctx, cloud, n_hyp, kernel, thr, k=1, fuse=1):
    ms = C.c_double()
    out = np.full(n_hyp, -7, np.int32)
    ctx.set_option(D.DLG_OPT_CULL, k)
    ctx.set_option(D.DLG_OPT_CULL_FUSE, fuse)
    try:
        ctx.check(_lib.load().dlg_score_benchmark(ctx.h, cloud.h, n_hyp, kernel, 1, thr, C.byref(ms),
                                                  out.ctypes.data_as(C.POINTER(C.c_int32))))
    finally:
        ctx.set_option(D.DLG_OPT_CULL, 1)
        ctx.set_option(D.DLG_OPT_CULL_FUSE, 1)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def set_a(bound, ok, k):
    """the K good hypotheses with the largest bound, ties to the lower index"""
    good = np.flatnonzero(ok)
    order = good[np.lexsort((good, -bound[good].astype(np.int64)))]
    return set(int(i) for i in order[:k])


def test_default_is_fused(pctx):
    assert pctx.get_option(D.DLG_OPT_CULL_FUSE) == 1


# ---- 1. the bound ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hyp", (48, 256, DMAX))
@pytest.mark.parametrize("name", BOUND_CLOUDS)
def test_bound_equals_unfused(pctx, uploaded, name, n_hyp):
    thr = CLOUDS[name]()[2]
    fused = bench_counts(pctx, uploaded(name), n_hyp, D.DLG_SCORE_BOUND, thr, fuse=1)
    plain = bench_counts(pctx, uploaded(name), n_hyp, D.DLG_SCORE_BOUND, thr, fuse=0)
    again = bench_counts(pctx, uploaded(name), n_hyp, D.DLG_SCORE_BOUND, thr, fuse=1)
    diff = np.flatnonzero(fused != plain)
    assert diff.size == 0, [(int(i), int(fused[i]), int(plain[i])) for i in diff[:4]]
    assert np.array_equal(again, plain)  # (after the unfused sequence left its tile counts behind)
    assert (plain >= 0).all() and (plain % TILE == 0).all()
    if name == "collinear":
        assert not plain.any()
    else:
        assert plain.max() > 0


def test_big_cloud_scored_set(pctx, uploaded):
    """the 600100-point cloud, culled counts: GPU against GPU"""
    fused = bench_counts(pctx, uploaded("big"), DMAX, D.DLG_SCORE_CULLED, THR, 64, fuse=1)
    plain = bench_counts(pctx, uploaded("big"), DMAX, D.DLG_SCORE_CULLED, THR, 64, fuse=0)
    assert np.array_equal(fused, plain)
    assert (plain >= 0).sum() >= 64


# ---- 2. the scored set ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_hyp", (48, 256, DMAX))
@pytest.mark.parametrize("k", (2, 63, 64, 65, DMAX))
@pytest.mark.parametrize("name", CULL_CLOUDS)
def test_scored_set_equals_unfused(pctx, uploaded, name, k, n_hyp):
    thr = CLOUDS[name]()[2]
    ok, counts = ref_head(name, n_hyp)
    fused = bench_counts(pctx, uploaded(name), n_hyp, D.DLG_SCORE_CULLED, thr, k, fuse=1)
    plain = bench_counts(pctx, uploaded(name), n_hyp, D.DLG_SCORE_CULLED, thr, k, fuse=0)
    diff = np.flatnonzero(fused != plain)
    assert diff.size == 0, [(int(i), int(fused[i]), int(plain[i])) for i in diff[:4]]
    assert ((fused >= 0) | (fused == -1)).all()
    scored = fused >= 0
    assert not (scored & ~ok).any()
    wrong = np.flatnonzero(scored & (fused != counts))
    assert wrong.size == 0, [(int(i), int(fused[i]), int(counts[i])) for i in wrong[:4]]
    best = int(counts[ok].max())
    assert fused[int(np.flatnonzero(ok & (counts == best))[0])] == best
    assert scored.sum() >= min(k, int(ok.sum()))


# ---- 3. set A's tie rule --------------------------------------------------------------------------
def test_set_a_ties_go_to_the_lower_index(pctx, uploaded):
    ok, counts = ref_head("multi", DMAX)
    bound = bench_counts(pctx, uploaded("multi"), DMAX, D.DLG_SCORE_BOUND, THR)
    good = np.flatnonzero(ok)
    order = good[np.lexsort((good, -bound[good].astype(np.int64)))]
    b = bound[order]
    # K >= 2 (DLG_OPT_CULL 1 means 64) with the K-th and (K+1)-th bounds equal
    ties = [k for k in range(2, order.size) if b[k - 1] == b[k]]
    assert ties, "no tie among the bounds"
    # the smallest, one near the wave size if there is one, and the largest
    picks = sorted({ties[0], min(ties, key=lambda k: abs(k - 64)), ties[-1]})
    for k in picks:
        got = bench_counts(pctx, uploaded("multi"), DMAX, D.DLG_SCORE_CULLED, THR, k)
        scored = set(int(i) for i in np.flatnonzero(got >= 0))
        a = set_a(bound, ok, k)
        assert len(a) == k and a <= scored, (k, sorted(a - scored)[:4])
        # the tied hypothesis just outside A is scored only if pass B takes it
        nxt = int(order[k])
        best_a = max(int(counts[i]) for i in a)
        assert (nxt in scored) == (int(bound[nxt]) >= best_a)


def test_set_a_with_few_good_draws(pctx, uploaded):
    # fewer good draws than K: all of them
    ok, counts = ref_head("multi", 48)
    got = bench_counts(pctx, uploaded("multi"), 48, D.DLG_SCORE_CULLED, THR, 64)
    assert 0 < ok.sum() < 64 and np.array_equal(got >= 0, ok) and np.array_equal(got[ok], counts[ok])
    # exactly K good draws: all of them, nothing left for pass B
    ok, counts = ref_head("multi", 256)
    k = int(ok.sum())
    assert 2 <= k <= 256
    got = bench_counts(pctx, uploaded("multi"), 256, D.DLG_SCORE_CULLED, THR, k)
    assert np.array_equal(got >= 0, ok) and np.array_equal(got[ok], counts[ok])


# ---- 4. state left behind -------------------------------------------------------------------------
def test_no_state_left_between_calls():
    """bound D = 4096, bound D = 48, bound D = 4096, culled counts D = 4096 on one context: each
    equals the same call on a fresh context"""
    pts = CLOUDS["multi"]()[0]
    calls = ((DMAX, D.DLG_SCORE_BOUND), (48, D.DLG_SCORE_BOUND), (DMAX, D.DLG_SCORE_BOUND),
             (DMAX, D.DLG_SCORE_CULLED))
    fresh = {}
    for call in set(calls):
        ctx = new_ctx()
        cloud = D.Cloud(ctx, pts)
        try:
            fresh[call] = bench_counts(ctx, cloud, call[0], call[1], THR, 64)
        finally:
            cloud.close()
            ctx.close()
    ctx = new_ctx()
    cloud = D.Cloud(ctx, pts)
    try:
        for i, call in enumerate(calls):
            got = bench_counts(ctx, cloud, call[0], call[1], THR, 64)
            assert np.array_equal(got, fresh[call]), (i, call)
        # and a second culled call after the first (its tile counts cleared, its tickets reset)
        got = bench_counts(ctx, cloud, DMAX, D.DLG_SCORE_CULLED, THR, 64)
        assert np.array_equal(got, fresh[(DMAX, D.DLG_SCORE_CULLED)])
    finally:
        cloud.close()
        ctx.close()


# ---- 5. rounds ------------------------------------------------------------------------------------
def _five_planes():
    return plane_cloud(40000, 5, seed=81)[0]


def _noise():
    return np.random.default_rng(82).uniform(-5.0, 5.0, size=(20000, 3)).astype(np.float32)


EXTRACT = {"planes": (_five_planes, 500), "noise": (_noise, 0)}


@functools.lru_cache(maxsize=None)
def extract_reference(which, refit):
    make, min_inl = EXTRACT[which]
    return O.extract_planes(make(), THR, max_planes=4, min_inliers=min_inl, max_iterations=255,
                            probability=1.0, refit=refit)


def gpu_extract(ctx, cloud, which, refit, fuse):
    ctx.set_option(D.DLG_OPT_CULL_FUSE, fuse)
    try:
        prm = D.make_params(THR, max_iterations=255, probability=1.0,
                            refit_mode=D.DLG_REFIT_FAST if refit == "fast" else D.DLG_REFIT_PCL)
        return D.extract_planes(cloud, prm, max_planes=4, min_inliers=EXTRACT[which][1])
    finally:
        ctx.set_option(D.DLG_OPT_CULL_FUSE, 1)


def assert_same_extract(e, ref):
    assert e["n_planes"] == ref["n_planes"]
    assert np.array_equal(bits(e["coeffs"]), bits(ref["coeffs"]))
    assert np.array_equal(e["offsets"], ref["offsets"])
    assert np.array_equal(e["inliers"], ref["inliers"])


@pytest.mark.parametrize("which", ("planes", "noise"))
def test_extract_both_settings(pctx, which):
    """both refit modes, DLG_OPT_CULL_FUSE 1, 0 and 1 again with a reset between: the oracle's
    planes and equal dlg_cull_stats counters"""
    cloud = D.Cloud(pctx, EXTRACT[which][0]())
    try:
        first = True
        for refit in ("pcl", "fast"):
            ref = extract_reference(which, refit)
            stats = []
            for fuse in (1, 0, 1):
                if not first:
                    cloud.reset()
                first = False
                pctx.cull_stats(reset=True)
                e = gpu_extract(pctx, cloud, which, refit, fuse)
                stats.append(pctx.cull_stats(reset=True))
                assert_same_extract(e, ref)
            assert stats[0] == stats[1] == stats[2], stats
            assert stats[0]["rounds"] >= 1 and stats[0]["scored_a"] >= 1, stats[0]
            if which == "noise":
                assert stats[0]["rounds"] == 1 and stats[0]["fallbacks"] == 1, stats[0]
            else:
                assert stats[0]["culled"] > 0, stats[0]
    finally:
        cloud.close()


def test_perpendicular_plane_mostly_invalid(pctx):
    """SACMODEL_PERPENDICULAR_PLANE in a room, axis z, 5 degrees: most good draws are planes that
    isModelValid rejects (NaN planes on the device: they pass no sphere test)"""
    pts = R.room(16385)
    z, eps = (0.0, 0.0, 1.0), math.radians(5.0)
    ref = R.segment(pts, THR, model=R.PERP, axis=z, eps=eps, max_iterations=255, probability=1.0,
                    refit_mode="pcl")
    pctx.set_axis(z, eps)
    cloud = D.Cloud(pctx, pts)
    stats = []
    try:
        for i, fuse in enumerate((1, 0)):
            if i:
                cloud.reset()
            pctx.set_option(D.DLG_OPT_CULL_FUSE, fuse)
            pctx.cull_stats(reset=True)
            prm = D.make_params(THR, max_iterations=255, probability=1.0, refit_mode=D.DLG_REFIT_PCL,
                                model=R.PERP)
            inl, coeff, st = D.segment_cloud(cloud, prm)
            stats.append(pctx.cull_stats(reset=True))
            assert st["has_model"] and ref["ok"]
            assert list(st["best_sample"]) == list(ref["best_sample"])
            assert st["n_unrefined"] == ref["n_unrefined"]
            assert np.array_equal(bits(coeff), bits(ref["coeff"])) and np.array_equal(inl, ref["inliers"])
    finally:
        pctx.set_option(D.DLG_OPT_CULL_FUSE, 1)
        cloud.close()
        pctx.set_axis((0, 0, 0), 0.0)
    assert stats[0] == stats[1] and stats[0]["rounds"] == 1 and stats[0]["culled"] > 0, stats
