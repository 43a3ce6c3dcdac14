"""Every scorer's per-hypothesis counts against the oracle (countWithinDistance, all D hypotheses).

The end-to-end parity tests see only the winning hypothesis, and tests/test_score_variants.py
compares the scorers with one another; both stay green when a piece all scorers share (the
hypothesis build, the sample gather, thr_ceil, the spheres and prune margin, the compacted spatial
copy) moves every count the same way, or when a losing hypothesis is miscounted.  Here the
hypotheses dlg_score_benchmark draws are replayed on the host (the draw is part of its contract,
include/dialog_ransac.h) and every count is held against three references:

  (a) the oracle: plane_coefficients + count_within over the active points, array-equal;
  (b) a float64 bracket lo <= count <= hi that knows nothing of the oracle's float op order nor of
      thr_ceil: with dist = |P.c[:3] + c[3]| and S = |P| |c[:3]| + |c[3]| in float64, a 4-term
      float dot (3 products, 3 sums) of the same float inputs is within gamma_4 S ~ 4 u S
      (u = 2^-24) of dist, and E = 8 u S doubles that: lo = #(dist < thr - E),
      hi = #(dist < thr + E).  A case's bracket must be tight: sum(hi - lo) <= 1 % of its tests;
  (c) an analytic count for the strict `<` at exact equality (the "slab" cloud).

test_reference_is_consistent (no GPU) runs (a) through (b) and (c), so the GPU tests compare with
a reference that was itself checked.  The SACMODEL_NORMAL_PLANE scorers' counts are held to the
same three references, through dlg_score_samples, in tests/test_np_counts_oracle.py.
"""
import ctypes as C
import functools
from typing import NamedTuple

import numpy as np
import pytest

import dialog_amd as D
from dialog_amd.synth import plane_cloud
from oracle import oracle as O

DMAX = 4096
U = 2.0 ** -24
AMBIGUOUS_CAP = 0.01
TILE_POINTS = 32  # points per tile of the spatial copy
LIST_CHUNK = 1024  # super-tile plane-list entries the tile scorers hold in registers at a time
THR_SLAB = 0.25
BELOW = np.nextafter(np.float32(THR_SLAB), np.float32(0.0))  # largest float < 0.25
SLAB_LAYERS = np.array([0.0, 0.0, 0.0, 0.0, THR_SLAB, -THR_SLAB, BELOW, -BELOW], np.float32)
EXTRACT_KW = dict(max_iterations=200, probability=0.99)
EXTRACT_MIN_INLIERS = 100


# ---- clouds: name -> (points, indices or None, threshold) --------------------------------------
def _sized(n):
    p, _, _ = plane_cloud(n, 2, sigma=0.01, seed=600 + n)
    return p, None, 0.02


def _noisy():
    return plane_cloud(5003, 5, sigma=0.015, seed=11)[0], None, 0.02


def _far():
    p = plane_cloud(5003, 5, sigma=0.015, seed=12)[0]
    return (p + np.float32(1000.0)).astype(np.float32), None, 0.02


def _tiny():
    p = plane_cloud(3001, 3, sigma=0.01, seed=14)[0]
    return (p * np.float32(1e-3)).astype(np.float32), None, 2e-5


def _quantised():
    p = plane_cloud(5003, 4, sigma=0.01, seed=16)[0]
    return (np.round(p * 2) / 2).astype(np.float32), None, 0.25


def _slab():
    # x, y multiples of 0.125; z on five layers, half of the points on z = 0
    n = 1537
    rng = np.random.default_rng(21)
    p = np.empty((n, 3), np.float32)
    p[:, :2] = rng.integers(-32, 33, size=(n, 2)) * 0.125
    p[:, 2] = SLAB_LAYERS[np.arange(n) % SLAB_LAYERS.size]
    return p, None, THR_SLAB


def _coplanar():
    return plane_cloud(3001, 1, outlier_frac=0.0, sigma=0.0, seed=17)[0], None, 0.02


def _wide():
    return plane_cloud(5003, 6, sigma=0.01, seed=15)[0], None, 0.3


def _nonfinite():
    p = plane_cloud(5003, 4, sigma=0.01, seed=13)[0]
    p[::7, 0] = np.nan
    p[3::11, 2] = np.inf
    return p, None, 0.02


def _indexed():
    p = plane_cloud(5000, 4, sigma=0.01, seed=43)[0]
    idx = np.random.default_rng(9).choice(5000, 3000, replace=False).astype(np.int32)  # unsorted
    return p, idx, 0.02


def _extract_points():
    return plane_cloud(40000, 6, seed=41)[0]


@functools.lru_cache(maxsize=None)
def _extract_oracle():
    """the oracle's first two planes of the extraction cloud and its remaining list (PCL's order:
    the ascending set difference)"""
    p = _extract_points()
    e = O.extract_planes(p, 0.02, max_planes=2, min_inliers=EXTRACT_MIN_INLIERS, **EXTRACT_KW)
    assert e["n_planes"] == 2
    rem = np.setdiff1d(np.arange(p.shape[0]), e["inliers"]).astype(np.int32)
    return e, rem


def _extract_rem():
    return _extract_points(), _extract_oracle()[1], 0.02


def _extract_full():
    return _extract_points(), None, 0.02


SIZES = (3, 5, 31, 32, 33, 511, 512, 513, 4097)
TINY_N = 33  # up to here `% n` repeats positions in many draws
CLOUDS = {f"n{n}": functools.partial(_sized, n) for n in SIZES}
CLOUDS.update(noisy=_noisy, far=_far, tiny=_tiny, quantised=_quantised, slab=_slab,
              coplanar=_coplanar, wide=_wide, nonfinite=_nonfinite, indexed=_indexed,
              extract_rem=_extract_rem, extract_full=_extract_full)


class Case(NamedTuple):
    cloud: str
    D: int
    pruning: bool = False  # the pruned paths must rule pairs out: pairs < tiles * D
    long_lists: bool = False  # the super-tile plane lists must run past LIST_CHUNK entries


# every n with D = 65; every D with n = 513 and n = 4097 (64-plane groups, the 1024-entry list
# chunk, the 4096 maximum); the numeric edges at a few thousand points with partial tiles
CASES = [Case(f"n{n}", 65) for n in SIZES if n < 513]
CASES += [Case(f"n{n}", d) for n in (513, 4097) for d in (1, 63, 64, 65, 257, DMAX)]
CASES += [Case("noisy", 257, True), Case("far", 257, True), Case("tiny", 257),
          Case("quantised", 257), Case("slab", 257), Case("coplanar", 257),
          Case("wide", DMAX, True, True), Case("nonfinite", 257, True), Case("indexed", 257)]
EXTRACT_D = 257
REF_D = {"extract_rem": EXTRACT_D, "extract_full": EXTRACT_D}
for _c in CASES:
    REF_D[_c.cloud] = max(REF_D.get(_c.cloud, 0), _c.D)


def case_id(c):
    return f"{c.cloud}-D{c.D}"


# ---- host replay of dlg_score_benchmark's hypotheses -------------------------------------------
@functools.lru_cache(maxsize=None)
def _stream():
    return O.rnd_stream(3 * DMAX, seed=777)


def replay_positions(n_hyp, n_active):
    """dlg_score_benchmark's draw: position i of 3 * D is (uint32)rnd() % n_active over
    Mt19937(777), an index into the active list in list order, three per hypothesis."""
    return (_stream()[:3 * n_hyp] % n_active).reshape(n_hyp, 3)


class Ref(NamedTuple):
    active: np.ndarray  # the active points in list order
    thr: float
    n_finite: int
    pos: np.ndarray     # [D, 3] list positions
    ok: np.ndarray      # isSampleGood
    coef: np.ndarray    # [D, 4] float32
    counts: np.ndarray  # (a): the oracle's countWithinDistance, 0 for a rejected sample
    lo: np.ndarray      # (b)
    hi: np.ndarray

    def head(self, n_hyp):
        """the first n_hyp hypotheses (the draw of a smaller D is a prefix of a larger one's)"""
        return self._replace(**{k: getattr(self, k)[:n_hyp]
                                for k in ("pos", "ok", "coef", "counts", "lo", "hi")})


def float64_bracket(active, coef, ok, thr):
    finite = active[np.isfinite(active).all(axis=1)].astype(np.float64)
    pn = np.linalg.norm(finite, axis=1)
    lo = np.zeros(coef.shape[0], np.int64)
    hi = np.zeros(coef.shape[0], np.int64)
    with np.errstate(invalid="ignore"):
        for h0 in range(0, coef.shape[0], 256):  # (keeps the [points, planes] blocks small)
            c = coef[h0:h0 + 256].astype(np.float64)
            dist = np.abs(finite @ c[:, :3].T + c[:, 3])
            S = pn[:, None] * np.linalg.norm(c[:, :3], axis=1) + np.abs(c[:, 3])
            E = 8.0 * U * S
            lo[h0:h0 + 256] = (dist < thr - E).sum(axis=0)
            hi[h0:h0 + 256] = (dist < thr + E).sum(axis=0)
    lo[~ok] = 0
    hi[~ok] = 0
    return lo, hi, finite.shape[0]


@functools.lru_cache(maxsize=None)
def reference(cloud):
    """References (a) and (b) of a cloud's hypotheses, computed once and shared (read-only)."""
    pts, idx, thr = CLOUDS[cloud]()
    active = np.ascontiguousarray(pts if idx is None else pts[idx], np.float32)
    n_hyp = REF_D[cloud]
    pos = replay_positions(n_hyp, active.shape[0])
    ok = np.zeros(n_hyp, bool)
    coef = np.zeros((n_hyp, 4), np.float32)
    counts = np.zeros(n_hyp, np.int64)
    for d in range(n_hyp):
        ok[d], coef[d] = O.plane_coefficients(*active[pos[d]])
        if ok[d]:
            counts[d] = O.count_within(active, coef[d], thr)
    lo, hi, n_finite = float64_bracket(active, coef, ok, thr)
    for a in (active, pos, ok, coef, counts, lo, hi):
        a.flags.writeable = False
    return Ref(active, thr, n_finite, pos, ok, coef, counts, lo, hi)


def zero_planes(ref):
    """accepted samples with a zero normal (repeated positions through 0/0 = NaN, or collinear
    points): the plane (0, 0, 0, -0), which counts every finite point"""
    return ref.ok & (ref.coef[:, :3] == 0).all(axis=1)


def slab_hypotheses(ref):
    """slab cloud: hypotheses from three z = 0 points that span a triangle (the cross product's z
    is exact in float64 for these coordinates): the plane (0, 0, +-1, 0)"""
    s = ref.active[ref.pos].astype(np.float64)  # [D, 3 samples, xyz]
    a, b = s[:, 1] - s[:, 0], s[:, 2] - s[:, 0]
    return ref.ok & (s[:, :, 2] == 0).all(axis=1) & (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0] != 0)


def count_violations(counts, ref, cloud):
    """references (b) and (c), and the coplanar cloud's full count, for any counts of ref's
    hypotheses (the oracle's or a device path's) -> list of findings"""
    bad = []
    out = np.flatnonzero((counts < ref.lo) | (counts > ref.hi))
    if out.size:
        bad.append(("outside the float64 bracket", int(out.size),
                    [(int(i), int(ref.lo[i]), int(counts[i]), int(ref.hi[i])) for i in out[:4]]))
    if cloud == "slab":
        z = ref.active[:, 2]
        want = int((z == 0).sum() + (np.abs(z) == BELOW).sum())  # |z| = 0.25 is no inlier
        k = slab_hypotheses(ref)
        wrong = np.flatnonzero(k & (counts != want))
        if wrong.size:
            bad.append(("slab count", want, [(int(i), int(counts[i])) for i in wrong[:4]]))
    if cloud == "coplanar":
        wrong = np.flatnonzero(ref.ok & (counts != ref.active.shape[0]))
        if wrong.size:
            bad.append(("coplanar count", [(int(i), int(counts[i])) for i in wrong[:4]]))
    return bad


def check_reference(ref, cloud):
    """the conditions under which a comparison with ref means something"""
    n_hyp = ref.ok.size
    assert ref.counts.sum() > 0
    finite_plane = ref.ok & np.isfinite(ref.coef).all(axis=1)
    if ref.active.shape[0] <= TINY_N:
        # this path never reaches a winner end to end, and no sphere test may prune it
        assert zero_planes(ref).sum() >= 1 and (~ref.ok).sum() >= 1
        assert np.array_equal(ref.counts[zero_planes(ref)],
                              np.full(zero_planes(ref).sum(), ref.n_finite))
    else:
        assert 4 * finite_plane.sum() >= n_hyp, (int(finite_plane.sum()), n_hyp)
    share = float((ref.hi - ref.lo).sum()) / (n_hyp * ref.n_finite)
    if cloud == "slab":  # all ties by design: reference (c) decides it
        k = slab_hypotheses(ref)
        assert k.sum() >= 16, int(k.sum())
        c = ref.coef[k]
        assert (c[:, :2] == 0).all() and (np.abs(c[:, 2]) == 1).all() and (c[:, 3] == 0).all()
    else:
        assert share <= AMBIGUOUS_CAP, share
    return share


@pytest.mark.parametrize("cloud", sorted(CLOUDS))
def test_reference_is_consistent(cloud):
    """No GPU: the oracle's counts (a) pass the float64 bracket (b), the analytic slab and
    coplanar counts (c), and every case's conditions hold (non-trivial counts, a tight bracket,
    enough slab hypotheses, zero planes and rejected samples at tiny n)."""
    ref = reference(cloud)
    pts, idx, _ = CLOUDS[cloud]()
    assert ref.active.shape[0] == (pts.shape[0] if idx is None else idx.shape[0])
    assert ref.pos.min() >= 0 and ref.pos.max() < ref.active.shape[0]
    for n_hyp in sorted({c.D for c in CASES if c.cloud == cloud} | {REF_D[cloud]}):
        r = ref.head(n_hyp)
        check_reference(r, cloud)
        assert not count_violations(r.counts, r, cloud)


# ---- the device paths --------------------------------------------------------------------------
class Path(NamedTuple):
    name: str
    kernel: int
    tile_scorer: int
    morton: bool = False


PATHS = [Path("exact", D.DLG_SCORE_EXACT, D.DLG_TILE_EXACT),
         Path("bf16", D.DLG_SCORE_BF16, D.DLG_TILE_EXACT),
         Path("pruned/tile-exact", D.DLG_SCORE_PRUNED, D.DLG_TILE_EXACT),
         Path("pruned/tile-bf16", D.DLG_SCORE_PRUNED, D.DLG_TILE_BF16),
         Path("pruned/tile-mfma", D.DLG_SCORE_PRUNED, D.DLG_TILE_MFMA),
         Path("pruned/morton", D.DLG_SCORE_PRUNED, D.DLG_TILE_EXACT, morton=True)]


@pytest.fixture(scope="module")
def morton_ctx():
    """a context of its own whose spatial copies are Morton-ordered (the option applies when a
    copy is built)"""
    ctx = D.Context(0)
    ctx.set_option(D.DLG_OPT_SPATIAL_CURVE, 0)
    assert ctx.get_option(D.DLG_OPT_SPATIAL_CURVE) == 0
    yield ctx
    ctx.close()


def device_counts(ctx, cloud, n_hyp, path, thr):
    """dlg_score_benchmark(reps = 1) -> (counts, the pruned kernel's work counters)"""
    from dialog_amd import _lib
    ms = C.c_double()
    out = np.full(n_hyp, -1, np.int32)
    ctx.set_option(D.DLG_OPT_PRUNE_TILE_SCORER, path.tile_scorer)
    ctx.set_option(D.DLG_OPT_PRUNE_STATS, 1)  # (clears the counters)
    try:
        ctx.check(_lib.load().dlg_score_benchmark(ctx.h, cloud.h, n_hyp, path.kernel, 1, thr,
                                                  C.byref(ms),
                                                  out.ctypes.data_as(C.POINTER(C.c_int32))))
        stats = ctx.prune_stats(reset=True)
    finally:
        ctx.set_option(D.DLG_OPT_PRUNE_STATS, 0)
        ctx.set_option(D.DLG_OPT_PRUNE_TILE_SCORER, D.DLG_TILE_EXACT)
    return out, stats


def path_findings(ctx, cloud, ref, cloud_name, paths, pruning=False, long_lists=False):
    """every path's counts against (a), (b) and (c) -> list of findings (empty: all equal)"""
    n_hyp = ref.ok.size
    tiles = -(-ref.n_finite // TILE_POINTS)
    bad = []
    for path in paths:
        got, stats = device_counts(ctx, cloud, n_hyp, path, ref.thr)
        pairs = stats["pairs"]
        diff = np.flatnonzero(got != ref.counts)
        if diff.size:
            bad.append((path.name, "differs from the oracle", int(diff.size),
                        [(int(i), int(got[i]), int(ref.counts[i])) for i in diff[:4]]))
        bad += [(path.name,) + v for v in count_violations(got, ref, cloud_name)]
        if path.kernel == D.DLG_SCORE_PRUNED:
            if pairs == 0 and ref.counts.sum() > 0:
                bad.append((path.name, "no prune statistics"))
            if pruning and not pairs < tiles * n_hyp:
                bad.append((path.name, "nothing pruned", int(pairs), tiles * n_hyp))
            # (the lanes-as-planes scorers count every tile's list once: a mean length past the
            # chunk means lists that take several passes; the bf16 blocks count it per pass)
            if (long_lists and path.tile_scorer != D.DLG_TILE_BF16
                    and not stats["list_entries"] > LIST_CHUNK * tiles):
                bad.append((path.name, "short plane lists", int(stats["list_entries"]), tiles))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_counts_equal_oracle(gpu_ctx, morton_ctx, case):
    """Every scorer path's counts of all D replayed hypotheses: equal to the oracle's, inside the
    float64 bracket, the analytic counts on the slab and coplanar clouds; on the cases marked
    `pruning` the pruned paths scored fewer (tile, plane) pairs than there are, and on the one
    marked `long_lists` the plane lists ran past the register chunk."""
    pts, idx, _ = CLOUDS[case.cloud]()
    ref = reference(case.cloud).head(case.D)
    check_reference(ref, case.cloud)
    bad = []
    for ctx in (gpu_ctx, morton_ctx):
        cloud = D.Cloud(ctx, pts, indices=idx)
        try:
            cloud.build_spatial()
            bad += path_findings(ctx, cloud, ref, case.cloud,
                                 [p for p in PATHS if p.morton == (ctx is morton_ctx)],
                                 case.pruning, case.long_lists)
        finally:
            cloud.close()
    assert not bad, bad


@pytest.mark.gpu
def test_counts_after_extraction_and_reset(gpu_ctx, morton_ctx):
    """Two planes extracted through the default lean path, then the scorers over the remaining
    points: the list is materialised from the pristine copy for the exhaustive kernels, the pruned
    kernels read the compacted spatial copy with re-derived spheres.  After reset the counts over
    the whole cloud are back."""
    pts = _extract_points()
    e_ref, _ = _extract_oracle()
    rem_ref = reference("extract_rem")
    full_ref = reference("extract_full")
    check_reference(rem_ref, "extract_rem")
    check_reference(full_ref, "extract_full")
    prm = D.make_params(0.02, **EXTRACT_KW)
    bad = []
    for ctx in (gpu_ctx, morton_ctx):
        paths = [p for p in PATHS if p.morton == (ctx is morton_ctx)]
        cloud = D.Cloud(ctx, pts)
        try:
            cloud.build_spatial()
            e = D.extract_planes(cloud, prm, max_planes=2, min_inliers=EXTRACT_MIN_INLIERS)
            assert e["stats"]["lean_rounds"] == 2
            assert np.array_equal(e["inliers"], e_ref["inliers"])
            assert cloud.n_active == rem_ref.active.shape[0]
            bad += [("remaining",) + b
                    for b in path_findings(ctx, cloud, rem_ref, "extract_rem", paths)]
            cloud.reset()
            assert cloud.n_active == pts.shape[0]
            bad += [("reset",) + b
                    for b in path_findings(ctx, cloud, full_ref, "extract_full", paths)]
        finally:
            cloud.close()
    assert not bad, bad
