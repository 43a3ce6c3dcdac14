"""Every SACMODEL_NORMAL_PLANE scorer's per-hypothesis counts against the oracle (all D draws).

The counterpart of tests/test_score_counts_oracle.py for model 11: the exhaustive k_score_np
(kernels.hip), the default pruned k_score_tiles_ex<NPM> and DLG_TILE_BF16's k_score_tiles_rl<NPM>
(spatial.hip), each with its own queue, drain and slot encoding, all sharing np_dev.hpp (the
prefilter as one float compare against np_de_limit, the float-acos fast decision of np_full with
its 4e-4 band and PCL's double arithmetic inside it) and make_plan's gate (the pruned scorer only
when every finite curvature gives w = lambda (1 - curvature) in [0, 1)).  dlg_score_samples returns
every draw's count; the draws are RansacControl's first batch, and every count is held against

  (a) the oracle: axis_ref.score over plane_coefficients' twin + count_within_np, array-equal
      (counts, good, valid, coefficient bits);
  (b) a float64 bracket lo <= count <= hi that knows nothing of the float op order, of the
      prefilter nor of the fast band: from the float inputs in float64, de = |P.c[:3] + c[3]|,
      S = |P| |c[:3]| + |c[3]|, rad = n^.c^ (both normalised in float64; a zero vector gives
      rad = 0), dn = acos(|rad|), w = lambda (1 - curvature), v = |w dn + (1 - w) de|, and
      E = |1 - w| 8 u S + |w| Ddn + 1e-15 (u = 2^-24) with Ddn = max(acos(|rad| - d) - dn,
      dn - acos(|rad| + d)) clamped to [0, 1], d = 16 u (two float normalisations and the 4-term
      float dot): lo = #(v < thr - E), hi = #(v < thr + E).  A pair with a NaN anywhere counts in
      neither.  A case's bracket must be tight: sum(hi - lo) <= 1 % of its tests;
  (c) analytic counts where every test is a tie (the NP "slab" clouds): floor hypotheses
      (0, 0, +-1, 0) over layers |z| in {0, 0.25, nextbelow(0.25)} with w = 0.5 exactly --
      parallel normals (dn = 0: 0.5 |z| against thr 0.125, a tie of the prefilter's own compare)
      and perpendicular normals (rad = 0, dn = acos(0) = M_PI - dn: thr the double
      v0 = 0.5 (pi/2) + 0.125 leaves |z| = 0.25 out, nextafter(v0) takes it in).  A third slab
      has its tie where thr / (1 - w) = 0.02 is no float and (float)0.02 lies below it: the layer
      |z| = (float)0.02 is an inlier, which a prefilter limit taken without np_de_limit's search
      would drop.

Beside the issue's clouds: `band01k` puts its band points within +-w 5e-7 of thr, just above the
inputs' own rounding, where a float acos verdict differs from the double one on some tens of a
floor hypothesis's 3600 pairs (the `band` clouds' +-8e-4 w is too wide for that); `gate_spread` spreads w over [0.09, 0.9] with inliers at d_euclid 0.3 that only
the limit of the LARGEST w keeps in a dense cloud (make_plan's use of np_lim_max's monotonicity).

test_reference_is_consistent (no GPU) runs (a) through (b) and (c) and asserts the conditions under
which a comparison means something (non-trivial counts, prefilter rejections, pairs decided outside
the band, thousands of in-band pairs of both verdicts on the `band` clouds, rejected samples and
zero planes at tiny n), so the GPU tests compare with a reference that was itself checked.
DLG_OPT_PRUNE_STATS proves which kernel ran: pairs > 0 where the gate admits the pruned scorer,
pairs < tiles * D where it must prune, pairs == 0 where the exhaustive kernel must take over.
"""
import functools
import math
from typing import NamedTuple

import numpy as np
import pytest

import dialog_amd as D
from dialog_amd.synth import plane_cloud
from oracle import oracle as O

import axis_ref as R
from test_axis_models_gpu import draws, run_ranks
from test_normal_plane import np_twin_dist
from test_score_counts_oracle import (AMBIGUOUS_CAP, BELOW, EXTRACT_KW, EXTRACT_MIN_INLIERS,
                                      SLAB_LAYERS, TILE_POINTS, TINY_N, U, _extract_oracle,
                                      slab_hypotheses, zero_planes)

DMAX = 4096
NP = D.SACMODEL_NORMAL_PLANE
THR = 0.05
THR_TINY = 0.2  # n <= TINY_N: a zero plane's w pi/2 <= 0.157 lies below it (counts every point)
BAND = 4e-4     # np_full's fast-decision band, per unit of w
DELTA = 16 * U
ONE_BELOW = math.nextafter(1.0, 0.0)
V0_PERP = 0.5 * math.acos(0.0) + 0.5 * 0.25  # the perpendicular slab's value at |z| = 0.25


class Cloud(NamedTuple):
    points: np.ndarray
    normals: np.ndarray  # [n, 4] (nx, ny, nz, curvature), one record per point
    idx: object          # the active list (ids into points) or None
    thr: float
    lam: float


def generator_normals(lab, planes, seed, curv=(0.0, 0.3)):
    """the generator plane's normal plus noise (random directions on the outliers), not
    normalised to the last bit; curvature uniform in `curv`"""
    rng = np.random.default_rng(seed)
    n = lab.shape[0]
    v = rng.normal(size=(n, 3))
    inl = lab >= 0
    v[inl] = planes[lab[inl], :3] + rng.normal(scale=0.05, size=(int(inl.sum()), 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    nrm = np.empty((n, 4), np.float32)
    nrm[:, :3] = v
    nrm[:, 3] = rng.uniform(curv[0], curv[1], n)
    return nrm


def _plane_np(n, planes, sigma, seed):
    p, lab, pl = plane_cloud(n, planes, sigma=sigma, seed=seed)
    return p, generator_normals(lab, pl, seed + 1000)


def _sized(n):
    p, nrm = _plane_np(n, 2, 0.01, 700 + n)
    if n <= TINY_N:
        # a third of the points are copies of point 0 (the draws' positions are distinct): draws
        # (copy, copy, k) are rejected (ratios 0, 0, 0), draws (copy, m, copy) are accepted (ratios
        # +inf, -inf, +inf) with a zero cross product
        m = max(2, n // 3)
        p[1:m], nrm[1:m] = p[0], nrm[0]
        p[m] = p[0] + np.array([0.5, -0.25, 0.75], np.float32)
        return Cloud(p, nrm, None, THR_TINY, 0.1)
    return Cloud(p, nrm, None, THR, 0.1)


def _noisy(lam=0.1):
    p, nrm = _plane_np(5003, 5, 0.015, 111)
    return Cloud(p, nrm, None, THR, lam)


def _far():
    p, nrm = _plane_np(5003, 5, 0.015, 112)
    return Cloud((p + np.float32(1000.0)).astype(np.float32), nrm, None, THR, 0.1)


def _quantised():
    p, nrm = _plane_np(5003, 4, 0.01, 116)
    nrm[:, :3] = np.round(nrm[:, :3] * 4) / 4  # (some become zero normals)
    return Cloud((np.round(p * 8) / 8).astype(np.float32), nrm, None, THR, 0.1)


def _nonfinite():
    p, nrm = _plane_np(5003, 4, 0.01, 113)
    p[::7, 0] = np.nan
    p[3::11, 2] = np.inf
    nrm[5::13] = np.nan       # NaN normal records
    nrm[2::17, :3] = 0.0      # zero normals
    nrm[4::19, 3] = np.nan    # NaN curvature
    nrm[6::23, 1] = np.nan    # one NaN component
    return Cloud(p, nrm, None, THR, 0.1)


def _antiparallel():
    p, lab, pl = plane_cloud(5003, 4, sigma=0.01, seed=117)
    nrm = generator_normals(lab, pl, 1117)
    flip = (lab >= 0) & (np.arange(lab.shape[0]) % 2 == 0)
    nrm[flip, :3] = -nrm[flip, :3]
    return Cloud(p, nrm, None, THR, 0.1)


def _indexed():
    p, nrm = _plane_np(5000, 4, 0.01, 143)
    idx = np.random.default_rng(9).choice(5000, 3000, replace=False).astype(np.int32)  # unsorted
    return Cloud(p, nrm, idx, THR, 0.1)


# a third slab: thr / (1 - w) = 0.02 is no float and (float)0.02 lies below it, so the prefilter's
# limit is the next float up: the layer |z| = (float)0.02 passes (0.5 |z| < 0.01), the next one ties
LIM_IN = np.float32(0.02)
LIM_OUT = np.nextafter(LIM_IN, np.float32(1.0))
LIM_LAYERS = np.array([0.0, 0.0, 0.0, 0.0, LIM_OUT, -LIM_OUT, LIM_IN, -LIM_IN], np.float32)
assert 0.5 * float(LIM_IN) < 0.01 <= 0.5 * float(LIM_OUT)


def _slab(perp, thr, layers=SLAB_LAYERS):
    # x, y multiples of 0.125; z on the layers; normals exactly parallel or perpendicular to the
    # floor hypotheses' (0, 0, +-1), curvature 0 and lambda 0.5: w = 0.5 exactly
    n = 1537
    rng = np.random.default_rng(21)
    p = np.empty((n, 3), np.float32)
    p[:, :2] = rng.integers(-32, 33, size=(n, 2)) * 0.125
    p[:, 2] = layers[np.arange(n) % layers.size]
    nrm = np.zeros((n, 4), np.float32)
    nrm[:, 0 if perp else 2] = 1.0
    return Cloud(p, nrm, None, thr, 0.5)


def _band(lam, knife=False):
    """a z = 0 floor that carries the hypotheses; band points at heights z_i with normals tilted
    by theta_i about a horizontal axis such that w theta_i + (1 - w) |z_i| = thr + delta_i, delta_i
    uniform over +-2 (w 4e-4): for a floor hypothesis half of them fall inside np_full's band
    (PCL's double arithmetic decides), a quarter on either side of it.  Curvature 0: w = lambda.
    knife: a smaller floor (all its hypotheses are the same plane, so each band point is one
    distinct pair), theta_i in [0.2, 0.4] and delta_i within +-w 5e-7, just above the w 2e-7 that
    the normals' own float rounding moves w theta_i by: a float acos verdict, off by up to half a
    float ulp of theta_i, then differs from the double one on some tens of the pairs."""
    n, n_floor = 5003, 1000 if knife else 2000
    n_band = n - n_floor - 403
    rng = np.random.default_rng(31)
    w = lam
    p = np.empty((n, 3), np.float64)
    v = rng.normal(size=(n, 3))  # (the outliers' normals)
    p[:n_floor, :2] = rng.integers(-32, 33, size=(n_floor, 2)) * 0.125
    p[:n_floor, 2] = 0.0
    v[:n_floor] = (0.0, 0.0, 1.0)
    b = slice(n_floor, n_floor + n_band)
    theta = rng.uniform(0.2 if knife else 0.02, min(0.4, 0.8 * THR / w), n_band)
    delta = rng.uniform(-1.0, 1.0, n_band) * (w * (5e-7 if knife else 2.0 * BAND))
    phi = rng.uniform(0.0, 2.0 * math.pi, n_band)
    p[b, :2] = rng.uniform(-4.0, 4.0, size=(n_band, 2))
    p[b, 2] = (THR + delta - w * theta) / (1.0 - w) * rng.choice([-1.0, 1.0], n_band)
    v[b] = np.c_[np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)]
    o = slice(n_floor + n_band, n)
    p[o] = np.c_[rng.uniform(-4.0, 4.0, size=(n - n_floor - n_band, 2)),
                 rng.uniform(0.5, 2.0, n - n_floor - n_band)]
    v[o] /= np.linalg.norm(v[o], axis=1, keepdims=True)
    perm = rng.permutation(n)
    nrm = np.zeros((n, 4), np.float32)
    nrm[:, :3] = v[perm]
    return Cloud(np.ascontiguousarray(p[perm], np.float32), nrm, None, THR, lam)


def _gate(kind):
    """the noisy cloud's points with curvatures / weights on either side of make_plan's gate"""
    c = _noisy()
    nrm = c.normals.copy()
    rng = np.random.default_rng(51)
    lam = 0.1
    if kind == "curv":      # w = lambda (1 - curvature) in [-0.05, 0.15]: some below 0
        nrm[:, 3] = rng.uniform(-0.5, 1.5, nrm.shape[0])
    elif kind == "w1":      # a zero curvature with lambda = 1: w reaches 1
        nrm[100, 3] = 0.0
        lam = 1.0
    elif kind == "lam2":
        lam = 2.0
    elif kind == "edge":    # w_max = lambda (1 - 0) one double below 1: admitted, nothing pruned
        nrm[100, 3] = 0.0
        lam = ONE_BELOW
    elif kind == "negzero":
        nrm[::3, 3] = -0.0
    elif kind == "allnan":
        nrm[:, 3] = np.nan
    return Cloud(c.points, nrm, None, THR, lam)


def _gate_spread():
    """weights spread over [0.09, 0.9] (lambda 0.9, curvatures in [0, 0.9]): the prefilter limit
    of the largest w is 0.5, of the smallest 0.055.  Two dense parallel sheets 0.3 apart with clean
    normals: for a hypothesis on one sheet the other sheet's flat points (w near 0.9) are inliers
    at d_euclid 0.3 (0.9 dn + 0.1 * 0.3 < 0.05), in tiles a limit below 0.3 minus their radius
    would prune."""
    n, per = 5003, 2000
    rng = np.random.default_rng(61)
    p = rng.uniform(-0.5, 0.5, size=(n, 3))
    v = rng.normal(size=(n, 3))
    for k, z in enumerate((0.0, 0.3)):
        s = slice(k * per, (k + 1) * per)
        p[s, 2] = z + rng.normal(0.0, 0.003, per)
        v[s] = np.array([0.0, 0.0, 1.0]) + rng.normal(scale=0.01, size=(per, 3))
    p[2 * per:, 2] = rng.uniform(-2.0, 2.0, n - 2 * per)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    perm = rng.permutation(n)
    nrm = np.empty((n, 4), np.float32)
    nrm[:, :3] = v[perm]
    nrm[:, 3] = rng.uniform(0.0, 0.9, n)
    return Cloud(np.ascontiguousarray(p[perm], np.float32), nrm, None, THR, 0.9)


@functools.lru_cache(maxsize=None)
def _extract_cloud():
    p, lab, pl = plane_cloud(40000, 6, seed=41)  # (test_score_counts_oracle._extract_points())
    return p, generator_normals(lab, pl, 1041)


@functools.lru_cache(maxsize=None)
def _extract_np_oracle():
    """the oracle's first two NORMAL_PLANE planes of the extraction cloud, and what remains"""
    p, nrm = _extract_cloud()
    e = O.extract_planes(p, THR, max_planes=2, min_inliers=EXTRACT_MIN_INLIERS, normals=nrm,
                         normal_distance_weight=0.1, **EXTRACT_KW)
    assert e["n_planes"] == 2
    return e, np.setdiff1d(np.arange(p.shape[0]), e["inliers"]).astype(np.int32)


def _extract(which):
    p, nrm = _extract_cloud()
    idx = {"full": None, "np_rem": lambda: _extract_np_oracle()[1],
           "plane_rem": lambda: _extract_oracle()[1]}[which]
    return Cloud(p, nrm, idx() if idx else None, THR, 0.1)


SIZES = (3, 5, 31, 32, 33, 63, 64, 65, 511, 512, 513, 4097)
CLOUDS = {f"n{n}": functools.partial(_sized, n) for n in SIZES}
CLOUDS.update(noisy=_noisy, heavy=functools.partial(_noisy, 0.7),
              lam0=functools.partial(_noisy, 0.0), far=_far, quantised=_quantised, nonfinite=_nonfinite, antiparallel=_antiparallel,
              indexed=_indexed,
              slab_par=functools.partial(_slab, False, 0.125),
              slab_lim=functools.partial(_slab, False, 0.01, LIM_LAYERS),
              slab_perp_out=functools.partial(_slab, True, V0_PERP),
              slab_perp_in=functools.partial(_slab, True, math.nextafter(V0_PERP, math.inf)),
              band01=functools.partial(_band, 0.1), band07=functools.partial(_band, 0.7),
              band01k=functools.partial(_band, 0.1, True),
              extract_full=functools.partial(_extract, "full"),
              extract_np_rem=functools.partial(_extract, "np_rem"),
              extract_plane_rem=functools.partial(_extract, "plane_rem"))
CLOUDS.update(gate_spread=_gate_spread)
CLOUDS.update({f"gate_{k}": functools.partial(_gate, k)
               for k in ("curv", "w1", "lam2", "edge", "negzero", "allnan")})


class Case(NamedTuple):
    cloud: str
    D: int
    gate: str = "pruned"   # what make_plan must decide on the pruned paths: "pruned" (pairs > 0),
                           # "fallback" (the exhaustive kernel: pairs == 0) or "either"
    pruning: bool = False  # the pruned paths must rule pairs out: pairs < tiles * D
    general: bool = True   # the prefilter and outside-the-band conditions apply


# every n with D = 65 (the 32-point tile, the 64-lane drains, k_score_np<2, 256>'s 512-point chunk,
# the 512-point super-tile); every D at n = 513 and 4097 (the 64-pair drain, k_score_np's
# 256-hypothesis tile, the 4096 maximum); launch_score_np launches no other instantiation
CASES = [Case(f"n{n}", 65) for n in SIZES if n < 513]
CASES += [Case(f"n{n}", d) for n in (513, 4097) for d in (1, 63, 64, 65, 255, 256, 257, DMAX)]
CASES += [Case("noisy", 257, pruning=True), Case("heavy", 257), Case("lam0", 257),
          Case("far", 257, pruning=True), Case("quantised", 257),
          Case("nonfinite", 257, pruning=True), Case("antiparallel", 257), Case("indexed", 257),
          Case("slab_par", 257, general=False), Case("slab_perp_out", 257, general=False),
          Case("slab_perp_in", 257, general=False), Case("slab_lim", 257, general=False),
          Case("band01", 257), Case("band07", 257), Case("band01k", 257),
          Case("gate_curv", 257, "fallback", general=False),
          Case("gate_w1", 257, "fallback", general=False),
          Case("gate_lam2", 257, "fallback", general=False),
          Case("gate_edge", 257, "pruned", general=False), Case("gate_spread", 257, "pruned"),
          Case("gate_negzero", 257, "either"), Case("gate_allnan", 257, "either", general=False)]
LIST_D = 257
REF_D = {}
for _c in CASES:
    REF_D[_c.cloud] = max(REF_D.get(_c.cloud, 0), _c.D)
for _k in CLOUDS:
    REF_D.setdefault(_k, LIST_D)  # (the clouds of the list tests)


def case_id(c):
    return f"{c.cloud}-D{c.D}"


# ---- the references ------------------------------------------------------------------------------
class Ref(NamedTuple):
    active: np.ndarray   # the active points in list order
    nrm: np.ndarray      # their normal records
    thr: float
    lam: float
    n_finite: int        # finite points (what a spatial copy holds)
    n_pairable: int      # points without a NaN in the point or its normal record
    pos: np.ndarray      # [D, 3] list positions
    ok: np.ndarray       # isSampleGood
    coef: np.ndarray     # [D, 4] float32, NaN for a rejected sample
    counts: np.ndarray   # (a)
    lo: np.ndarray       # (b)
    hi: np.ndarray
    n_pref: np.ndarray   # per hypothesis: pairs the prefilter (1 - w) de >= thr rejects (float64)
    n_clear: np.ndarray  # pairs past the prefilter that np_full decides outside its band
    band_in: np.ndarray  # pairs inside the band, v < thr
    band_out: np.ndarray  # pairs inside the band, v >= thr
    n_wide: np.ndarray   # inliers with d_euclid above twice the limit of the cloud's smallest w

    def head(self, n_hyp):
        """the first n_hyp draws (a smaller batch is a prefix of a larger one)"""
        return self._replace(**{k: getattr(self, k)[:n_hyp]
                                for k in ("pos", "ok", "coef", "counts", "lo", "hi", "n_pref",
                                          "n_clear", "band_in", "band_out", "n_wide")})


def float64_bracket(active, nrm, coef, ok, thr, lam):
    """reference (b), and the float64 census of the prefilter and of np_full's band"""
    pair_ok = np.isfinite(active).all(axis=1) & ~np.isnan(nrm).any(axis=1)
    P = active[pair_ok].astype(np.float64)
    N = nrm[pair_ok, :3].astype(np.float64)
    w = (lam * (1.0 - nrm[pair_ok, 3].astype(np.float64)))[:, None]
    pn = np.linalg.norm(P, axis=1)[:, None]
    nn = np.linalg.norm(N, axis=1)[:, None]
    Nh = np.divide(N, nn, out=np.zeros_like(N), where=nn > 0)
    n_hyp = coef.shape[0]
    out = {k: np.zeros(n_hyp, np.int64) for k in ("lo", "hi", "n_pref", "n_clear", "band_in",
                                                   "band_out", "n_wide")}
    w_in = w[(w >= 0.0) & (w < 1.0)]
    lim_min = thr / (1.0 - w_in.min()) if w_in.size else math.inf
    with np.errstate(all="ignore"):
        for h0 in range(0, n_hyp, 256):  # (keeps the [points, planes] blocks small)
            c = coef[h0:h0 + 256].astype(np.float64)
            cn = np.linalg.norm(c[:, :3], axis=1)
            ch = np.divide(c[:, :3], cn[:, None], out=np.zeros_like(c[:, :3]),
                           where=cn[:, None] > 0)
            de = np.abs(P @ c[:, :3].T + c[:, 3])
            S = pn * cn + np.abs(c[:, 3])
            rad = np.minimum(np.abs(Nh @ ch.T), 1.0)
            dn = np.arccos(rad)
            ddn = np.maximum(np.arccos(np.clip(rad - DELTA, -1.0, 1.0)) - dn,
                             dn - np.arccos(np.clip(rad + DELTA, -1.0, 1.0)))
            ddn = np.clip(ddn, 0.0, 1.0)
            b = (1.0 - w) * de
            v = np.abs(w * dn + b)
            E = np.abs(1.0 - w) * 8.0 * U * S + np.abs(w) * ddn + 1e-15
            s = slice(h0, h0 + 256)
            out["lo"][s] = (v < thr - E).sum(axis=0)
            out["hi"][s] = (v < thr + E).sum(axis=0)
            pref = (w >= 0.0) & (w <= 1.0) & (b >= thr)
            e = w * BAND + 1e-12 + 1e-9 * np.abs(b)
            fast = (w >= 0.0) & ~pref
            inband = fast & (np.abs(v - thr) <= e)
            out["n_pref"][s] = pref.sum(axis=0)
            out["n_clear"][s] = (fast & ~inband).sum(axis=0)
            out["band_in"][s] = (inband & (v < thr)).sum(axis=0)
            out["band_out"][s] = (inband & ~(v < thr)).sum(axis=0)
            out["n_wide"][s] = ((v < thr) & (de > 2.0 * lim_min)).sum(axis=0)
    dead = ~ok | ~np.isfinite(coef).all(axis=1)
    for a in out.values():
        a[dead] = 0
    return out, int(pair_ok.sum())


@functools.lru_cache(maxsize=None)
def reference(cloud):
    """References (a) and (b) of a cloud's draws, computed once and shared (read-only)."""
    c = CLOUDS[cloud]()
    idx = None if c.idx is None else np.asarray(c.idx, np.int64)
    active = np.ascontiguousarray(c.points if idx is None else c.points[idx], np.float32)
    nrm = np.ascontiguousarray(c.normals if idx is None else c.normals[idx], np.float32)
    pos = draws(active.shape[0], REF_D[cloud])
    a = R.score(c.points, c.thr, pos, R.NORMAL_PLANE, active=idx, normals=c.normals, lam=c.lam)
    assert (a["valid"] == 1).all()  # (no isModelValid gate on this model)
    ok = a["good"] == 1
    b, n_pairable = float64_bracket(active, nrm, a["coeffs"], ok, c.thr, c.lam)
    out = Ref(active, nrm, c.thr, c.lam, int(np.isfinite(active).all(axis=1).sum()), n_pairable,
              pos, ok, a["coeffs"], a["counts"].astype(np.int64), **b)
    for arr in out:
        if isinstance(arr, np.ndarray):
            arr.flags.writeable = False
    return out


def slab_counts(ref, cloud):
    """reference (c): the count of a floor hypothesis (0, 0, +-1, 0) from the layer populations"""
    z = np.abs(ref.active[:, 2])
    if cloud == "slab_perp_in":  # thr one double above the |z| = 0.25 layer's value
        return int(z.size)
    inner = LIM_IN if cloud == "slab_lim" else BELOW
    return int((z == 0).sum() + (z == inner).sum())  # the outer layer ties with thr: no inlier


def count_violations(counts, ref, cloud):
    """references (b) and (c) and the degenerate models' counts, for any counts of ref's draws
    (the oracle's or a device path's) -> list of findings"""
    bad = []
    out = np.flatnonzero((counts < ref.lo) | (counts > ref.hi))
    if out.size:
        bad.append(("outside the float64 bracket", int(out.size),
                    [(int(i), int(ref.lo[i]), int(counts[i]), int(ref.hi[i])) for i in out[:4]]))
    if cloud.startswith("slab"):
        want = slab_counts(ref, cloud)
        wrong = np.flatnonzero(slab_hypotheses(ref) & (counts != want))
        if wrong.size:
            bad.append(("slab count", want, [(int(i), int(counts[i])) for i in wrong[:4]]))
    if cloud == "lam0":  # w = 0: the plane model's float test
        want = np.array([O.count_within(ref.active, ref.coef[i], ref.thr) if ref.ok[i] else 0
                         for i in range(ref.ok.size)])
        wrong = np.flatnonzero(counts != want)
        if wrong.size:
            bad.append(("lambda = 0 is not count_within", [(int(i), int(counts[i]), int(want[i]))
                                                           for i in wrong[:4]]))
    if cloud == "gate_allnan" and counts.any():  # NaN < thr: never an inlier
        bad.append(("NaN curvature counted", int(counts.sum())))
    return bad


def check_reference(ref, case):
    """the conditions under which a comparison with ref means something -> the ambiguous share"""
    cloud, n_hyp = case.cloud, ref.ok.size
    finite_plane = ref.ok & np.isfinite(ref.coef).all(axis=1)
    if cloud != "gate_allnan":
        assert ref.counts.sum() > 0
    if ref.active.shape[0] <= TINY_N:
        zp = zero_planes(ref)
        assert zp.sum() >= 1 and (~ref.ok).sum() >= 1, (int(zp.sum()), int((~ref.ok).sum()))
        # a zero plane: de = 0, rad = 0, v = w pi/2 < THR_TINY for every point
        assert np.array_equal(ref.counts[zp], np.full(zp.sum(), ref.n_pairable))
    assert 4 * finite_plane.sum() >= n_hyp, (int(finite_plane.sum()), n_hyp)
    if case.general and ref.active.shape[0] > 3:
        # (n = 3: every draw is a permutation of the same three points, which the tiny-n
        # condition above makes degenerate -- zero planes and rejected samples only)
        assert ref.n_pref.sum() >= 1 and ref.n_clear.sum() >= 1
    tests = max(1, n_hyp * ref.n_pairable)
    share = float((ref.hi - ref.lo).sum()) / tests
    if cloud.startswith("slab"):  # all ties by design: reference (c) decides them
        k = slab_hypotheses(ref)
        assert k.sum() >= 16, int(k.sum())
        c = ref.coef[k]
        assert (c[:, :2] == 0).all() and (np.abs(c[:, 2]) == 1).all() and (c[:, 3] == 0).all()
    else:
        assert share <= AMBIGUOUS_CAP, share
    if cloud.startswith("band"):
        k = slab_hypotheses(ref)  # (only the floor has z = 0 exactly)
        n_in, n_out = int(ref.band_in[k].sum()), int(ref.band_out[k].sum())
        assert n_in + n_out >= 1000, (n_in, n_out)
        assert min(n_in, n_out) >= 0.2 * (n_in + n_out), (n_in, n_out)
    if cloud == "gate_spread":  # inliers that only the largest w's limit keeps
        assert ref.n_wide.sum() >= 1000, int(ref.n_wide.sum())
    return share


@pytest.mark.parametrize("cloud", sorted(CLOUDS))
def test_reference_is_consistent(cloud):
    """No GPU: the oracle's counts (a) pass the float64 bracket (b) and the analytic counts (c),
    and every case's conditions hold.  Prints each case's ambiguous share and in-band census."""
    ref = reference(cloud)
    c = CLOUDS[cloud]()
    assert ref.active.shape[0] == (c.points.shape[0] if c.idx is None else len(c.idx))
    assert ref.pos.min() >= 0 and ref.pos.max() < ref.active.shape[0]
    cases = [k for k in CASES if k.cloud == cloud] or [Case(cloud, LIST_D)]
    for case in cases:
        assert np.array_equal(draws(ref.active.shape[0], case.D), ref.pos[:case.D])
        r = ref.head(case.D)
        share = check_reference(r, case)
        k = slab_hypotheses(r) if cloud.startswith("band") else np.ones(case.D, bool)
        print(f"{case_id(case)}: ambiguous share {share:.2e}, prefiltered {int(r.n_pref.sum())}, "
              f"in band {int(r.band_in[k].sum())} in + {int(r.band_out[k].sum())} out of "
              f"{int(k.sum())} hypotheses, clear {int(r.n_clear.sum())}, "
              f"wide {int(r.n_wide.sum())}")
        assert not count_violations(r.counts, r, cloud)


# ---- the device paths ----------------------------------------------------------------------------
DEFAULTS = {D.DLG_OPT_PRUNE: -1, D.DLG_OPT_PRUNE_NP: 1,
            D.DLG_OPT_PRUNE_TILE_SCORER: D.DLG_TILE_EXACT}


class Path(NamedTuple):
    name: str
    opts: dict
    pruned: bool  # a pruned NORMAL_PLANE scorer (when make_plan's gate admits it)


TILE_EX = Path("pruned/tile-exact", {}, True)
TILE_RL = Path("pruned/tile-bf16", {D.DLG_OPT_PRUNE_TILE_SCORER: D.DLG_TILE_BF16}, True)
NP_OFF = Path("prune-np-0", {D.DLG_OPT_PRUNE_NP: 0}, False)
EXHAUSTIVE = Path("exhaustive", {D.DLG_OPT_PRUNE: 0}, False)
# (the pruned paths first: the exhaustive kernel materialises a lean list's coordinates)
LIST_PATHS = [TILE_EX, TILE_RL, NP_OFF, EXHAUSTIVE]


@pytest.fixture(scope="module")
def morton_ctx():
    """a context of its own whose spatial copies are Morton-ordered (the option applies when a
    copy is built)"""
    ctx = D.Context(0)
    ctx.set_option(D.DLG_OPT_SPATIAL_CURVE, 0)
    assert ctx.get_option(D.DLG_OPT_SPATIAL_CURVE) == 0
    yield ctx
    ctx.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def device_score(ctx, cloud, ref, path):
    """dlg_score_samples on one path -> (its result, the pruned kernels' work counters)"""
    prm = D.make_params(ref.thr, model=NP, normal_distance_weight=ref.lam)
    for k, v in path.opts.items():
        ctx.set_option(k, v)
    ctx.set_option(D.DLG_OPT_PRUNE_STATS, 1)  # (clears the counters)
    try:
        got = D.score_samples(cloud, prm, ref.pos)
        stats = ctx.prune_stats(reset=True)
    finally:
        ctx.set_option(D.DLG_OPT_PRUNE_STATS, 0)
        for k in path.opts:
            ctx.set_option(k, DEFAULTS[k])
    return got, stats


def path_findings(ctx, cloud, ref, case, paths, tag=""):
    """every path's result against (a), (b) and (c), and the counters against the case's gate
    -> list of findings (empty: all as it must be)"""
    n_hyp = ref.ok.size
    tiles = -(-ref.n_finite // TILE_POINTS)
    scorable = bool((ref.ok & np.isfinite(ref.coef).all(axis=1)).any())
    nan = np.isnan(ref.coef)
    bad = []
    for path in paths:
        name = tag + path.name
        got, stats = device_score(ctx, cloud, ref, path)
        pairs = stats["pairs"]
        if not np.array_equal(got["good"], ref.ok.astype(np.int32)):
            bad.append((name, "good differs"))
        if not (got["valid"] == 1).all():
            bad.append((name, "valid is not all 1"))
        if not (np.array_equal(np.isnan(got["coeffs"]), nan)
                and np.array_equal(bits(got["coeffs"])[~nan], bits(ref.coef)[~nan])):
            bad.append((name, "coefficient bits differ"))
        diff = np.flatnonzero(got["counts"] != ref.counts)
        if diff.size:
            bad.append((name, "differs from the oracle", int(diff.size),
                        [(int(i), int(got["counts"][i]), int(ref.counts[i])) for i in diff[:4]]))
        bad += [(name,) + v for v in count_violations(got["counts"].astype(np.int64), ref,
                                                      case.cloud)]
        if not path.pruned or case.gate == "fallback":
            if pairs != 0:
                bad.append((name, "the pruned kernel ran", int(pairs)))
        elif case.gate == "pruned":
            if pairs == 0 and scorable:
                bad.append((name, "the pruned kernel did not run"))
            if case.pruning and not pairs < tiles * n_hyp:
                bad.append((name, "nothing pruned", int(pairs), tiles * n_hyp))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_counts_equal_oracle(gpu_ctx, morton_ctx, case):
    """Every NORMAL_PLANE scorer path's result for all D draws: counts, good, valid and
    coefficient bits equal to the oracle's, counts inside the float64 bracket and equal to the
    analytic slab counts; the prune counters show the kernel the case's gate demands.  The spatial
    copy is built before the normals are attached, and after."""
    c = CLOUDS[case.cloud]()
    ref = reference(case.cloud).head(case.D)
    check_reference(ref, case)
    bad = []

    def run(ctx, order, paths, tag=""):
        if order == "none":
            ctx.set_option(D.DLG_OPT_PRUNE, 0)  # (applies at upload: no spatial copy)
        try:
            cloud = D.Cloud(ctx, c.points, indices=c.idx)
        finally:
            ctx.set_option(D.DLG_OPT_PRUNE, -1)
        try:
            if order == "before":
                cloud.build_spatial()
            cloud.set_normals(c.normals)
            if order == "after":
                cloud.build_spatial()
            return path_findings(ctx, cloud, ref, case, paths, tag)
        finally:
            cloud.close()

    bad += run(gpu_ctx, "none", [EXHAUSTIVE])
    bad += run(gpu_ctx, "before", [TILE_EX, TILE_RL, NP_OFF])
    bad += run(gpu_ctx, "after", [TILE_EX, TILE_RL], "copy-after-normals/")
    bad += run(morton_ctx, "before", [TILE_EX], "morton/")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("rounds", ["normal_plane", "plane"])
def test_counts_after_extraction_and_reset(gpu_ctx, morton_ctx, rounds):
    """Two extraction rounds through the default lean path (NORMAL_PLANE rounds, or SACMODEL_PLANE
    rounds on a cloud that carries normals: the spatial copy's normals are compacted with it), then
    every scorer over the remaining list; after reset over the whole cloud again."""
    p, nrm = _extract_cloud()
    if rounds == "normal_plane":
        e_ref, rem_name = _extract_np_oracle()[0], "extract_np_rem"
        prm = D.make_params(THR, model=NP, normal_distance_weight=0.1, **EXTRACT_KW)
    else:
        e_ref, rem_name = _extract_oracle()[0], "extract_plane_rem"
        prm = D.make_params(0.02, **EXTRACT_KW)
    rem_case, full_case = Case(rem_name, LIST_D), Case("extract_full", LIST_D)
    rem_ref, full_ref = reference(rem_name), reference("extract_full")
    check_reference(rem_ref, rem_case)
    check_reference(full_ref, full_case)
    bad = []
    for ctx, tag in ((gpu_ctx, ""), (morton_ctx, "morton/")):
        paths = LIST_PATHS if ctx is gpu_ctx else [TILE_EX]
        cloud = D.Cloud(ctx, p)
        try:
            cloud.build_spatial()
            cloud.set_normals(nrm)
            e = D.extract_planes(cloud, prm, max_planes=2, min_inliers=EXTRACT_MIN_INLIERS)
            assert e["stats"]["lean_rounds"] == 2
            assert np.array_equal(e["inliers"], e_ref["inliers"])
            assert cloud.n_active == rem_ref.active.shape[0]
            bad += path_findings(ctx, cloud, rem_ref, rem_case, paths, tag + "remaining/")
            cloud.reset()
            assert cloud.n_active == p.shape[0]
            bad += path_findings(ctx, cloud, full_ref, full_case, paths, tag + "reset/")
        finally:
            cloud.close()
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("prune", [-1, 1])
@pytest.mark.parametrize("hyp_shard", [0, 1])
def test_counts_two_ranks(hyp_shard, prune):
    """Two loopback ranks, point-sharded (an uneven cut, the normals attached per shard) and
    hypothesis-sharded, without and with spatial copies: the one-rank reference's result."""
    c = CLOUDS["n4097"]()
    case = Case("n4097", 257, "either")
    ref = reference("n4097").head(257)
    check_reference(ref, case)
    cut = 1500

    def body(ctx, r):
        ctx.set_option(D.DLG_OPT_HYP_SHARD, hyp_shard)
        ctx.set_option(D.DLG_OPT_PRUNE, prune)
        if hyp_shard:
            cloud = D.Cloud(ctx, c.points)
            cloud.set_normals(c.normals)
        else:
            lo, hi = (0, cut) if r == 0 else (cut, c.points.shape[0])
            cloud = D.Cloud(ctx, c.points[lo:hi], id_base=lo)
            cloud.set_normals(c.normals[lo:hi])
        try:
            prm = D.make_params(ref.thr, model=NP, normal_distance_weight=ref.lam)
            return D.score_samples(cloud, prm, ref.pos)
        finally:
            cloud.close()

    nan = np.isnan(ref.coef)
    for got in run_ranks(2, body):
        assert np.array_equal(got["good"], ref.ok.astype(np.int32))
        assert (got["valid"] == 1).all()
        assert np.array_equal(np.isnan(got["coeffs"]), nan)
        assert np.array_equal(bits(got["coeffs"])[~nan], bits(ref.coef)[~nan])
        assert np.array_equal(got["counts"], ref.counts)


# ---- the select side of the same arithmetic ------------------------------------------------------
SELECT_KW = dict(max_iterations=100, probability=0.99)


@functools.lru_cache(maxsize=None)
def band_winner(cloud):
    """the oracle's unrefined winner on a band cloud -- a floor hypothesis -- and the inliers the
    numpy twin of the NORMAL_PLANE distance gives it"""
    c = CLOUDS[cloud]()
    r = O.sac_segment(c.points, c.thr, normals=c.normals, normal_distance_weight=c.lam,
                      optimize=False, **SELECT_KW)
    co = r["coeff"]
    assert r["ok"] and (co[:2] == 0).all() and abs(co[2]) == 1 and co[3] == 0
    inl = np.flatnonzero(np_twin_dist(co, c.points, c.normals, c.lam) < c.thr).astype(np.int32)
    assert np.array_equal(inl, r["inliers"])
    # the band is loaded: the winner decides thousands of pairs inside it
    ref = reference(cloud)
    k = np.flatnonzero(slab_hypotheses(ref))[0]
    assert ref.band_in[k] + ref.band_out[k] >= 1000 and ref.counts[k] == inl.size
    return r, inl


def test_band_winner_reference():
    for cloud in ("band01", "band07"):
        band_winner(cloud)


@pytest.mark.gpu
@pytest.mark.parametrize("cloud", ["band01", "band07"])
def test_select_on_the_band(gpu_ctx, cloud):
    """The select kernels share np_test / np_full with the scorers: the winner's inlier list of a
    band cloud (optimize off: the hypothesis's own coefficients) from segment() over a spatial
    copy, from a lean extraction round, with DLG_OPT_LEAN_ROUNDS 0 and with DLG_OPT_PRUNE 0."""
    c = CLOUDS[cloud]()
    r, inl = band_winner(cloud)
    prm = D.make_params(c.thr, model=NP, normal_distance_weight=c.lam, optimize=False, **SELECT_KW)

    def check(got_inl, got_coeff, what):
        assert np.array_equal(bits(got_coeff), bits(r["coeff"])), what
        assert np.array_equal(got_inl, inl), (what, got_inl.size, inl.size)

    def extract(lean, prune):
        gpu_ctx.set_option(D.DLG_OPT_LEAN_ROUNDS, lean)
        gpu_ctx.set_option(D.DLG_OPT_PRUNE, prune)
        try:
            cl = D.Cloud(gpu_ctx, c.points)
            try:
                if prune:
                    cl.build_spatial()
                cl.set_normals(c.normals)
                s_inl, s_coeff, st = D.segment_cloud(cl, prm)
                assert st["iterations"] == r["iterations"]
                check(s_inl, s_coeff, ("segment", lean, prune))
                e = D.extract_planes(cl, prm, max_planes=1)
                assert e["n_planes"] == 1
                check(e["inliers"], e["coeffs"][0], ("extract", lean, prune))
                return e["stats"]["lean_rounds"]
            finally:
                cl.close()
        finally:
            gpu_ctx.set_option(D.DLG_OPT_LEAN_ROUNDS, 1)
            gpu_ctx.set_option(D.DLG_OPT_PRUNE, -1)

    assert extract(1, -1) == 1
    assert extract(0, -1) == 0
    assert extract(1, 0) == 0
