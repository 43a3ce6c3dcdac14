"""np_lim_max (dialog_amd/csrc/np_limit_host.hpp: the host restatement of np_de_limit, the
NORMAL_PLANE prefilter (1 - w) d_euclid >= thr as one float compare d_euclid >= lim) on the CPU
against its definition: lim is the smallest float x >= 0 with (1 - w) x >= thr as a double product.

The header finds it with a nextafter search from (float)(thr / (1 - w)); here the product's
monotonicity in x gives it by bisection over the bit patterns of the non-negative floats, and the
result is checked against the definition itself (it passes, its predecessor does not).  Swept:
w in {0, tiny, 0.1, 0.5, 1 - 2^-53, 1, > 1, < 0, NaN} and more, thr in {0, denormal, 5e-5, 0.05,
1e30, inf, NaN, negative} and more; and the monotonicity in w that make_plan relies on when it
takes the cloud's largest w for every point.
"""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF_BITS = 0x7F800000

W = [0.0, 5e-324, 1e-300, 2.0 ** -60, 0.1, 0.3, 0.5, 0.7, 0.9999999, 1.0 - 2.0 ** -53,
     1.0, 1.0 + 2.0 ** -52, 2.0, 1e30, math.inf, -0.0, -5e-324, -0.1, -math.inf, math.nan]
THRESHOLDS = [0.0, -0.0, 5e-324, 1e-310, 1e-45, 1e-40, 1.1754944e-38, 5e-5, 0.02, 0.05, 0.125,
              1.0, 3.0e38, 3.5e38, 1e30, 1e300, math.inf, math.nan, -0.05, -math.inf]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("npl") / "np_limit_host"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpp", "np_limit_host.cpp"), "-o", str(exe)],
                   check=True)
    return str(exe)


def host_limits(exe, pairs):
    text = "".join(f"{_c(w)} {_c(t)}\n" for w, t in pairs)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    bits = np.array([int(x, 16) for x in out.split()], np.uint32)
    assert bits.size == len(pairs)
    return bits


def _c(v):
    return "nan" if v != v else ("inf" if v == math.inf else "-inf" if v == -math.inf
                                 else float(v).hex())


def as_float(b):
    return float(np.array([b], np.uint32).view(np.float32)[0])


def passes(w, thr, b):
    """(1 - w) x >= thr as a double product, x the float with bit pattern b"""
    return (1.0 - w) * as_float(b) >= thr


def brute_limit(w, thr):
    """bit pattern of the smallest float x >= 0 with (1 - w) x >= thr, by the definition; None
    for a NaN result"""
    if not w >= 0.0 or not 1.0 - w > 0.0:
        return INF_BITS  # the prefilter does not apply: every d_euclid goes to the full test
    if thr != thr:
        return None
    if passes(w, thr, 0):
        return 0
    if not passes(w, thr, INF_BITS):
        return INF_BITS  # (cannot happen for 1 - w > 0 and a non-NaN thr)
    lo, hi = 0, INF_BITS  # fails at lo, passes at hi; non-negative floats order like their bits
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if passes(w, thr, mid) else (mid, hi)
    return hi


def test_limit_equals_its_definition(harness):
    rng = np.random.default_rng(3)
    pairs = [(w, t) for w in W for t in THRESHOLDS]
    pairs += [(float(w), float(t)) for w, t in zip(rng.uniform(0, 1, 2000),
                                                    10.0 ** rng.uniform(-6, 1, 2000))]
    # weights next to 1 and thresholds next to powers of two (the search starts on a rounding edge)
    pairs += [(1.0 - 2.0 ** -k, 2.0 ** -j) for k in range(1, 54, 4) for j in range(0, 30, 3)]
    pairs += [(0.5, math.nextafter(0.125, d)) for d in (0.0, 1.0)]
    got = host_limits(harness, pairs)
    for (w, thr), b in zip(pairs, got):
        want = brute_limit(w, thr)
        if want is None:
            assert as_float(b) != as_float(b), (w, thr)
            continue
        assert int(b) == want, (w, thr, as_float(b), as_float(want))
        if 0 < want < INF_BITS:  # the definition itself
            assert passes(w, thr, want) and not passes(w, thr, want - 1), (w, thr)
    # the cases the kernels' comments name
    look = dict(zip(pairs, got))
    assert as_float(look[(0.5, 0.125)]) == 0.25          # a tie of the product: 0.25 is rejected
    assert as_float(look[(0.0, 0.05)]) == float(np.float32(0.05))  # smallest float >= 0.05
    assert look[(1.0, 0.05)] == INF_BITS and look[(-0.1, 0.05)] == INF_BITS
    assert look[(0.1, 0.0)] == 0 and look[(0.1, -0.05)] == 0


def test_limit_is_monotone_in_w(harness):
    """0 <= w1 <= w2 < 1 gives lim(w1) <= lim(w2): the largest w's limit bounds every point's"""
    rng = np.random.default_rng(4)
    ws = np.unique(np.concatenate([rng.uniform(0, 1, 3000), 1.0 - 2.0 ** -np.arange(1, 54.0),
                                   [0.0, 5e-324, 0.1, 0.5]]))
    ws = ws[ws < 1.0]
    for thr in (5e-324, 1e-40, 5e-5, 0.05, 0.125, 1.0, 1e30, math.inf):
        b = host_limits(harness, [(float(w), thr) for w in ws]).astype(np.int64)
        assert (b <= INF_BITS).all()  # non-negative, no NaN: the bit patterns order like the floats
        assert (np.diff(b) >= 0).all(), thr
