"""The two early outs of dlg::segs_intersect (dialog_amd/csrc/pp_math.hpp) on the host.

The reference's isBothLineSegsIntersect (Dialog/PlaneDetect.h:1966-2015) has no early out; the
kernel's statement rejects a (ray, edge) pair before the square roots from hand-derived error
bounds (T and m in pp_math.hpp).  tests/cpp/pp_math_host.cpp (built with ASan + UBSan, a program
of its own, never loaded into Python) compares it with the oracle's literal statement
(oracle/pcl_oracle.c, orc_segs_intersect) on tuples aimed at those bounds: origin offset x edge
length x class of d = nab . ncd, 80 % of the crossings within 2 (0.0006 + 0.02 L) of an end of the
edge, and directed degenerate tuples.  Any mismatch is a wrong bound.

The device side of the same comparison is tests/test_postprocess_edges_gpu.py.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
PER_CELL = 15000  # x 504 cells = 7.56M sampled tuples + 1.68M directed: ~10 s under ASan
SEED = 1


def rocm_include():
    """<rocm>/include, from where dialog_amd/build.py finds hipcc (pp_math.hpp needs float4)"""
    from dialog_amd.build import hipcc
    for exe in (hipcc(), os.path.realpath(hipcc())):
        inc = os.path.join(os.path.dirname(os.path.dirname(exe)), "include")
        if os.path.exists(os.path.join(inc, "hip", "hip_runtime.h")):
            return inc
    raise RuntimeError("no hip/hip_runtime.h beside hipcc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    d = tmp_path_factory.mktemp("pp_math")
    obj, exe = str(d / "pcl_oracle.o"), str(d / "pp_math_host")
    subprocess.run(["gcc", "-std=gnu11", *SAN, "-Wno-unknown-pragmas", "-c",
                    os.path.join(ROOT, "oracle/pcl_oracle.c"), "-o", obj], check=True)
    subprocess.run(["g++", "-std=c++17", *SAN, "-D__HIP_PLATFORM_AMD__", "-I", rocm_include(),
                    "-I", os.path.join(ROOT, "dialog_amd/csrc"),
                    os.path.join(ROOT, "tests/cpp/pp_math_host.cpp"), obj, "-o", exe, "-lm"],
                   check=True)
    r = subprocess.run([exe, str(PER_CELL), str(SEED)], capture_output=True, text=True, env=ENV,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    cells, directed, total, bad = [], None, None, []
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "cell":
            cells.append(dict(offset=float(t[1]), length=float(t[2]), d=float(t[3]), n=int(t[4]),
                              true=int(t[5]), false_band=int(t[6]), bad=int(t[7])))
        elif t[0] == "directed":
            directed = dict(n=int(t[1]), true=int(t[2]), bad=int(t[4]))
        elif t[0] == "total":
            total = dict(n=int(t[1]), true=int(t[2]), bad=int(t[3]))
        elif t[0] == "bad":
            bad.append(line)
    return dict(cells=cells, directed=directed, total=total, bad=bad, text=r.stdout)


def test_early_outs_agree_with_the_literal_test(report):
    print(report["text"])
    assert len(report["cells"]) == 7 * 6 * 12
    assert all(c["n"] == PER_CELL for c in report["cells"])
    wrong = [c for c in report["cells"] if c["bad"]]
    assert not wrong and not report["bad"], (wrong[:5], report["bad"][:5])
    assert report["directed"]["bad"] == 0
    assert report["total"]["bad"] == 0
    assert report["total"]["n"] == 504 * PER_CELL + report["directed"]["n"]


def test_no_cell_is_vacuous(report):
    """a condition on the sampler: near the origin (offsets <= 1e4) every cell has at least 1 % of
    its tuples accepted by the literal test and at least 1 % rejected with the crossing inside the
    band around an end of the edge; the directed tuples have both verdicts too"""
    for c in report["cells"]:
        if c["offset"] <= 1e4:
            assert c["true"] >= 0.01 * c["n"], c
            assert c["false_band"] >= 0.01 * c["n"], c
    d = report["directed"]
    assert d["n"] > 1_000_000 and 0.05 * d["n"] < d["true"] < 0.95 * d["n"]
