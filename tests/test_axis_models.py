"""CPU: the axis-constrained plane models' host side (SACMODEL_PERPENDICULAR_PLANE,
SACMODEL_PARALLEL_PLANE; DESIGN.md §2, parity unpinned).

* the restatement the GPU tests compare with (tests/axis_ref.py) takes its perpendicular-plane
  angle bit for bit from the C oracle's own getAngle3D (orc_normal_plane_dist with lambda 1 and a
  plane through the origin returns exactly that angle);
* the float thresholds the device compares against give, for every float, the verdict of the
  acos / sin formula evaluated directly -- 2000 random dot products and the 129 floats around
  each threshold, which is where the bisection's monotonicity assumption could fail;
* the new ABI entries exist, the ABI version is unchanged, dlg_ctx_set_axis rejects NaN;
* the validity and threshold functions under ASan + UBSan in a stand-alone program.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import dialog_amd as D
from dialog_amd import _lib
from oracle import oracle as O

import axis_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = [1e-3, math.radians(5.0), math.radians(30.0), math.radians(89.9), math.pi / 2]
F = np.float32


def around(f, k=64):
    """the 2 k + 1 floats centred on f, in bit-pattern order (through zero)"""
    def key(b):  # float bits -> a monotone integer
        return (b & 0x7FFFFFFF) if not (b & 0x80000000) else -(b & 0x7FFFFFFF) - 1

    def unkey(v):
        return v if v >= 0 else (0x80000000 | (-v - 1))

    b = int(np.array(f, F).view(np.uint32))
    keys = np.arange(key(b) - k, key(b) + k + 1)
    keys = keys[(keys <= 0x7F800000) & (keys >= -0x7F800000 - 1)]
    return np.array([unkey(int(v)) for v in keys], np.uint32).view(F)


def test_helper_angle_is_the_oracles_get_angle_3d():
    rng = np.random.default_rng(1)
    axes = [(0, 0, 1), (0.3, -1.7, 2.0), (1e-3, 0, 0), (0, 0, 0), (5, 5, -5)]
    planes = rng.normal(size=(300, 3)).astype(F)
    planes[:40] *= F(1e-3)
    planes[40:60, 1:] = 0  # axis-aligned normals: |rad| = 1 exactly
    planes[60] = 0
    for a in axes:
        a4 = np.array([a[0], a[1], a[2], 0.0], F)
        for c in planes:
            c4 = np.array([c[0], c[1], c[2], 0.0], F)
            want = O.normal_plane_dist(c4, (0, 0, 0), a4, lam=1.0)
            got = R.perp_angle(R.dot_predux(R.normalized4(a4[:3]), R.normalized4(c)))
            assert np.float64(want).view(np.uint64) == np.float64(got).view(np.uint64), (a, c)


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("model", [R.PERP, R.PAR])
def test_threshold_verdict_equals_the_formula(model, eps):
    rng = np.random.default_rng(7)
    _, _, (t_lo, t_hi) = D.axis_verdicts(model, eps, np.zeros(1, F))
    f = [rng.uniform(-1.0, 1.0, 1500).astype(F), rng.normal(0, 1.5, 500).astype(F),
         around(t_lo), around(t_hi), around(F(0)), around(F(1)), around(F(-1)),
         np.array([np.inf, -np.inf, np.nan, 3.0, -3.0], F)]
    if model == R.PAR:
        s_floor = t_hi
        assert float(s_floor) <= abs(math.sin(eps)) < float(np.nextafter(s_floor, F(np.inf)))
        f.append(around(-s_floor))
    f = np.concatenate(f)
    by_thr, by_formula, _ = D.axis_verdicts(model, eps, f)
    direct = np.array([(R.perp_valid_f if model == R.PERP else R.par_valid_f)(v, eps) for v in f])
    assert np.array_equal(by_formula.astype(bool), direct)  # the library's formula is the spec's
    assert np.array_equal(by_thr.astype(bool), direct)      # ... and the thresholds decide alike
    if eps < math.pi / 2:
        assert 0 < np.count_nonzero(direct) < direct.size   # (both verdicts occur)


@pytest.mark.parametrize("model", [R.PERP, R.PAR])
def test_eps_zero_accepts_everything(model):
    f = np.concatenate([np.linspace(-2, 2, 101).astype(F), np.array([np.nan, np.inf], F)])
    for eps in (0.0, -1.0):
        by_thr, by_formula, _ = D.axis_verdicts(model, eps, f)
        assert by_thr.all() and by_formula.all()


def test_abi_entries_and_version():
    L = _lib.load()
    assert L.dlg_abi_version() == 5 == _lib.ABI_VERSION
    for s in ("dlg_ctx_set_axis", "dlg_ctx_get_axis", "dlg_score_samples", "dlg_axis_verdicts"):
        assert hasattr(L, s), s
    assert D.SACMODEL_PERPENDICULAR_PLANE == 9 and D.SACMODEL_PARALLEL_PLANE == 15
    assert L.dlg_abi_struct_size(1) == C.sizeof(_lib.SacParams)  # dlg_sac_params keeps its layout
    # argument checks that need no context or device
    ax = (C.c_float * 3)(0, 0, 1)
    assert L.dlg_ctx_set_axis(None, ax, 0.1) == _lib.DLG_ERR_INVALID
    bad = np.zeros(4, np.int32)
    f = np.zeros(4, F)
    fp = f.ctypes.data_as(C.POINTER(C.c_float))
    ip = bad.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.dlg_axis_verdicts(0, 0.1, fp, 4, ip, ip, None) == _lib.DLG_ERR_INVALID
    assert L.dlg_axis_verdicts(9, math.nan, fp, 4, ip, ip, None) == _lib.DLG_ERR_INVALID


def test_axis_model_under_sanitizers(tmp_path):
    """tests/cpp/axis_model_san.cpp: axis_model.hpp's validity, threshold and sample-plane
    functions built with g++ -fsanitize=address,undefined (its own main; nothing is loaded into
    Python); it checks thresholds against the formula itself and prints a checksum."""
    exe = str(tmp_path / "axis_model_san")
    san = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.run(["g++", "-std=c++17", *san, "-I", os.path.join(ROOT, "dialog_amd/csrc"),
                    os.path.join(ROOT, "tests/cpp/axis_model_san.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.startswith("ok ")


def test_cpp_shim_axis_program_compiles_and_links(tmp_path):
    """tests/cpp/shim_axis.cpp (setAxis / setEpsAngle / the two pcl::SacModel values /
    ExtractParams' axis) compiles with g++ against the shim header and links the library"""
    exe = tmp_path / "shim_axis"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "shim_axis.cpp"), "-o", str(exe),
           "-L", os.path.dirname(_lib.LIB_PATH), "-ldialog_amd",
           f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
