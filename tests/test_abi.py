"""CPU: the C-ABI library builds, loads and exports every symbol include/*.h declares; without a
GPU the product fails loudly (no CPU fallback); host-only entry points behave."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dialog_amd
from dialog_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "dialog_ransac.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dlg_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    L = _lib.load()
    syms = header_symbols()
    assert len(syms) >= 20
    missing = [s for s in syms if not hasattr(L, s)]
    assert not missing, missing
    assert set(syms) == set(_lib.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dlg_\w+)", out))
    assert set(syms) <= exported


def test_library_is_gfx950_code_object():
    """The fat binary embedded in the .so carries a gfx950 code object (and no other target)."""
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    for other in (b"--gfx942", b"--gfx90a", b"--gfx1100"):
        assert other not in blob


def test_params_defaults_match_pcl():
    p = dialog_amd.make_params()
    L = _lib.load()
    d = _lib.SacParams()
    L.dlg_sac_params_default(C.byref(d))
    assert d.max_iterations == 50 and d.probability == 0.99 and d.optimize == 1
    assert d.seed == 12345 and d.model == 0 and d.threshold == 0.0
    assert p.max_iterations == 50
    assert L.dlg_abi_version() == _lib.ABI_VERSION == 5
    assert L.dlg_status_string(0) == b"ok"


def test_option_ids_match_the_header():
    """every DLG_OPT_* of the header has the same value in the binding, and the package exports it"""
    src = open(os.path.join(ROOT, "include", "dialog_ransac.h")).read()
    ids = {k: int(v) for k, v in re.findall(r"\b(DLG_OPT_[A-Z0-9_]+)\s*=\s*(\d+)", src)}
    assert len(ids) >= 27 and len(set(ids.values())) == len(ids)
    assert ids["DLG_OPT_ICP_REVERSED"] == 26 and ids["DLG_OPT_ICP_MAX_BLOCKS"] == 27
    assert max(ids.values()) == 27
    for name, v in ids.items():
        assert getattr(_lib, name) == v, name
        assert getattr(dialog_amd, name) == v, name


def test_struct_layouts_match_the_header():
    """The ctypes structs have the header's sizes (dlg_abi_struct_size reports sizeof of each): a
    binding built for another layout would read or write past the caller's struct."""
    L = _lib.load()
    pairs = [(0, _lib.Points), (1, _lib.SacParams), (2, _lib.SacStats), (3, _lib.ExtractStats),
             (4, _lib.Planes), (5, _lib.PostProcessParams), (26, _lib.KnnRecord)]
    for which, cls in pairs:
        assert L.dlg_abi_struct_size(which) == C.sizeof(cls), cls.__name__
    assert L.dlg_abi_struct_size(99) == -1
    assert L.dlg_abi_struct_size(27) == -1


def test_knn_stats_is_exported():
    """dlg_knn_stats / dlg_knn_record: an added entry under the same ABI version; the record is
    168 bytes (12 levels) and the call refuses null arguments without a context"""
    L = _lib.load()
    assert "dlg_knn_stats" in _lib.SYMBOLS and hasattr(L, "dlg_knn_stats")
    assert hasattr(dialog_amd.Context, "knn_stats")
    assert L.dlg_abi_struct_size(26) == C.sizeof(_lib.KnnRecord) == 168
    assert [f[0] for f in _lib.KnnRecord._fields_] == ["valid", "k", "n", "levels_planned",
                                                       "reserved", "queries", "built"]
    assert len(_lib.KnnRecord().queries) == len(_lib.KnnRecord().built) == 12
    r = _lib.KnnRecord()
    assert L.dlg_knn_stats(None, C.byref(r)) == _lib.DLG_ERR_INVALID
    assert L.dlg_abi_version() == _lib.ABI_VERSION == 5


def test_debug_pip_masks_is_exported():
    """dlg_debug_pip_masks: an added debug entry under the same ABI version; the Python wrapper
    exists and the call refuses a null context"""
    L = _lib.load()
    assert "dlg_debug_pip_masks" in _lib.SYMBOLS and hasattr(L, "dlg_debug_pip_masks")
    assert "dlg_debug_pip_masks" in header_symbols()
    assert callable(dialog_amd.debug_pip_masks)
    need = C.c_int64(-1)
    assert L.dlg_debug_pip_masks(None, None, None, 0.1, 0, None, None, None, 0,
                                 C.byref(need)) == _lib.DLG_ERR_INVALID
    assert L.dlg_abi_version() == _lib.ABI_VERSION == 5


def test_no_device_fails_loudly(monkeypatch):
    """On a box without a gfx950 device the product refuses to run (no silent CPU path)."""
    try:
        import torch  # noqa: F401  (only to ask whether a GPU exists)
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        pytest.skip("GPU present: covered by the -m gpu tests")
    with pytest.raises(dialog_amd.DialogError) as ei:
        dialog_amd.Context(0)
    assert ei.value.status == 3  # DLG_ERR_NO_DEVICE
    seg = dialog_amd.SACSegmentation()
    seg.setModelType(dialog_amd.SACMODEL_PLANE)
    seg.setMethodType(dialog_amd.SAC_RANSAC)
    seg.setDistanceThreshold(0.01)
    seg.setInputCloud(np.zeros((10, 3), np.float32))
    with pytest.raises(dialog_amd.DialogError):
        seg.segment()


@pytest.mark.parametrize("prog", ["shim_smoke", "plane_clouds_glue", "poly_planes_glue"])
def test_cpp_shim_compiles_and_links(tmp_path, prog):
    """The PCL-compatible C++ host shim compiles with g++ against the header and links the .so
    (shim_smoke: every shim entry; plane_clouds_glue: INTEGRATION.md §3's PlaneDetect.h adapter
    with the reference's struct Plane)."""
    src = os.path.join(ROOT, "tests", "cpp", prog + ".cpp")
    exe = tmp_path / prog
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", str(exe),
           "-L", os.path.dirname(_lib.LIB_PATH), "-ldialog_amd",
           f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
