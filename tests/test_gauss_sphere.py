"""CPU: the Gaussian-sphere plane seeds' host side.  dlg_gs_space and the defaults against the numpy
restatement (tests/gsphere_ref.py) and the reference's config.txt values; the restatement's literal
segmentPlanes BFS against its set version (plane sizes 2 m - 1); every GPU test input's filtered
votes stable; gsphere_model.hpp with the host phases under ASan + UBSan as a stand-alone program."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import gsphere_cases as K
import gsphere_ref as R
import dialog_amd as D
from dialog_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
       "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
f32 = np.float32
NAMES = tuple(K.cases())
FIELDS = [k for k, _ in _lib.GsParams._fields_]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("num_res", [0.25, 0.1, 0.05])
def test_space_equals_the_restatement(num_res):
    P, size = R.create_ps(num_res)
    Q = D.gauss_sphere_space(dict(num_res=num_res))
    assert size == int(np.floor(f32(2.0) / f32(num_res) + f32(0.5)))
    assert len(P) > 0 and Q.shape == P.shape
    assert np.array_equal(bits(Q), bits(P))
    assert D.gauss_sphere_space(dict(num_res=num_res), corners=False) == len(P)


def test_space_capacity_and_bad_resolution():
    L = _lib.load()
    prm = D.gauss_sphere_params(num_res=0.25)
    n = C.c_int64(0)
    buf = np.full((10, 3), 7.0, f32)
    assert L.dlg_gs_space(C.byref(prm), buf.ctypes.data_as(C.POINTER(C.c_float)), 10,
                          C.byref(n)) == _lib.DLG_ERR_CAPACITY
    assert n.value == len(R.create_ps(0.25)[0]) and (buf == 7.0).all()
    for bad in (0.0, -0.1, float("nan"), float("inf"), 0.001):
        prm = D.gauss_sphere_params(num_res=bad)
        assert L.dlg_gs_space(C.byref(prm), None, 0, C.byref(n)) == _lib.DLG_ERR_INVALID


def test_defaults_equal_config_txt():
    """the ten keys of the reference's Dialog/config.txt (lines 10-20), as floats and ints"""
    p = D.gauss_sphere_params()
    want = dict(num_res=0.01, std_dev_gaussian=0.05, search_radius_create_gradient=0.03,
                t_vote_num=500, radius_base=0.03, delta_radius=0.01, s_threshold=0.9,
                dev_threshold=15.0, search_radius_for_plane_seg=0.1, t_num_of_single_plane=500)
    assert FIELDS == list(want) == list(R.DEFAULTS)
    for k, v in want.items():
        got = getattr(p, k)
        assert got == (v if isinstance(v, int) else float(f32(v))), k
        assert R.DEFAULTS[k] == v
    L = _lib.load()
    assert L.dlg_abi_struct_size(23) == C.sizeof(_lib.GsParams) == 40
    assert L.dlg_abi_struct_size(24) == C.sizeof(_lib.GsStats) == 112
    assert L.dlg_abi_struct_size(25) == C.sizeof(_lib.GsResult) == 136


@pytest.mark.parametrize("name", ["size_equal_T", "coplanar_gap"])
def test_literal_bfs_planes_hold_2m_minus_1_points(name):
    """the reference's BFS pushes every point but the seed twice: its size test sees 2 m - 1"""
    pts, nrm, prm = K.cases()[name]
    ref = K.reference(name)
    sinks = list(zip(ref["sink_cells"], ref["sink_votes"]))
    r, t = prm["search_radius_for_plane_seg"], prm["t_num_of_single_plane"]
    lit = R.segment_planes_literal(pts, ref["cell_of_point"], ref["sink"], sinks, r, t)
    sets = R.segment_planes(pts, ref["cell_of_point"], ref["sink"], sinks, r, t, brute=True)
    grid = R.segment_planes(pts, ref["cell_of_point"], ref["sink"], sinks, r, t, brute=False)
    assert len(lit) == len(sets) == len(grid) >= 2
    for a, b, c in zip(lit, sets, grid):
        assert len(a) == 2 * len(b) - 1
        assert np.array_equal(np.unique(a), np.sort(b)) and a[0] == b[0]
        assert np.array_equal(b, c)
    off = ref["plane_offsets"]
    assert [len(b) for b in sets] == list(np.diff(off))


def test_size_rule_at_its_edge():
    """26 points: 2 m - 1 = 51 is kept at T = 51 and dropped at T = 52; 25 points never"""
    a, b = K.reference("size_equal_T"), K.reference("size_below_T")
    sa, sb = list(np.diff(a["plane_offsets"])), list(np.diff(b["plane_offsets"]))
    assert 26 in sa and 25 not in sa and max(sa) > 300
    assert 26 not in sb and 25 not in sb and max(sb) == max(sa)
    c = K.reference("sink_total_below_T")
    assert len(c["sink_cells"]) == 2 and list(c["sink_votes"]) == [300, 99]  # 50 == T_vote: dropped
    assert list(np.diff(c["plane_offsets"])) == [300]                        # 99 = T - 1: nothing


@pytest.mark.parametrize("name", NAMES)
def test_every_case_is_stable(name):
    """floor(G + 0.5f) of every PS cell is the same with every kernel weight one double ulp down
    or up: the GPU tests exclude no cell"""
    ref = K.reference(name)
    assert ref["stable"].all(), np.nonzero(~ref["stable"])[0]


def test_cases_cover_what_they_are_for():
    assert len(K.reference("coplanar_gap")["sink_cells"]) == 2
    assert len(K.reference("coplanar_gap")["plane_offsets"]) - 1 == 3
    assert len(K.reference("offset_planes")["sink_cells"]) == 1
    assert len(K.reference("offset_planes")["plane_offsets"]) - 1 == 2
    nf = K.reference("non_finite")
    bad = ~np.isfinite(K.cases()["non_finite"][1]).all(1)
    assert bad.sum() > 100 and (nf["cell_of_point"][bad] == -1).all()
    assert not np.isin(np.nonzero(bad)[0], nf["plane_ids"]).any() and 100 not in nf["plane_ids"]
    sp = K.reference("sphere")
    pts, _, prm = K.cases()["sphere"]
    occ = np.nonzero(sp["raw_vote"])[0]
    r2 = R.radius2(f32(3.0 * float(f32(prm["std_dev_gaussian"]))))
    most = max(np.count_nonzero(R.d2_to_all(sp["P"][c], sp["P"][occ]) < r2)
               for c in range(0, len(sp["P"]), 7))
    assert most > 256  # beyond the register sort
    for name in NAMES:
        assert len(K.reference(name)["plane_offsets"]) - 1 >= 1, name


# ---- gsphere_model.hpp and the host phases, under the sanitizers ---------------------------------
@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gsan") / "gsphere_model_san")
    subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "dialog_amd/csrc"),
                    os.path.join(ROOT, "tests/cpp/gsphere_model_san.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("name", NAMES)
def test_model_header_against_the_restatement(model_exe, tmp_path, name):
    _, nrm, prm = K.cases()[name]
    ref = K.reference(name)
    p = D.gauss_sphere_params(**prm)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(nrm)) + bytes(p) + np.ascontiguousarray(nrm, f32).tobytes())
    subprocess.run([model_exe, src, dst], check=True, env=ENV)
    blob = open(dst, "rb").read()
    cells, n_sinks, n_fallback = struct.unpack_from("<3i", blob)
    pos = 12

    def take(count, dtype):
        nonlocal pos
        a = np.frombuffer(blob, dtype, count, pos)
        pos += a.nbytes
        return a

    assert cells == len(ref["P"])
    assert np.array_equal(take(3 * cells, np.uint32), bits(ref["P"]).ravel())
    assert np.array_equal(take(len(nrm), np.int32), ref["cell_of_point"])
    assert np.array_equal(take(cells, np.int32), ref["raw_vote"])
    assert np.array_equal(take(cells, np.int32), ref["filtered_vote"])
    assert np.array_equal(take(cells, np.int32), ref["sink_init"])
    assert np.array_equal(take(cells, np.int32), ref["sink"])
    assert np.array_equal(take(n_sinks, np.int32), ref["sink_cells"])
    assert np.array_equal(take(n_sinks, np.int64), ref["sink_votes"])
    assert pos == len(blob)
    if name == "non_unit":
        assert n_fallback > 0  # (the box bound fails far from the shell)
    if name in ("box_corner", "negative"):
        assert n_fallback == 0  # (the lattice ends one step short of an axis normal's query)
