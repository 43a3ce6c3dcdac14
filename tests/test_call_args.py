"""CPU: dialog_amd/csrc/call_args.hpp, the argument checks every call that takes a cloud and an index
list shares, as a stand-alone program under ASan + UBSan (tests/cpp/call_args_san.cpp).  The header
needs no HIP; each row's status and text are compared with the table below."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
       "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

OK, INVALID = 0, 1
STRIDE = "stride_bytes must be >= 12 and a multiple of 4"
# row -> (status, text: the whole message, or the check's result)
WANT = {
    "points null": (INVALID, "points: null or negative size"),
    "points n=-1": (INVALID, "points: null or negative size"),
    "source xyz null": (INVALID, "source: null or negative size"),
    "points empty": (OK, "ok"),
    "points stride 8": (INVALID, STRIDE),
    "points stride 14": (INVALID, STRIDE),
    "points stride 16": (OK, "ok"),
    "target n at 2^31-1": (OK, "ok"),
    "target n above 2^31-1": (INVALID, "target: more than 2147483647 points"),
    "points n at 2^30-1": (OK, "ok"),
    "points n above 2^30-1": (INVALID, "points: more than 1073741823 points"),
    "list none": (OK, "m=5"),
    "list valid": (OK, "m=3"),
    "list empty": (OK, "m=0"),
    "list n_indices=-1": (INVALID, "negative n_indices"),
    "list too long": (INVALID, "more than 2^31-1 indices"),
    "list entry -1": (INVALID, "index out of range"),
    "list entry n": (INVALID, "index out of range"),
    "out stride 12": (OK, "ok"),
    "out stride 16": (OK, "ok"),
    "out stride 20": (INVALID, "out_stride_bytes must be 12 or 16"),
    "guess null": (OK, "1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1"),
    "guess given": (OK, " ".join(str(k) for k in range(1, 17))),
    "guess NaN": (INVALID, "the guess is not finite"),
    "guess inf": (INVALID, "the guess is not finite"),
    "world 1": (OK, "ok"),
    "world 2": (INVALID, "voxel grid: the points are one rank's shard (world > 1); the neighbours "
                         "across its cut need the whole cloud"),
}


def test_every_check_on_its_edge_rows(tmp_path):
    exe = str(tmp_path / "call_args_san")
    subprocess.run(["g++", "-std=c++17", *SAN, "-I", os.path.join(ROOT, "dialog_amd/csrc"),
                    os.path.join(ROOT, "tests/cpp/call_args_san.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {}
    for line in r.stdout.splitlines():
        name, status, text = line.split("|", 2)
        got[name] = (int(status), text)
    assert got == WANT
