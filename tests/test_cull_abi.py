"""CPU: DLG_OPT_CULL, the DLG_SCORE_BOUND / DLG_SCORE_CULLED benchmark ids and dlg_cull_stats in
the header, the binding and the package agree.  The header writes the option's value as an
expression (the id after DLG_OPT_ICP_MAX_BLOCKS), so it is read through the compiler here, not
with a pattern over the text."""
import os
import subprocess

import dialog_amd
from dialog_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r"""
#include <stdio.h>
#include "dialog_ransac.h"
int main(void) {
  printf("%d %d %d %d\n", (int)DLG_OPT_CULL, (int)DLG_OPT_ICP_MAX_BLOCKS, (int)DLG_SCORE_BOUND,
         (int)DLG_SCORE_CULLED);
  return 0;
}
"""


def test_cull_ids_match_the_header(tmp_path):
    src = tmp_path / "ids.c"
    src.write_text(PROG)
    exe = tmp_path / "ids"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    cull, last, bound, culled = (int(v) for v in out)
    assert cull == 28 and last == 27
    assert _lib.DLG_OPT_CULL == dialog_amd.DLG_OPT_CULL == cull
    assert _lib.DLG_SCORE_BOUND == dialog_amd.DLG_SCORE_BOUND == bound == 3
    assert _lib.DLG_SCORE_CULLED == dialog_amd.DLG_SCORE_CULLED == culled == 4


def test_cull_stats_is_exported():
    L = _lib.load()
    assert "dlg_cull_stats" in _lib.SYMBOLS and hasattr(L, "dlg_cull_stats")
    assert hasattr(dialog_amd.Context, "cull_stats")
