"""CPU: DLG_OPT_CULL_FUSE (29, the id after DLG_OPT_CULL) agrees in the header, the binding and the
package.  The header writes the value as an expression, so it is read through the compiler."""
import os
import subprocess

import dialog_amd
from dialog_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r"""
#include <stdio.h>
#include "dialog_ransac.h"
int main(void) {
  printf("%d %d\n", (int)DLG_OPT_CULL_FUSE, (int)DLG_OPT_CULL);
  return 0;
}
"""


def test_cull_fuse_id_matches_the_header(tmp_path):
    src = tmp_path / "ids.c"
    src.write_text(PROG)
    exe = tmp_path / "ids"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    fuse, cull = (int(v) for v in out)
    assert fuse == 29 and cull == 28
    assert _lib.DLG_OPT_CULL_FUSE == dialog_amd.DLG_OPT_CULL_FUSE == fuse
