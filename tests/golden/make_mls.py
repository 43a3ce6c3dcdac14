"""Writes tests/golden/mls_small.npz: for every case of tests/mls_ref.py's cases() the input, the
base run of the numpy reference (the 7 float components of every row, the index values, the
neighbour counts, the branch counts) and the stable mask -- the rows whose 7 components keep the
base run's bits when the reference is rerun with every exp / atan2 / cos / sin result moved +4 and
-4 double ulps, with the sums reversed, and with both.  CPU only:

    python tests/golden/make_mls.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mls_ref as M  # noqa: E402
from dialog_amd import pcd  # noqa: E402


def main():
    shadow = np.ascontiguousarray(pcd.read_pcd(os.path.join(HERE, "double_shadow.pcd"))[:, :3],
                                  np.float32)
    out, meta = {}, {}
    for name, (pts, radius, kw) in M.cases(shadow).items():
        base, stable = M.stable_mask(pts, radius, **kw)
        out[name + "/points"] = pts
        out[name + "/rows"] = np.concatenate([base["xyz"], base["normals"]], 1).astype(np.float32)
        out[name + "/src"] = base["src_index"]
        out[name + "/nb"] = base["neighbours"]
        out[name + "/stable"] = stable
        out[name + "/stats"] = np.array([base["stats"][k] for k in M.STAT_KEYS], np.int64)
        if "idx" in kw:
            out[name + "/idx"] = np.asarray(kw["idx"], np.int32)
        meta[name] = dict(radius=radius, **{k: v for k, v in kw.items() if k != "idx"})
        print(f"{name}: rows {len(stable)} unstable {int((~stable).sum())} {base['stats']}")
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "mls_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
