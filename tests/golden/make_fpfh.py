"""Writes tests/golden/fpfh_small.npz: for every case of tests/fpfh_ref.py's cases() the input (the
points, the normals pca_normals() gave them, the index list) and the numpy reference's results:
the neighbour counts, the stable masks (by point and by row, packed bits), the integer stats, every
STEP-th row of the descriptors and of the SPFH counts, and the SHA-256 of all of them (the whole
tables would not fit the size a committed fixture may have).  CPU only:

    python tests/golden/make_fpfh.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import fpfh_ref as F  # noqa: E402
from dialog_amd import pcd  # noqa: E402

STEP = 8


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def entry(ref):
    """what the fixture keeps of a reference run"""
    return {
        "nb": ref["neighbours"].astype(np.int16),
        "stable": np.packbits(ref["stable"]),
        "stable_spfh": np.packbits(ref["stable_spfh"]),
        "hist": ref["hist"][::STEP].copy(),
        "counts": ref["counts"][::STEP].astype(np.uint16),
    }, dict(stats=ref["stats"], hist_sha=digest(ref["hist"]), counts_sha=digest(ref["counts"]))


def main():
    shadow = np.ascontiguousarray(pcd.read_pcd(os.path.join(HERE, "double_shadow.pcd"))[:, :3],
                                  np.float32)
    out, meta = {}, {}
    for name, (pts, r_normals, radius, idx) in F.cases(shadow).items():
        nrm = F.pca_normals(pts, r_normals)
        ref = F.fpfh_ref(pts, nrm, radius, idx)
        arrays, m = entry(ref)
        out[name + "/points"] = pts
        out[name + "/normals"] = nrm
        if idx is not None:
            out[name + "/idx"] = np.asarray(idx, np.int32)
        for k, v in arrays.items():
            out[name + "/" + k] = v
        meta[name] = dict(radius=radius, r_normals=r_normals, **m)
        print(f"{name}: n {len(pts)} rows {len(ref['stable'])} unstable rows "
              f"{int((~ref['stable']).sum())} points {int((~ref['stable_spfh']).sum())} "
              f"{ref['stats']}")
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "fpfh_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
