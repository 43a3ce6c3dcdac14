"""Writes tests/golden/sac_ia_small.npz: the inputs of tests/sac_ia_ref.py's cases (double_shadow.pcd's
two halves, 446 and 545 points, with fpfh_ref's descriptors; every distinct array stored once under
its hash) and what its align() gives on them: final, aligned, every hypothesis record, the counts,
the error and the fitness score.  Built from the restatement only; each case is asserted to reach
the path it is there for.  CPU only, run from the repository root:

    python tests/golden/make_sac_ia.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import sac_ia_ref as S  # noqa: E402

INPUTS = ("src", "fs", "tgt", "ft", "guess")
SCALARS = ("converged", "best_iteration", "n_valid", "n_invalid", "draws", "relaxations",
           "n_queries", "error", "fitness")


def main():
    out, meta = {}, {}
    cases = S.build_cases()
    for name, case in cases.items():
        r = S.run_case(case)
        S.check_paths(name, case, r)
        m = dict(inputs={}, args={k: case[k] for k in S.ALIGN_KEYS if k in case},
                 E=str(r["E"]), **{k: r[k] for k in SCALARS})
        for k in INPUTS:
            if k in case:
                a = np.ascontiguousarray(case[k], np.float32)
                key = "a/" + hashlib.sha256(a.tobytes()).hexdigest()[:12]
                out[key] = a
                m["inputs"][k] = key
        out[f"{name}/final"] = r["final"]
        out[f"{name}/aligned"] = r["aligned"]
        for k, v in S.hypothesis_arrays(r).items():
            out[f"{name}/{k}"] = v
        meta[name] = m
        print(name, {k: m[k] for k in SCALARS}, "iterations", len(r["hyp"]))
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "sac_ia_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
