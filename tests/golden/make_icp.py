"""Writes tests/golden/icp_small.npz: the inputs of tests/icp_ref.py's cases and what its align()
gives on them (final, history, aligned, state, iterations, fitness).  Run from the repository root:
python tests/golden/make_icp.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import icp_ref as R  # noqa: E402


def main():
    out, meta = {}, {}
    cases = R.build_cases()
    assert list(cases) == R.CASE_NAMES
    for name, case in cases.items():
        r = R.run_case(case)
        n_corr, mse, ee, T = R.history_arrays(r)
        out[f"{name}/src"] = case["src"]
        out[f"{name}/tgt"] = case["tgt"]
        for k in ("indices", "guess"):
            if k in case:
                out[f"{name}/{k}"] = np.asarray(case[k])
        out[f"{name}/final"] = r["final"]
        out[f"{name}/aligned"] = r["aligned"]
        out[f"{name}/n_corr"], out[f"{name}/mse"], out[f"{name}/e"], out[f"{name}/T"] = n_corr, mse, ee, T
        out[f"{name}/fitness"] = np.float64(r["fitness"])
        meta[name] = dict(state=r["state"], iterations=r["iterations"], converged=r["converged"],
                          args={k: float(case[k]) if k != "max_iterations" else int(case[k])
                                for k in R.ALIGN_KEYS if k in case and k not in ("indices", "guess")})
        print(name, meta[name], "n_corr", n_corr.tolist(), "e", ee[:, 0].tolist(), "mse", mse.tolist()[:3], mse.tolist()[-1:])
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "icp_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
