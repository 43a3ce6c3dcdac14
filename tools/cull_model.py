"""CPU model of the culled scoring's tile bound (DLG_OPT_CULL; scheme in DESIGN.md §3, table in §7
"Culled rounds").

For a synthetic cloud (dialog_amd.synth.plane_cloud) and D random three-point planes it builds
tiles of 32 points along a space-filling curve (Hilbert, as the library, or Z-order), their
box-midpoint bounding spheres, the bound UB_h = 32 x (tiles whose sphere plane h comes within
threshold + radius of) and the exact counts of the K hypotheses with the largest UB; then B = their
best exact count and the hypotheses left with UB >= B.  Rounds after the first are modelled by
removing the points of the first `removed` planes of the cloud.

  python tools/cull_model.py [--points 1000000] [--planes 20] [--hyps 4096] [--k 64]
                             [--removed 0,10,17,19] [--curve hilbert|morton] [--seed-offset 3]

numpy only; 10 M points take a few minutes and ~2 GB.  The near test is |n.c + d| <= thr + r in
float64 (the device adds a rounding margin of ~1e-5 to thr: slightly more pairs).
The candidates are the K largest UB over all D planes, ties to the lower index (the device takes
them among the good draws only; the model's random planes are all good).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dialog_amd.synth import SEED_BASE, plane_cloud  # noqa: E402

TILE = 32


def spread10(v):
    v = v.astype(np.uint32) & 0x3FF
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


def hilbert10(x, y, z):
    """Skilling's transpose form, 10 bits per axis (spatial.hip hilbert10)"""
    X = [x.astype(np.uint32), y.astype(np.uint32), z.astype(np.uint32)]
    Q = 1 << 9
    while Q > 1:
        P = np.uint32(Q - 1)
        for i in range(3):
            hit = (X[i] & Q) != 0
            if i == 0:
                X[0] = np.where(hit, X[0] ^ P, X[0])
            else:
                t = (X[0] ^ X[i]) & P
                X[0] = np.where(hit, X[0] ^ P, X[0] ^ t)
                X[i] = np.where(hit, X[i], X[i] ^ t)
        Q >>= 1
    X[1] ^= X[0]
    X[2] ^= X[1]
    t = np.zeros_like(X[0])
    Q = 1 << 9
    while Q > 1:
        t = np.where((X[2] & Q) != 0, t ^ np.uint32(Q - 1), t)
        Q >>= 1
    X = [v ^ t for v in X]
    return (spread10(X[0]) << 2) | (spread10(X[1]) << 1) | spread10(X[2])


def curve_order(p, curve):
    a = np.abs(p).max(axis=0).astype(np.float64)
    q = np.clip((p + a) * (1023.99 / (2.0 * a)), 0, 1023).astype(np.uint32)
    if curve == "hilbert":
        key = hilbert10(q[:, 0], q[:, 1], q[:, 2])
    else:
        key = spread10(q[:, 0]) | (spread10(q[:, 1]) << 1) | (spread10(q[:, 2]) << 2)
    return np.argsort(key, kind="stable")


def tile_spheres(p):
    n = p.shape[0]
    nt = -(-n // TILE)
    pad = np.concatenate([p, np.repeat(p[-1:], nt * TILE - n, axis=0)]).reshape(nt, TILE, 3)
    c = 0.5 * (pad.min(axis=1) + pad.max(axis=1))
    r = np.sqrt(((pad - c[:, None, :]) ** 2).sum(axis=2)).max(axis=1)
    return c.astype(np.float64), r.astype(np.float64)


def random_planes(p, d, rng):
    i = rng.integers(0, p.shape[0], size=(d, 3))
    a, b, c = (p[i[:, k]].astype(np.float64) for k in range(3))
    nrm = np.cross(b - a, c - a)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    return np.concatenate([nrm, -(nrm * a).sum(axis=1, keepdims=True)], axis=1)


def model(p, planes, thr, k):
    c, r = tile_spheres(p)
    ub = np.zeros(planes.shape[0], np.int64)
    for h0 in range(0, planes.shape[0], 64):
        pl = planes[h0:h0 + 64]
        near = np.abs(c @ pl[:, :3].T + pl[:, 3]) <= thr + r[:, None]
        ub[h0:h0 + 64] = TILE * near.sum(axis=0)
    top = np.argsort(-ub, kind="stable")[:k]
    pd = p.astype(np.float64)
    exact = np.array([(np.abs(pd @ planes[h, :3] + planes[h, 3]) < thr).sum() for h in top])
    b = int(exact.max())
    left = int((ub >= b).sum() - (ub[top] >= b).sum())
    pairs = ub.sum() // TILE
    return dict(tiles=c.shape[0], median_ub=int(np.median(ub)), B=b, left_after_k=left,
                pair_fraction=round(float(pairs) / (c.shape[0] * planes.shape[0]), 4),
                pairs_top_k_share=round(float(ub[top].sum()) / max(float(ub.sum()), 1.0), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--planes", type=int, default=20)
    ap.add_argument("--hyps", type=int, default=4096)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--threshold", type=float, default=0.02)
    ap.add_argument("--removed", default="0,10,17,19")
    ap.add_argument("--curve", choices=("hilbert", "morton"), default="hilbert")
    ap.add_argument("--seed-offset", type=int, default=3)
    a = ap.parse_args()
    pts, lab, _ = plane_cloud(a.points, a.planes, seed=SEED_BASE + a.seed_offset)
    rng = np.random.default_rng(777)
    print("| active points | median UB | B | left with UB >= B after K | pair fraction | top-K share of pairs |")
    print("|---|---|---|---|---|---|")
    for rem in (int(v) for v in a.removed.split(",")):
        p = pts[(lab < 0) | (lab >= rem)]
        p = p[curve_order(p, a.curve)]
        m = model(p, random_planes(p, a.hyps, rng), a.threshold, a.k)
        print(f"| {p.shape[0]} ({rem} removed) | {m['median_ub']} | {m['B']} | {m['left_after_k']} | "
              f"{m['pair_fraction']} | {m['pairs_top_k_share']} |")


if __name__ == "__main__":
    main()
