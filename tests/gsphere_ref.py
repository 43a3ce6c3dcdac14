"""numpy restatement of the reference's Gaussian-sphere plane seeds, written literally
(Dialog/PlaneDetect.h:667-1015: createPS, voteForPS, filtPS, createGradientField with
findMaxVoteInPS, rectifySinkFields, segmentPlanes).

Every search is brute force over all parameter-space (PS) cells, with KdTreeFLANN's float distance
((0 + dx dx) + dy dy) + dz dz, a radius hit when d2 < float32(float(r) * float(r)), hits in
(d2, index) order.  Queues are literal.  segment_planes_literal reproduces the reference's BFS with
its duplicated pushes; segment_planes is the set version the library returns.

What the restatement fixes where the reference build leaves it open: ties by
the lowest index, Eigen's norm() as sqrt((x x + y y) + z z), pow(d2, 0.5f) as sqrt, no vote for a
non-finite normal, points with non-finite coordinates in no plane, the sine of rectifySinkFields as
the double sine rounded to float.
"""
from __future__ import annotations

import math
from collections import deque

import numpy as np

f32 = np.float32
PI = f32(3.141592653)
E = f32(2.7182818)

DEFAULTS = dict(num_res=0.01, std_dev_gaussian=0.05, search_radius_create_gradient=0.03,
                t_vote_num=500, radius_base=0.03, delta_radius=0.01, s_threshold=0.9,
                dev_threshold=15.0, search_radius_for_plane_seg=0.1, t_num_of_single_plane=500)


def lattice_size(num_res):
    return int(np.floor(f32(2.0) / f32(num_res) + f32(0.5)))


def create_ps(num_res):
    """-> (cells x 3 float32 min corners in PS order, size)"""
    res = f32(num_res)
    size = lattice_size(res)
    lo = np.arange(size).astype(f32) * res - f32(1.0)
    hi = lo + res
    mn = np.full((size, size, size), np.finfo(f32).max, f32)
    mx = np.full((size, size, size), np.finfo(f32).tiny, f32)
    for cx in (lo, hi):
        for cy in (lo, hi):
            for cz in (lo, hi):
                x, y, z = cx[:, None, None], cy[None, :, None], cz[None, None, :]
                nr = np.sqrt((x * x + y * y) + z * z)
                mn = np.minimum(mn, nr)
                mx = np.maximum(mx, nr)
    keep = (mx >= f32(1.0)) & (mn <= f32(1.0))
    i, j, k = np.nonzero(keep)  # C order: i outer, k inner
    return np.stack([lo[i], lo[j], lo[k]], 1).astype(f32), size


def d2_to_all(q, P):
    ex, ey, ez = q[0] - P[:, 0], q[1] - P[:, 1], q[2] - P[:, 2]
    return ((f32(0.0) + ex * ex) + ey * ey) + ez * ez


def radius2(r):
    return f32(float(f32(r)) * float(f32(r)))


def radius_search(P, c, radius):
    """hits of the search from cell c: (indices, d2) in (d2, index) order"""
    d = d2_to_all(P[c], P)
    hit = np.nonzero(d < radius2(radius))[0]
    o = np.argsort(d[hit], kind="stable")
    return hit[o], d[hit][o]


def vote(normals, num_res, P):
    """-> (cell_of_point, votes)"""
    res = f32(num_res)
    nrm = np.asarray(normals, f32).reshape(-1, 3)
    cell = np.full(len(nrm), -1, np.int32)
    ok = np.isfinite(nrm).all(1)
    with np.errstate(over="ignore", invalid="ignore"):
        q = (np.floor(nrm / res) * res).astype(f32)
    if len(P):
        uq, inv = np.unique(q[ok].view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
        near = np.empty(len(uq), np.int32)
        for t, row in enumerate(uq.view(f32)):
            with np.errstate(over="ignore", invalid="ignore"):
                near[t] = np.argmin(d2_to_all(row, P))  # the first of equals
        cell[ok] = near[inv.reshape(-1)]
    votes = np.bincount(cell[cell >= 0], minlength=len(P)).astype(np.int32)
    return cell, votes


_wcache: dict = {}


def kernel_weight(d2v, std_dev):
    """(float32 weight, the same with the double result one ulp down, one ulp up)"""
    key = (f32(d2v).tobytes(), f32(std_dev).tobytes())
    w = _wcache.get(key)
    if w is None:
        x = float(np.sqrt(f32(d2v)))
        s = float(f32(std_dev))
        sigma = s * s
        A = 2.0 * float(PI) * sigma
        B = x * x / (-2.0 * sigma)
        C = math.pow(float(E), B)
        D = C / A
        w = (f32(D), f32(np.nextafter(D, -np.inf)), f32(np.nextafter(D, np.inf)))
        _wcache[key] = w
    return w


def filt(P, votes, std_dev):
    """-> (filtered votes, stable flags)"""
    radius = f32(3.0 * float(f32(std_dev)))
    out = np.zeros(len(P), np.int32)
    stable = np.ones(len(P), bool)
    occ = np.nonzero(votes)[0]
    if not len(occ):
        return out, stable
    r2 = radius2(radius)
    for c in range(len(P)):
        d = d2_to_all(P[c], P[occ])
        hit = np.nonzero(d < r2)[0]
        if not len(hit):
            continue
        o = np.lexsort((occ[hit], d[hit]))
        G = [f32(0.0), f32(0.0), f32(0.0)]
        for h in hit[o]:
            w = kernel_weight(d[h], std_dev)
            v = f32(votes[occ[h]])
            for t in range(3):
                G[t] = f32(G[t] + f32(w[t] * v))
        r = [int(np.floor(f32(g + f32(0.5)))) for g in G]
        out[c] = r[0]
        stable[c] = r[0] == r[1] == r[2]
    return out, stable


def gradient_field(P, fv, raw, radius, t_vote_num):
    """-> (sink_init, [(index, vote_num)] of the kept sinks); findMaxVoteInPS rescans every time"""
    n = len(P)
    sink_init = np.full(n, -1, np.int32)
    sinks = []
    while True:
        maxvote, index = -1, -1
        cand = np.nonzero((sink_init == -1) & (fv != 0) & (fv > -1))[0]
        if len(cand):
            index = int(cand[np.argmax(fv[cand])])  # strict >: the first maximum
            maxvote = int(fv[index])
        if maxvote == -1:
            break
        sink_init[index] = index
        vote_num = int(raw[index])
        Q = deque([index])
        while Q:
            cur = Q.popleft()
            idx, _ = radius_search(P, cur, radius)
            for o in idx[1:]:
                if fv[o] == 0:
                    continue
                if fv[o] > fv[cur]:
                    continue
                if sink_init[o] == -1:
                    sink_init[o] = index
                    vote_num += int(raw[o])
                    Q.append(int(o))
        if vote_num > t_vote_num:
            sinks.append((index, vote_num))
    return sink_init, sinks


def rectify_sinks(P, sinks, sink_init, radius_base, delta_radius, s_threshold, dev_threshold):
    sink = np.full(len(P), -1, np.int32)
    rad = f32(f32(f32(dev_threshold) * PI) / f32(180.0))
    rmax = f32(f32(math.sin(float(f32(rad * f32(0.5))))) * f32(2.0))
    for index, _ in sinks:
        radius = f32(radius_base)
        while True:
            if radius > rmax:
                break
            idx, _d = radius_search(P, index, radius)
            s_total = f32(len(idx))
            s_sink = f32(np.count_nonzero(sink_init[idx] == index))
            with np.errstate(invalid="ignore", divide="ignore"):
                if f32(s_sink / s_total) < f32(s_threshold):
                    break
            m = idx[(sink_init[idx] == index) & (sink[idx] == -1)]
            sink[m] = index
            radius = f32(radius + f32(delta_radius))
    return sink


class _Search:
    """radius search over a point list: brute force, or the same hits through a hash grid"""

    def __init__(self, pts, radius, brute):
        self.p = np.asarray(pts, f32)
        self.r2 = radius2(radius)
        self.brute = brute
        if not brute:
            self.cell = float(f32(radius)) * 1.001 + 1e-12
            self.key = np.floor(self.p.astype(np.float64) / self.cell).astype(np.int64)
            self.grid = {}
            for i, k in enumerate(map(tuple, self.key)):
                self.grid.setdefault(k, []).append(i)

    def hits(self, i):
        if self.brute:
            cand = np.arange(len(self.p))
        else:
            kx, ky, kz = self.key[i]
            cand = []
            for a in (-1, 0, 1):
                for b in (-1, 0, 1):
                    for c in (-1, 0, 1):
                        cand += self.grid.get((kx + a, ky + b, kz + c), [])
            cand = np.array(sorted(cand), np.int64)
        d = d2_to_all(self.p[i], self.p[cand])
        return cand[d < self.r2]


def _sink_lists(points, cell_of_point, sink, sinks):
    """per kept sink the reference's `planes` list as cloud indices: by PS cell, then point index;
    points with non-finite coordinates left out"""
    pts = np.asarray(points, f32).reshape(-1, 3)
    fin = np.isfinite(pts).all(1)
    lab = np.where((cell_of_point >= 0) & fin, sink[np.maximum(cell_of_point, 0)], -1)
    out = []
    for index, _ in sinks:
        m = np.nonzero(lab == index)[0]
        out.append(m[np.argsort(cell_of_point[m], kind="stable")])
    return out


def segment_planes_literal(points, cell_of_point, sink, sinks, radius, t_single, brute=True):
    """the reference's BFS: every plane as the list it pushes (cloud indices, duplicates kept)"""
    pts = np.asarray(points, f32).reshape(-1, 3)
    planes = []
    for lst in _sink_lists(pts, cell_of_point, sink, sinks):
        if len(lst) < t_single:
            continue
        S = _Search(pts[lst], radius, brute)
        done = np.zeros(len(lst), bool)
        while True:
            rest = np.nonzero(~done)[0]
            if not len(rest):
                break
            seed = int(rest[0])
            plane = []
            Q = deque([seed])
            while Q:
                cur = Q.popleft()
                done[cur] = True
                plane.append(cur)
                for o in S.hits(cur):
                    if done[o]:
                        continue
                    done[o] = True
                    Q.append(int(o))
                    plane.append(int(o))
            if len(plane) >= t_single:
                planes.append(lst[np.array(plane)])
    return planes


def segment_planes(points, cell_of_point, sink, sinks, radius, t_single, brute=False):
    """the set version: a component of m points is kept iff 2 m - 1 >= t_single; each plane as
    its distinct cloud indices in list order, planes by their first point in the list"""
    pts = np.asarray(points, f32).reshape(-1, 3)
    planes = []
    for lst in _sink_lists(pts, cell_of_point, sink, sinks):
        if len(lst) < t_single:
            continue
        S = _Search(pts[lst], radius, brute)
        comp = np.full(len(lst), -1, np.int64)
        for seed in range(len(lst)):
            if comp[seed] != -1:
                continue
            comp[seed] = seed
            Q = deque([seed])
            while Q:
                cur = Q.popleft()
                for o in S.hits(cur):
                    if comp[o] == -1:
                        comp[o] = seed
                        Q.append(int(o))
        for seed in np.unique(comp):
            m = np.nonzero(comp == seed)[0]
            if 2 * len(m) - 1 >= t_single:
                planes.append(lst[m])
    return planes


def run(points, normals, prm, brute=False):
    """the whole pipeline -> dict of everything the library reports"""
    p = dict(DEFAULTS)
    p.update(prm)
    pts = np.asarray(points, f32).reshape(-1, 3)
    P, size = create_ps(p["num_res"])
    cell, raw = vote(normals, p["num_res"], P)
    fv, stable = filt(P, raw, p["std_dev_gaussian"])
    sink_init, sinks = gradient_field(P, fv, raw, p["search_radius_create_gradient"],
                                      p["t_vote_num"])
    sink = rectify_sinks(P, sinks, sink_init, p["radius_base"], p["delta_radius"],
                         p["s_threshold"], p["dev_threshold"])
    planes = segment_planes(pts, cell, sink, sinks, p["search_radius_for_plane_seg"],
                            p["t_num_of_single_plane"], brute)
    off = np.zeros(len(planes) + 1, np.int64)
    if planes:
        off[1:] = np.cumsum([len(x) for x in planes])
    ids = np.concatenate(planes).astype(np.int32) if planes else np.zeros(0, np.int32)
    return dict(P=P, size=size, cell_of_point=cell, raw_vote=raw, filtered_vote=fv, stable=stable,
                sink_init=sink_init, sink=sink,
                sink_cells=np.array([s[0] for s in sinks], np.int32),
                sink_votes=np.array([s[1] for s in sinks], np.int64),
                plane_offsets=off, plane_ids=ids)
