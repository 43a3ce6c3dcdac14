"""Scenes for postProcessPlanes' point-in-polygon test and clusterFilt at their edges (no GPU here).

Used by tests/test_postprocess_edges.py (CPU: every scene reaches the branch, task split or
threshold it was built for) and tests/test_postprocess_edges_gpu.py (the device against the oracle).

A mask scene is dict(name, cloud, planes=[dict(coeff (4 floats), border)], t_dist, seed, hits,
tiny): `tiny` lists the planes whose border has 1 or 2 vertices;
`hits` names the classes of (ray, edge) pairs the scene is meant to reach (pair_classes below).
The oracle's answer for a scene is computed once and cached (oracle_masks).
"""
import functools

import numpy as np

from oracle import oracle as O

f32, f64 = np.float32, np.float64

# the L-shaped border of the issue, in z = 0: a collinear middle vertex (2,0) and a duplicate (4,0)
L_XY = np.array([(0, 0), (2, 0), (4, 0), (4, 0), (4, 2), (2, 2), (2, 4), (0, 4), (0, 2)], f64)
# a refit-like plane close to z = 0: the rays are then not exactly parallel / perpendicular to
# the axis-aligned edges, so |d| <= 0.001, d >= 0.9999 and d ~ -1 occur off their exact values
NEAR_Z = (4.9e-4, -1.1e-4, 0.99999994, -1.3e-4)


def _xy0(xy):
    return np.c_[np.asarray(xy, f64), np.zeros(len(xy))]


def grid_cloud(lo, hi, step_inv, rng, sigma=0.003):
    """the grid on [lo, hi]^2 at step 1 / step_inv (exact floats: points fall on edges and
    vertices), once with z ~ N(0, sigma) and once with z = 0"""
    k = np.arange(int(round((hi - lo) * step_inv)) + 1)
    g = lo + k / step_inv
    x, y = np.meshgrid(g, g, indexing="ij")
    flat = np.c_[x.ravel(), y.ravel()]
    return np.concatenate([np.c_[flat, rng.normal(0, sigma, len(flat))], _xy0(flat)])


def rim_points(xy, m, rng, width=0.0005, reach=0.5, sigma=0.003):
    """m points along the lines of the polygon's edges (each extended by `reach` past its ends),
    at most `width` to either side: where single crossings decide the vote, and where the rays
    parallel to an edge run along it"""
    xy = np.asarray(xy, f64)
    a, b = xy, np.roll(xy, -1, axis=0)
    keep = np.linalg.norm(b - a, axis=1) > 1e-9
    a, b = a[keep], b[keep]
    e = rng.integers(0, len(a), m)
    u = (b[e] - a[e]) / np.linalg.norm(b[e] - a[e], axis=1)[:, None]
    s = rng.uniform(-reach, np.linalg.norm(b[e] - a[e], axis=1) + reach)
    q = a[e] + s[:, None] * u + rng.uniform(-width, width, m)[:, None] * np.c_[-u[:, 1], u[:, 0]]
    return np.c_[q, rng.normal(0, sigma, m)]


def knot_points(xy, m, rng, width=0.0005, sigma=0.003):
    """m points within `width` of the polygon's vertices and (small polygons) of the other
    crossings of its edges' lines: there the rays along two edge directions are both in doubt, so
    the vote itself is close"""
    xy = np.asarray(xy, f64)
    knots = [tuple(v) for v in xy]
    a, b = xy, np.roll(xy, -1, axis=0)
    if len(xy) <= 20:
        lo, hi = xy.min(axis=0) - 0.5, xy.max(axis=0) + 0.5
        for i in range(len(xy)):
            for j in range(i + 1, len(xy)):
                u, v = b[i] - a[i], b[j] - a[j]
                den = u[0] * v[1] - u[1] * v[0]
                if abs(den) < 1e-9:
                    continue
                w = a[j] - a[i]
                x = a[i] + (w[0] * v[1] - w[1] * v[0]) / den * u
                if np.all(x >= lo) and np.all(x <= hi):
                    knots.append(tuple(np.round(x, 9)))
    knots = np.array(sorted(set(knots)))
    q = knots[rng.integers(0, len(knots), m)] + rng.uniform(-width, width, (m, 2))
    return np.c_[q, rng.normal(0, sigma, m)]


def near_border(xy, m, rng, **kw):
    """(the test's tolerance is 0.001 on a sum of two distances: a width of 0.0005 puts about a
    third of these points at 4, 5 or 6 odd rays of 10)"""
    return np.concatenate([rim_points(xy, m // 2, rng, **kw), knot_points(xy, m - m // 2, rng)])


def rigid(seed):
    """a random rotation (float64)"""
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def star_xy(n, r0=4.6, r1=3.2):
    th = np.arange(n) * (2.0 * np.pi / n)
    r = np.where(np.arange(n) % 2 == 0, r0, r1)
    return np.c_[r * np.cos(th), r * np.sin(th)]


def circle_xy(n, r):
    th = np.arange(n) * (2.0 * np.pi / n)
    return np.c_[r * np.cos(th), r * np.sin(th)]


def _scene(name, cloud, planes, hits=(), t_dist=0.1, seed=12345, tiny=()):
    """tiny: the planes whose border has 1 or 2 vertices (the only ones not asked for close votes)"""
    assert all(len(planes[k][1]) <= 2 for k in tiny)
    return dict(tiny=tuple(tiny), name=name, cloud=np.ascontiguousarray(cloud, f32),
                planes=[dict(coeff=np.asarray(c, f32), border=np.ascontiguousarray(b, f32))
                        for c, b in planes], t_dist=t_dist, seed=seed, hits=tuple(hits))


def scene_l_axis():
    rng = np.random.default_rng(101)
    cloud = np.concatenate([grid_cloud(-0.5, 4.5, 12, rng), near_border(L_XY, 2000, rng)])
    b = _xy0(L_XY)
    return _scene("l_axis", cloud, [((0, 0, 1, 0), b), (NEAR_Z, b)],
                  hits=("perp", "parallel", "anti", "short"))


def scene_l_moved(k):
    shift = [(10, -10, 5), (1e3, -1e3, 500), (1e5, -1e5, 5e4)][k]
    rng = np.random.default_rng(110 + k)
    R, t = rigid(7 + k), np.array(shift, f64)
    cloud = np.concatenate([grid_cloud(-0.5, 4.5, 12, rng), near_border(L_XY, 2000, rng)]) @ R.T + t
    b = _xy0(L_XY) @ R.T + t
    n = R @ np.array([0.0, 0.0, 1.0])
    return _scene(f"l_moved_{k}", cloud, [(np.r_[n, -n @ t], b)], hits=("perp", "parallel", "anti", "short"))


def scene_long(k):
    """rectangles 0.3 x 4000 and 4000 x 4000 in z = 0: |ab| and W of order 1e3 - 1e4; points
    around the corners and along the long sides"""
    w = [0.3, 4000.0][k]
    rng = np.random.default_rng(120 + k)
    rect = np.array([(0, 0), (w, 0), (w, 4000.0), (0, 4000.0)], f64)
    g = (np.arange(13) - 6) / 64.0  # +-0.094 around a corner at step 1/64
    gx, gy = np.meshgrid(g, g, indexing="ij")
    parts = [np.c_[cx + gx.ravel(), cy + gy.ravel()] for cx, cy in rect]
    m = 700
    for x0 in (0.0, w):  # along the two long sides, within +-0.004 of them and exactly on them
        y = rng.uniform(0, 4000.0, m)
        parts.append(np.c_[x0 + rng.uniform(-0.004, 0.004, m), y])
        parts.append(np.c_[np.full(60, x0), np.round(rng.uniform(0, 4000.0, 60))])
    xy = np.concatenate(parts)
    cloud = np.c_[xy, rng.normal(0, 0.003, len(xy))]
    return _scene(f"long_{k}", cloud, [((0, 0, 1, 0), _xy0(rect)), (NEAR_Z, _xy0(rect))],
                  hits=("perp", "parallel", "anti"))


def scene_short_edges():
    """a square whose bottom side starts with an edge of length 1e-16 (at the origin, where that
    is representable) and ends with a duplicate vertex (length exactly 0)"""
    rng = np.random.default_rng(130)
    xy = np.array([(0, 0), (1e-16, 0), (2, 0), (2, 0), (2, 2), (0, 2)], f64)
    cloud = np.concatenate([grid_cloud(-0.5, 2.5, 12, rng), near_border(xy[[0, 2, 4, 5]], 600, rng)])
    return _scene("short_edges", cloud, [((0, 0, 1, 0), _xy0(xy)), (NEAR_Z, _xy0(xy))],
                  hits=("short", "perp", "parallel", "anti"))


def scene_few_vertices():
    """borders of 1, 2 and 3 vertices (the first vertices of the L: the three are collinear; and
    a proper triangle).  The collinear border has close votes only around its vertices, and only
    when the ten rays split between its two directions: seed 1 draws edges 2 2 1 1 2 1 0 0 1 2,
    four rays along +y (edge 2 runs backwards) and six along -y, where the default seed gives 3:7.
    Those votes sit 0.0005 - 0.0012 from a vertex (nearer, all ten rays are odd), hence the wider
    knot points"""
    rng = np.random.default_rng(140)
    b = _xy0(L_XY)
    tri = _xy0([(0, 0), (4, 0), (0, 4)])
    cloud = np.concatenate([grid_cloud(-0.5, 4.5, 12, rng)[:61 * 61],
                            near_border(tri[:, :2], 2000, rng), near_border(L_XY[:3], 400, rng),
                            knot_points(L_XY[:3], 1200, rng, width=0.0012)])
    return _scene("few_vertices", cloud, [((0, 0, 1, 0), b[:1]), ((0, 0, 1, 0), b[:2]),
                                          ((0, 0, 1, 0), b[:3]), (NEAR_Z, tri)],
                  hits=("short",), seed=1, tiny=(0, 1))


def scene_nonplanar():
    """vertices up to 0.05 off the plane: rays and edges are skew lines.  The offsets are spread
    over four decades (0.05 down to 5e-5): the larger ones fail the crossing test near a vertex
    whatever the early outs do, the smaller ones leave it to them"""
    rng = np.random.default_rng(150)
    xy = star_xy(12, 2.0, 1.2) + 2.0
    b = np.c_[xy, rng.uniform(-1, 1, len(xy)) * np.resize([0.05, 0.005, 0.0005, 0.00005], len(xy))]
    cloud = np.concatenate([grid_cloud(-0.5, 4.5, 12, rng)[:61 * 61], near_border(xy, 3000, rng)])
    return _scene("nonplanar", cloud, [((0, 0, 1, 0), b), (NEAR_Z, b)])


def scene_star(k):
    """the 40-vertex star of the other tests (oblique edges: 0.05 <= |d| <= 0.97 for most pairs,
    which the axis-aligned borders never give), at the origin and rotated 1000 away from it"""
    rng = np.random.default_rng(170 + k)
    xy = star_xy(40)
    cloud = np.concatenate([grid_cloud(-5.0, 5.0, 4, rng), near_border(xy, 2500, rng)])
    b = _xy0(xy)
    if k == 0:
        return _scene("star_0", cloud, [((0, 0, 1, 0), b), (NEAR_Z, b)])
    R, t = rigid(31), np.array((1e3, -1e3, 500.0))
    n = R @ np.array([0.0, 0.0, 1.0])
    return _scene("star_1", cloud @ R.T + t, [(np.r_[n, -n @ t], b @ R.T + t)])


def scene_many_edges():
    """a 1000-gon of radius 3 with 600 candidates: 3 candidate blocks x 63 tasks of 16 edges, the
    last of 8; and borders of 16 and 17 vertices (one task, and a second task of one edge)"""
    rng = np.random.default_rng(160)
    cloud = np.concatenate([near_border(circle_xy(k, 3.0), 200, rng, reach=0.0)
                            for k in (1000, 16, 17)])
    return _scene("many_edges", cloud, [((0, 0, 1, 0), _xy0(circle_xy(1000, 3.0))),
                                        (NEAR_Z, _xy0(circle_xy(16, 3.0))),
                                        (NEAR_Z, _xy0(circle_xy(17, 3.0)))])


MASK_SCENES = {
    "l_axis": scene_l_axis,
    "l_moved_0": lambda: scene_l_moved(0),
    "l_moved_1": lambda: scene_l_moved(1),
    "l_moved_2": lambda: scene_l_moved(2),
    "long_0": lambda: scene_long(0),
    "long_1": lambda: scene_long(1),
    "short_edges": scene_short_edges,
    "few_vertices": scene_few_vertices,
    "nonplanar": scene_nonplanar,
    "many_edges": scene_many_edges,
    "star_0": lambda: scene_star(0),
    "star_1": lambda: scene_star(1),
}


@functools.lru_cache(maxsize=None)
def mask_scene(name):
    return MASK_SCENES[name]()


@functools.lru_cache(maxsize=None)
def oracle_masks(name):
    """per plane (ascending candidate ids int32, masks uint32) from orc_pip_parities"""
    s = mask_scene(name)
    out = []
    for pl in s["planes"]:
        cand, m = O.pip_parities(s["cloud"], pl["coeff"], pl["border"], s["t_dist"], s["seed"])
        ids = np.nonzero(cand)[0].astype(np.int32)
        out.append((ids, m[ids]))
    return out


# ---- the branch choice of isBothLineSegsIntersect, restated -------------------------------------
def _dot(a, b):  # Eigen 3.3 Vector3f: a0 b0 + (a1 b1 + a2 b2), in float
    return (a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])).astype(f32)


def _normalized(v):
    v = np.asarray(v, f32)
    z = _dot(v, v)
    s = np.sqrt(np.where(z > 0, z, f32(1))).astype(f32)
    return np.where((z > 0)[..., None], (v / s[..., None]).astype(f32), v)


def _project(p, c):
    c = np.asarray(c, f32)
    lam = (2.0 * (((c[0] * p[:, 0] + c[1] * p[:, 1]).astype(f32) + c[2] * p[:, 2]).astype(f32)
                  + c[3]).astype(f32).astype(f64)).astype(f32)
    return (p.astype(f64) - (lam.astype(f64) / 2.0)[:, None] * c[:3].astype(f64)).astype(f32)


def pair_classes(points, coeff, border, seed):
    """counts of (ray, edge) pairs of the given candidate points by the branch the crossing test
    takes: perp |d| <= 0.001, parallel d >= 0.9999, anti d <= -0.999 (the general branch where it
    divides by 1 - d^2 ~ 0), short dab <= 1e-15 (no early out); total = all pairs;
    short_by_edge = {edge index: (its dab, its pairs)} for the edges of the short class"""
    b = np.asarray(border, f32)
    nb = len(b)
    nxt = np.roll(b, -1, axis=0)
    with np.errstate(all="ignore"):
        nab = _normalized(nxt - b)
        dab = np.sqrt(((nxt - b) ** 2).astype(f32) @ np.ones(3, f32)).astype(f32)
        idx = np.array(O.msvc_rand(10, seed)) % nb
        dirs = _normalized(np.cross(_normalized(nxt[idx] - b[idx]),
                                    np.asarray(coeff, f32)[:3]).astype(f32))
        pc = _project(np.asarray(points, f32), coeff)
        pd = (pc[:, None, :] + f32(10000.0) * dirs[None, :, :]).astype(f32)
        ncd = _normalized(pd - pc[:, None, :])
        d = _dot(nab[None, None, :, :], ncd[:, :, None, :])
    short = np.broadcast_to(dab <= f32(1e-15), d.shape)
    return dict(perp=int((np.abs(d) <= f32(0.001)).sum()), parallel=int((d >= f32(0.9999)).sum()),
                anti=int((d <= f32(-0.999)).sum()), short=int(short.sum()), total=int(d.size),
                short_by_edge={int(j): (float(dab[j]), int(d[:, :, j].size))
                               for j in np.nonzero(dab <= f32(1e-15))[0]})


def task_split(cand_counts, border_sizes):
    """the task layout of the point-in-polygon launch (dialog_amd/csrc/postprocess_host.cpp,
    pip_masks), restated: -> (cblocks, split, chunk per plane, tasks per candidate block per plane)"""
    cblocks = sum((c + 255) // 256 for c in cand_counts)
    split = max(1, (2048 + cblocks - 1) // max(cblocks, 1))
    chunks = [max(16, (nb + split - 1) // split) for nb in border_sizes]
    per_block = [(nb + ch - 1) // ch for nb, ch in zip(border_sizes, chunks)]
    return cblocks, split, chunks, per_block


# ---- scenes for the full entry (refit, 1-NN marking, absorption, clusterFilt) -------------------
def star_border(n=40, shift=(0.0, 0.0)):
    return _xy0(star_xy(n) + np.asarray(shift, f64)).astype(f32)


def nearest_marks(cloud, plane_points):
    """the oracle's 1-NN marking restated: flann_d2 in float, first minimum"""
    proc = np.zeros(len(cloud), bool)
    c = np.asarray(cloud, f32)
    for q in np.asarray(plane_points, f32).reshape(-1, 3):
        e = (q[None, :] - c).astype(f32)
        d = ((f32(0) + e[:, 0] * e[:, 0]).astype(f32) + e[:, 1] * e[:, 1]).astype(f32)
        d = (d + e[:, 2] * e[:, 2]).astype(f32)
        proc[int(np.argmin(d))] = True
    return proc


def identical_planes(count):
    """`count` copies of one plane: 3 plane points 2 mm apart (none of them a cloud point) and
    the 40-vertex star; a cloud of 8 points.  Every plane has its own candidate block"""
    pts = np.array([(0.001, 0.001, 0), (0.003, 0.001, 0), (0.001, 0.003, 0)], f32)
    cloud = np.array([(0.5, 0.25, 0.01), (2.0, 1.0, -0.02), (-3.0, 0.5, 0.0), (4.0, 0.1, 0.03),
                      (4.5, 2.0, 0.0), (-1.0, -3.3, 0.05), (0.0, 6.0, 0.0), (1.0, 1.0, 0.5)], f32)
    pl = dict(coeff=np.array([0, 0, 1], f32), points=pts, border=star_border())
    return cloud, [pl] * count


def nan_middle():
    """4 planes, the one at index 1 with 2 points (its refit is NaN): for the planes after it
    the compact index on the device differs from the plane index"""
    from dialog_amd.synth import SEED_BASE, postprocess_scene
    cloud, planes = postprocess_scene(3000, 4, n_border=20, seed=SEED_BASE + 61)
    planes[1] = dict(coeff=planes[1]["coeff"], points=planes[1]["points"][:2],
                     border=planes[1]["border"])
    return cloud, planes


def exact_candidates(k):
    """one plane z = 0 (50 of its points, all cloud points), k unclaimed cloud points within
    t_dist of it and 100 beyond t_dist: exactly k candidates"""
    rng = np.random.default_rng(200 + k)
    own = np.c_[rng.uniform(-2, 2, (50, 2)), rng.normal(0, 0.002, 50)]
    near = np.c_[rng.uniform(-5, 5, (k, 2)), rng.uniform(-0.05, 0.05, k)]
    far = np.c_[rng.uniform(-5, 5, (100, 2)), rng.uniform(0.3, 1.0, 100)]
    cloud = np.concatenate([own, near, far]).astype(f32)
    perm = rng.permutation(len(cloud))
    cloud = cloud[perm]
    pts = cloud[np.argsort(perm)[:50]]
    return cloud, [dict(coeff=np.array([0, 0, 1], f32), points=pts, border=star_border())]


def overlapping():
    """two planes in z = 0 whose stars overlap: points inside both appear in both lists"""
    rng = np.random.default_rng(210)
    cloud = np.c_[rng.uniform(-6, 8, (1500, 2)), rng.normal(0, 0.004, 1500)].astype(f32)
    pls = []
    for sh in ((0.0, 0.0), (2.5, 0.5)):
        pts = (np.c_[rng.uniform(-1, 1, (30, 2)) + sh, rng.normal(0, 0.002, 30)]).astype(f32)
        pls.append(dict(coeff=np.array([0, 0, 1], f32), points=pts, border=star_border(shift=sh)))
    return cloud, pls


def one_spot(n, inside=True):
    """n copies of one point inside (or outside) the star: the cloud's bounding box has no extent"""
    pts = np.array([(0.001, 0.001, 0), (0.003, 0.001, 0), (0.001, 0.003, 0)], f32)
    cloud = np.tile(np.array([(1.0, 0.5, 0.01) if inside else (6.0, 6.0, 0.01)], f32), (n, 1))
    return cloud, [dict(coeff=np.array([0, 0, 1], f32), points=pts, border=star_border())]


def nn_ties():
    """1000 copies of one point, 3 copies of 20 others (all inside the star, near z = 0), shuffled;
    two points 0.05 above and below (1, 1, 0); two copies of a point with x = -0.0.  The plane's
    points: one of each distinct point (x = +0.0 for the last), and (1, 1, 0) itself"""
    rng = np.random.default_rng(220)
    base = np.c_[rng.uniform(-2, 2, (21, 2)), rng.normal(0, 0.003, 21)].astype(f32)
    cloud = np.concatenate([np.tile(base[:1], (1000, 1)), np.tile(base[1:], (3, 1)),
                            np.array([(1, 1, 0.05), (1, 1, -0.05)], f32),
                            np.array([(-0.0, 1.5, 0.004)] * 2, f32),
                            np.c_[rng.uniform(-6, 6, (200, 2)), rng.normal(0, 0.003, 200)]
                            .astype(f32)])
    cloud = cloud[rng.permutation(len(cloud))]
    pts = np.concatenate([base, np.array([(1, 1, 0), (0.0, 1.5, 0.004)], f32)])
    return cloud, [dict(coeff=np.array([0, 0, 1], f32), points=pts, border=star_border())], base


# ---- clusterFilt --------------------------------------------------------------------------------
def chain(n, step=0.2):
    """n points at `step` along x from the origin"""
    return np.c_[np.arange(n) * f64(step), np.zeros(n), np.zeros(n)].astype(f32)


def two_chains():
    """two chains of 1500 along x, 10 apart in y, joined only by their last points (a bridge of
    points at step 0.2 along y between them)"""
    a = chain(1500)
    b = a + np.array([0, 10.0, 0], f32)
    k = np.arange(1, 50)
    bridge = np.c_[np.full(49, a[-1, 0]), k * f64(0.2), np.zeros(49)].astype(f32)
    return np.concatenate([a, bridge, b])


def sized_components(T, seed=0):
    """components of exactly T and T + 1 points side by side (chains at step 0.2 along x, 5 apart
    in y), plus one of max(T - 1, 1); shuffled.  -> (points, component label per point)"""
    sizes = [s for s in (T, T + 1, max(T - 1, 1)) if s > 0]
    pts, lab = [], []
    for j, s in enumerate(sizes):
        pts.append(chain(s) + np.array([0, 5.0 * j, 0], f32))
        lab.append(np.full(s, j))
    pts, lab = np.concatenate(pts), np.concatenate(lab)
    perm = np.random.default_rng(300 + T + seed).permutation(len(pts))
    return pts[perm], lab[perm], sizes


def lattices(n=1500, r=0.25):
    """two interleaved 1-D lattices along x (spacing 0.9 r, each one component), the second
    offset by half a step and by 0.75 r in y and z: its points share the grid cells (edge r) of
    the first but are 1.15 r from them, so neighbouring sorted positions alternate between two
    components.  Points of the two alternate in index order too."""
    i = np.arange(n)
    a = np.c_[i * (0.9 * r), np.zeros(n), np.zeros(n)]
    b = np.c_[(i + 0.5) * (0.9 * r), np.full(n, 0.75 * r), np.full(n, 0.75 * r)]
    out = np.empty((2 * n, 3), f64)
    out[0::2], out[1::2] = a, b
    return out.astype(f32)


INT32_MAX = 2 ** 31 - 1


def _shuffled(p, seed):
    return p[np.random.default_rng(seed).permutation(len(p))]


@functools.lru_cache(maxsize=None)
def cluster_cases():
    """name -> (points, radius, T, kept): kept = how many points clusterFilt keeps (components of
    more than T points, compared as size_t), from the construction"""
    C = {}
    ch = chain(3000)
    for nm, p in (("chain", ch), ("chain_shuffled", _shuffled(ch, 1))):
        C[nm + "_T2999"] = (p, 0.25, 2999, 3000)
        C[nm + "_T3000"] = (p, 0.25, 3000, 0)
    tc = two_chains()
    C["two_chains_T3048"] = (tc, 0.25, len(tc) - 1, len(tc))
    C["two_chains_T3049"] = (tc, 0.25, len(tc), 0)
    for T in (0, 1, 63, 64, 255, 256):
        p, _, sizes = sized_components(T)
        C[f"sized_T{T}"] = (p, 0.25, T, sum(s for s in sizes if s > T))
    p, _, sizes = sized_components(64)
    C["T_minus_1"] = (p, 0.25, -1, 0)
    C["T_int32_max"] = (p, 0.25, INT32_MAX, 0)
    # pairs at the radius, built from the origin so that the float coordinates are exact:
    # d2 == r2 does not join (strict <), one ulp less does
    below = float(np.nextafter(f32(0.25), f32(0)))
    for ax in range(3):
        for nm, v, kept in (("at", 0.25, 0), ("below", below, 2)):
            q = np.zeros((2, 3), f32)
            q[1, ax] = v
            C[f"pair_{nm}_r_{'xyz'[ax]}"] = (q, 0.25, 1, kept)
    rng = np.random.default_rng(5)
    dup = np.concatenate([np.tile(np.array([(1.5, -2.0, 0.75)], f32), (600, 1)),
                          (10.0 * (1 + np.arange(5)))[:, None] * np.ones((1, 3), f32)])
    dup = _shuffled(dup.astype(f32), 2)
    C["duplicates_T1"] = (dup, 0.25, 1, 600)
    C["duplicates_T599"] = (dup, 0.25, 599, 600)
    C["duplicates_T600"] = (dup, 0.25, 600, 0)
    for n in (1, 2, 63, 64, 65, 255, 256, 257):  # either side of a wave and of a workgroup
        p = _shuffled(chain(n), n)
        C[f"n{n}_keep"] = (p, 0.25, n - 1, n)
        C[f"n{n}_drop"] = (p, 0.25, n, 0)
    p = rng.uniform(-3, 3, (500, 3)).astype(f32)
    p[100:110] = p[0]  # radius 0 joins nothing, not even equal points
    C["radius0_T0"] = (p, 0.0, 0, 500)
    C["radius0_T1"] = (p, 0.0, 1, 0)
    lt = lattices()
    C["lattices_T1499"] = (lt, 0.25, 1499, 3000)
    C["lattices_T1500"] = (lt, 0.25, 1500, 0)
    return C
