"""numpy restatement of pcl::MovingLeastSquares<PointXYZ, PointNormal> (PCL 1.8 mls.hpp, upsampling
NONE, from memory: parity unpinned), independent of the C code.  All arithmetic is
float64 unless marked float32; every sum over the neighbours is a sequential chain (np.cumsum).

    search structure: every finite point of the cloud, listed or not
    queries: the list entries in list order; a non-finite entry gives no row
    neighbours of q: float32 ((0 + dx^2) + dy^2) + dz^2 < float32(float64(r) * float64(r)), q included
    fewer than 3 neighbours: no row
    centroid = (sum p) / m;  C = sum (p - centroid)(p - centroid)^T (unnormalised)
    (lambda, n) = pcl::eigen33(C): smallest eigenvalue, the scaled closed-form routine
    d = -(n . centroid); dist = q . n + d; point = q - dist n
    curvature = trace(C); non-zero: |lambda / trace|; cast to float32
    polynomial_fit and m >= nr_coeff = (order + 1)(order + 2) / 2:
        v = n.unitOrthogonal() (Eigen, isMuchSmallerThan at 1e-12), u = n x v
        per neighbour: de = p - point; sq = float32(de . de); w = exp(-float64(sq) / sqr_gauss_param);
        uc = de . u; vc = de . v; f = de . n; t_j = uc^ui vc^vi (ui = 0..order, vi = 0..order - ui)
        A = sum (t w) t^T; b = sum (t w) f; c = llt(A).solve(b): Eigen's unblocked Cholesky on the
        lower triangle, which stops at the first pivot <= 0 and leaves the rest of the matrix as it
        was; the two triangular solves run over whatever it left (no success check)
        isfinite(c[0]): point += c[0] n; compute_normals: normal = n - c[order + 1] u - c[1] v
    else the projected point and n stand
    row: float32 position, float32 normal (not normalised) and curvature, the entry's index value
    compute_normals off: the normal and curvature fields are zero

Knobs (the order of the double sums and the last bits of the transcendental functions are not part
of the contract): order = "fwd" | "rev" (the neighbour order of every sum; "fwd" is ascending point
index), jitter = j (every exp, atan2, cos and sin result moved j float64 ulps), wrong = one of
WRONG_BUILDS.
"""
import numpy as np

f32 = np.float32
f64 = np.float64
EPS_D = np.finfo(f64).eps
MIN_D = np.finfo(f64).tiny
WRONG_BUILDS = ("plane_only", "weights_from_query", "normal_without_terms", "sq_in_double")
CODE_FIT, CODE_PLANE, CODE_NONFINITE = 0, 1, 2


def nr_coeff(order):
    return (order + 1) * (order + 2) // 2


def flann_d2(q, p):
    """q (a, 3), p (b, 3) float32 -> (a, b) float32, each operation rounded to float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        acc = np.zeros((len(q), len(p)), f32)
        for a in range(3):
            e = (q[:, a, None] - p[None, :, a]).astype(f32)
            acc = (acc + (e * e).astype(f32)).astype(f32)
    return acc


def _jit(x, j):
    if j:
        to = np.inf if j > 0 else -np.inf
        for _ in range(abs(j)):
            x = np.nextafter(x, to)
    return x


def _seq(x):
    """sequential sum over axis 1 (the neighbours)"""
    return np.cumsum(x, axis=1)[:, -1]


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _roots2(b, c):
    d = b * b - 4.0 * c
    d = np.where(d < 0.0, 0.0, d)
    sd = np.sqrt(d)
    return np.zeros_like(b), 0.5 * (b - sd), 0.5 * (b + sd)


def _compute_roots(m, jitter):
    m00, m01, m02 = m[:, 0, 0], m[:, 0, 1], m[:, 0, 2]
    m11, m12, m22 = m[:, 1, 1], m[:, 1, 2], m[:, 2, 2]
    c0 = m00 * m11 * m22 + 2.0 * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01
    c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12
    c2 = m00 + m11 + m22
    q0, q1, q2 = _roots2(c2, c1)
    s_inv3 = f64(1.0 / 3.0)
    s_sqrt3 = np.sqrt(f64(3.0))
    c2_3 = c2 * s_inv3
    a_3 = (c1 - c2 * c2_3) * s_inv3
    a_3 = np.where(a_3 > 0.0, 0.0, a_3)
    half_b = 0.5 * (c0 + c2_3 * (2.0 * c2_3 * c2_3 - c1))
    q = half_b * half_b + a_3 * a_3 * a_3
    q = np.where(q > 0.0, 0.0, q)
    rho = np.sqrt(-a_3)
    theta = _jit(np.arctan2(np.sqrt(-q), half_b), jitter) * s_inv3
    ct, st = _jit(np.cos(theta), jitter), _jit(np.sin(theta), jitter)
    r0 = c2_3 + 2.0 * rho * ct
    r1 = c2_3 - rho * (ct + s_sqrt3 * st)
    r2 = c2_3 - rho * (ct - s_sqrt3 * st)
    s = r0 >= r1
    r0, r1 = np.where(s, r1, r0), np.where(s, r0, r1)
    s2 = r1 >= r2
    r1, r2 = np.where(s2, r2, r1), np.where(s2, r1, r2)
    s3 = s2 & (r0 >= r1)
    r0, r1 = np.where(s3, r1, r0), np.where(s3, r0, r1)
    two = (np.abs(c0) < EPS_D) | (r0 <= 0.0)
    return np.where(two, q0, r0), np.where(two, q1, r1), np.where(two, q2, r2)


def eigen33(C, jitter=0):
    """C (Q, 3, 3) symmetric -> (smallest eigenvalue (Q,), its unit eigenvector (Q, 3))"""
    with np.errstate(all="ignore"):
        scale = np.abs(C).reshape(len(C), 9).max(1)
        scale = np.where(scale <= MIN_D, 1.0, scale)
        m = C / scale[:, None, None]
        r0, _, _ = _compute_roots(m, jitter)
        ev = r0 * scale
        m = m.copy()
        for k in range(3):
            m[:, k, k] = m[:, k, k] - r0

        def cross(a, b):
            return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                             a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)

        def sqn(v):
            return v[:, 0] * v[:, 0] + (v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])

        v1, v2, v3 = cross(m[:, 0], m[:, 1]), cross(m[:, 0], m[:, 2]), cross(m[:, 1], m[:, 2])
        l1, l2, l3 = sqn(v1), sqn(v2), sqn(v3)
        a = (l1 >= l2) & (l1 >= l3)
        b = ~a & (l2 >= l1) & (l2 >= l3)
        v = np.where(a[:, None], v1, np.where(b[:, None], v2, v3))
        ln = np.where(a, l1, np.where(b, l2, l3))
        return ev, v / np.sqrt(ln)[:, None]


def unit_orthogonal(n):
    with np.errstate(all="ignore"):
        x, y, z = n[:, 0], n[:, 1], n[:, 2]
        small = (np.abs(x) <= np.abs(z) * 1e-12) & (np.abs(y) <= np.abs(z) * 1e-12)
        i1 = 1.0 / np.sqrt(x * x + y * y)
        i2 = 1.0 / np.sqrt(y * y + z * z)
        zero = np.zeros_like(x)
        a = np.stack([-y * i1, x * i1, zero], 1)
        b = np.stack([zero, -z * i2, y * i2], 1)
        return np.where(small[:, None], b, a)


def llt_solve(A, b):
    """Eigen's unblocked LLT on the lower triangle of A (Q, N, N) and the two triangular solves of
    b (Q, N); a factorisation that meets a pivot <= 0 stops there"""
    A = A.copy()
    Q, N = b.shape
    alive = np.ones(Q, bool)
    with np.errstate(all="ignore"):
        for k in range(N):
            dot = np.zeros(Q)
            for j in range(k):
                dot = dot + A[:, k, j] * A[:, k, j]
            x = A[:, k, k] - dot
            alive = alive & ~(x <= 0.0)
            sx = np.sqrt(x)
            A[:, k, k] = np.where(alive, sx, A[:, k, k])
            for i in range(k + 1, N):
                dot = np.zeros(Q)
                for j in range(k):
                    dot = dot + A[:, i, j] * A[:, k, j]
                A[:, i, k] = np.where(alive, (A[:, i, k] - dot) / sx, A[:, i, k])
        y = np.zeros((Q, N))
        for i in range(N):
            dot = np.zeros(Q)
            for j in range(i):
                dot = dot + A[:, i, j] * y[:, j]
            y[:, i] = (b[:, i] - dot) / A[:, i, i]
        c = np.zeros((Q, N))
        for i in range(N - 1, -1, -1):
            dot = np.zeros(Q)
            for j in range(i + 1, N):
                dot = dot + A[:, j, i] * c[:, j]
            c[:, i] = (y[:, i] - dot) / A[:, i, i]
    return c


def _group(cloud, q, nb, r, poly_order, polynomial_fit, compute_normals, sqr_gauss, jitter, wrong):
    """queries q (Q, 3) float32 with their m neighbours nb (Q, m) (rows of cloud, in sum order)"""
    Q, m = nb.shape
    P = cloud[nb].astype(f64)  # (Q, m, 3)
    with np.errstate(all="ignore"):
        cen = np.stack([_seq(P[:, :, a]) for a in range(3)], 1) / f64(m)
        D = P - cen[:, None, :]
        C = np.empty((Q, 3, 3))
        for a in range(3):
            for b in range(a, 3):
                C[:, a, b] = C[:, b, a] = _seq(D[:, :, a] * D[:, :, b])
        ev, n = eigen33(C, jitter)
        qd = q.astype(f64)
        d = -_dot3(n, cen)
        dist = _dot3(qd, n) + d
        point = qd - dist[:, None] * n
        tr = (C[:, 0, 0] + C[:, 1, 1]) + C[:, 2, 2]
        curv = np.where(tr != 0.0, np.abs(ev / np.where(tr != 0.0, tr, 1.0)), tr).astype(f32)
        normal = n.copy()
        code = np.full(Q, CODE_PLANE, np.int32)
        nc = nr_coeff(poly_order)
        if polynomial_fit and m >= nc and wrong != "plane_only":
            v = unit_orthogonal(n)
            u = np.stack([n[:, 1] * v[:, 2] - n[:, 2] * v[:, 1], n[:, 2] * v[:, 0] - n[:, 0] * v[:, 2],
                          n[:, 0] * v[:, 1] - n[:, 1] * v[:, 0]], 1)
            de = P - point[:, None, :]
            dw = P - qd[:, None, :] if wrong == "weights_from_query" else de
            sq = _dot3(dw, dw)
            if wrong != "sq_in_double":
                sq = sq.astype(f32).astype(f64)
            w = _jit(np.exp(-sq / sqr_gauss), jitter)
            uc, vc, f = _dot3(de, u[:, None, :]), _dot3(de, v[:, None, :]), _dot3(de, n[:, None, :])
            t = []
            u_pow = np.ones_like(uc)
            for ui in range(poly_order + 1):
                v_pow = np.ones_like(vc)
                for vi in range(poly_order - ui + 1):
                    t.append(u_pow * v_pow)
                    v_pow = v_pow * vc
                u_pow = u_pow * uc
            A = np.zeros((Q, nc, nc))
            bv = np.zeros((Q, nc))
            for a in range(nc):
                tw = t[a] * w
                for b in range(a + 1):
                    A[:, a, b] = _seq(tw * t[b])
                bv[:, a] = _seq(tw * f)
            c = llt_solve(A, bv)
            ok = np.isfinite(c[:, 0])
            point = np.where(ok[:, None], point + c[:, 0, None] * n, point)
            if wrong != "normal_without_terms":
                normal = np.where(ok[:, None],
                                  n - c[:, poly_order + 1, None] * u - c[:, 1, None] * v, normal)
            code = np.where(ok, CODE_FIT, CODE_NONFINITE).astype(np.int32)
    nrm = np.concatenate([normal.astype(f32), curv[:, None]], 1)
    if not compute_normals:
        nrm = np.zeros_like(nrm)
    return point.astype(f32), nrm, code


def mls_ref(points, radius, poly_order=2, polynomial_fit=True, compute_normals=True,
            sqr_gauss_param=0.0, idx=None, order="fwd", jitter=0, wrong=None):
    assert order in ("fwd", "rev") and (wrong is None or wrong in WRONG_BUILDS)
    p = np.ascontiguousarray(points, f32).reshape(-1, 3)
    n = len(p)
    lst = np.arange(n, dtype=np.int64) if idx is None else np.asarray(idx, np.int64).reshape(-1)
    r = f32(radius)
    r2d = f64(r) * f64(r)
    r2 = f32(r2d)
    sqr_gauss = f64(sqr_gauss_param) if sqr_gauss_param > 0 else r2d
    fin_pt = np.isfinite(p).all(1)
    cloud = p[fin_pt]
    valid = fin_pt[lst] if len(lst) else np.zeros(0, bool)
    uniq, inv = np.unique(lst[valid], return_inverse=True)
    inv = inv.reshape(-1)
    U = len(uniq)
    cnt = np.zeros(U, np.int64)
    xyz = np.zeros((U, 3), f32)
    nrm = np.zeros((U, 4), f32)
    code = np.full(U, -1, np.int32)
    for s in range(0, U, 256):
        q = p[uniq[s:s + 256]]
        mask = flann_d2(q, cloud) < r2
        c = mask.sum(1)
        cnt[s:s + 256] = c
        cols = np.nonzero(mask)[1]
        off = np.concatenate([[0], np.cumsum(c)])[:-1]
        for m in np.unique(c):
            if m < 3:
                continue
            qs = np.nonzero(c == m)[0]
            nb = cols[off[qs][:, None] + np.arange(m)[None, :]]
            if order == "rev":
                nb = nb[:, ::-1]
            a, b, cd = _group(cloud, q[qs], nb, r, poly_order, polynomial_fit, compute_normals,
                              sqr_gauss, jitter, wrong)
            xyz[s + qs], nrm[s + qs], code[s + qs] = a, b, cd
    neighbours = np.full(len(lst), -1, np.int32)
    neighbours[valid] = cnt[inv]
    ent_u = np.full(len(lst), -1, np.int64)
    ent_u[valid] = inv
    keep = valid.copy()
    keep[valid] = cnt[inv] >= 3
    ku = ent_u[keep]
    ecnt = neighbours[valid]
    return {
        "xyz": xyz[ku], "normals": nrm[ku], "src_index": lst[keep].astype(np.int32),
        "neighbours": neighbours, "code": code[ku],
        "stats": {
            "n_finite": int(fin_pt.sum()), "n_out": int(keep.sum()),
            "n_too_few": int((ecnt < 3).sum()),
            "n_plane_only": int((code[ku] == CODE_PLANE).sum()),
            "n_fit_nonfinite": int((code[ku] == CODE_NONFINITE).sum()),
            "max_neighbours": int(ecnt.max()) if len(ecnt) else 0,
        },
    }


def rows7(res):
    """the 7 float components of every row as uint32 bit patterns (rows, 7)"""
    return np.concatenate([res["xyz"], res["normals"]], 1).astype(f32).view(np.uint32)


VARIANTS = (dict(jitter=4), dict(jitter=-4), dict(order="rev"), dict(order="rev", jitter=4))


def stable_mask(points, radius, base=None, **kw):
    """rows whose 7 components keep the base run's bits under the four variants"""
    base = mls_ref(points, radius, **kw) if base is None else base
    b = rows7(base)
    ok = np.ones(len(b), bool)
    for v in VARIANTS:
        ok &= (rows7(mls_ref(points, radius, **kw, **v)) == b).all(1)
    return base, ok


def ulp_diff(a, b):
    """|a - b| in float32 ulps of the monotone integer order (NaN against NaN: 0, else huge)"""
    a = np.asarray(a, f32)
    b = np.asarray(b, f32)

    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    d = np.abs(key(a) - key(b))
    nan = np.isnan(a) | np.isnan(b)
    return np.where(nan, np.where(np.isnan(a) & np.isnan(b), 0, 1 << 40), d)


def value_rule(got7, ref7, stable):
    """the parity rule's value part on float32 (rows, 7) arrays -> (max ulps, share bit-equal)"""
    g = np.asarray(got7, f32)[stable]
    w = np.asarray(ref7, f32)[stable]
    if g.size == 0:
        return 0, 1.0
    d = ulp_diff(g, w)
    return int(d.max()), float((d == 0).mean())


def passes_value_rule(got7, ref7, stable):
    mx, eq = value_rule(got7, ref7, stable)
    return mx <= 1 and eq >= 0.99


# ---- the inputs (seeds fixed) ----------------------------------------------------------------------
def wave_cloud(n=1500, seed=21):
    rng = np.random.RandomState(seed)
    xy = rng.uniform(0, 1, (n, 2))
    z = 0.05 * np.sin(6 * xy[:, 0]) * np.cos(5 * xy[:, 1]) + rng.normal(0, 0.002, n)
    return (np.column_stack([xy, z]) + np.array([3.0, -2.0, 1.5])).astype(f32)


def sphere_cloud(n=1500, seed=22):
    rng = np.random.RandomState(seed)
    v = rng.normal(0, 1, (n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return (v * (1.0 + rng.normal(0, 0.002, n))[:, None]).astype(f32)


def sparse_cloud(seed=23):
    rng = np.random.RandomState(seed)
    parts = [wave_cloud(1200, seed)]
    iso = np.column_stack([20.0 + 10.0 * np.arange(24), np.zeros(24), np.zeros(24)])
    parts.append(iso.astype(f32))
    for k, m in enumerate((3, 4, 5, 3, 4, 5, 6, 7)):
        c = np.array([20.0 + 10.0 * k, 50.0, 0.0])
        parts.append((c + rng.uniform(-0.02, 0.02, (m, 3))).astype(f32))
    A = np.concatenate(parts)
    return A[rng.permutation(len(A))]


def blob_cloud(n=1100):
    return wave_cloud(n, 24)


def option_cloud():
    """the first 700 wave points: the option, index-list and non-finite cases"""
    return wave_cloud()[:700].copy()


def nonfinite_cloud():
    A = option_cloud()
    A[5, 1] = np.nan
    A[77, 0] = np.inf
    A[300] = np.nan
    A[699, 2] = -np.inf
    return A


def index_list(n=700, seed=25):
    """permuted, with duplicates, a subset: 500 draws from 0..n-1"""
    return np.random.RandomState(seed).randint(0, n, 500).astype(np.int32)


def cases(shadow):
    """name -> (points, radius, keyword arguments of mls_ref); `qualifies`: the value rule applies
    (else the exact part only).  shadow: tests/golden/double_shadow.pcd's xyz."""
    w, o = wave_cloud(), option_cloud()
    r_o = 0.1
    return {
        "wave_o1": (w, 0.08, dict(poly_order=1)),
        "wave_o2": (w, 0.08, dict(poly_order=2)),
        "wave_o3": (w, 0.08, dict(poly_order=3)),
        "sphere": (sphere_cloud(), 0.15, {}),
        "sparse": (sparse_cloud(), 0.08, {}),
        "shadow_r02": (shadow, 0.02, {}),
        "shadow_r04": (shadow, 0.04, {}),
        "shadow_r01": (shadow, 0.01, {}),
        "blob": (blob_cloud(), 2.0, {}),
        "blob600": (blob_cloud()[:600].copy(), 2.0, {}),
        "opt_nofit": (o, r_o, dict(polynomial_fit=False)),
        "opt_nonormals": (o, r_o, dict(compute_normals=False)),
        "opt_gauss": (o, r_o, dict(sqr_gauss_param=float(f64(f32(r_o)) * f64(f32(r_o)) / 4.0))),
        "opt_index": (o, r_o, dict(idx=index_list())),
        "opt_nonfinite": (nonfinite_cloud(), r_o, {}),
        "opt_nonfinite_index": (nonfinite_cloud(), r_o,
                                dict(idx=np.concatenate([index_list(), [5, 77, 300, 699, 5]])
                                     .astype(np.int32))),
        "identical": (np.full((40, 3), 1.25, f32), 0.5, {}),
    }


# the clouds the value rule is asserted on, with the cap on their unstable rows (1 %)
QUALIFYING = ("wave_o1", "wave_o2", "wave_o3", "sphere", "sparse", "shadow_r02", "shadow_r04",
              "blob", "blob600", "opt_nofit", "opt_nonormals", "opt_gauss", "opt_index",
              "opt_nonfinite", "opt_nonfinite_index")
STAT_KEYS = ("n_finite", "n_out", "n_too_few", "n_plane_only", "n_fit_nonfinite", "max_neighbours")
