"""GPU: the calls that share the context's staging buffers (csrc/cloud_call.cpp: the raw upload, the
staged index list, the de-interleaved cloud with its flags and kept positions, the kept points and
their grids), one after the other on ONE context, forwards and then backwards at other sizes, so
that every shared buffer is both smaller and larger for one user than for the one before it.  Each
result must equal, bit for bit, the same call on a context created for it alone: both run the same
device code on the same input, so any difference is a buffer read stale or sized by the previous
caller.  (Bit equality is the comparison of the voxel, outlier, registration, SAC-IA and normals
tests with their references; the MLS and FPFH tests allow 1 ulp against a host reference, which two
runs of the same kernels do not need.)"""
import numpy as np
import pytest

import dialog_amd as D
from dialog_amd.synth import plane_cloud

pytestmark = pytest.mark.gpu

f32 = np.float32


def cloud(n, seed, holes=True):
    """n points on two 4 x 4 patches; every 97th one not finite (a kept position then differs from
    its row)"""
    p, _, _ = plane_cloud(n, 2, seed=seed, patch=4.0)
    if holes:
        p[5::97, seed % 3] = np.nan
    return p


def some(n, step):
    """an index list over n points: every step-th one, backwards"""
    return np.arange(0, n, step, dtype=np.int32)[::-1].copy()


def blob(*parts):
    """the bytes of a call's results (arrays, and dicts of numbers)"""
    out = []
    for p in parts:
        if isinstance(p, dict):
            p = np.concatenate([np.atleast_1d(np.asarray(p[k], np.float64)) for k in sorted(p)
                                if not k.endswith("_ms")])
        out.append(np.ascontiguousarray(p).tobytes())
    return tuple(out)


# ---- the eight calls: (ctx, n, seed) -> the bytes of everything the call returns --------------------
def sac_ia(ctx, n, seed):
    tgt = cloud(n, seed)
    src = cloud(n, seed, holes=False)[:n * 2 // 3] + f32(0.02)  # (part of the target, moved)
    rng = np.random.default_rng(seed)
    fs = rng.uniform(0, 100, (src.shape[0], 33)).astype(f32)
    ft = rng.uniform(0, 100, (n, 33)).astype(f32)
    ft[3::89, 7] = np.nan  # (rows that are not valid)
    final, aligned, hyp, st = D.sac_ia_align(src, fs, tgt, ft, max_iterations=16,
                                             k_correspondences=3, max_correspondence_distance=0.5,
                                             fitness_max_range=0.25, ctx=ctx,
                                             return_hypotheses=True, return_stats=True)
    assert st["fitness"] > 0.0  # (compute_fitness ran: the registration's pass over the staging)
    return blob(final, aligned, np.array([h["E"] % 2**63 for h in hyp], np.int64),
                np.array([h["match"] for h in hyp]), st)


def icp(ctx, n, seed):
    tgt = cloud(n, seed)
    src = tgt[:n * 3 // 4] + f32(0.02)  # (part of the target, moved; its holes too)
    final, aligned, st = D.icp_align(src, tgt, indices=some(src.shape[0], 2), max_iterations=4,
                                     max_correspondence_distance=1.0, fitness_max_range=0.25,
                                     ctx=ctx, return_stats=True)
    st.pop("state_name")
    return blob(final, aligned, st)


def sor(ctx, n, seed):
    kept, removed, dist, st = D.statistical_outlier_removal(cloud(n, seed), 8, 1.0,
                                                            indices=some(n, 3), ctx=ctx,
                                                            return_stats=True)
    return blob(kept, removed, dist, st)


def sor_cloud(ctx, n, seed):
    cl, kept, st = D.statistical_outlier_removal_cloud(cloud(n, seed), 8, 1.0, id_base=7, ctx=ctx,
                                                       return_stats=True)
    sig = cl.signature()  # (every coordinate bit and id of the cloud handed out)
    cl.close()
    return blob(kept, np.array([sig], np.uint64), st)


def mls(ctx, n, seed):
    xyz, nrm, src, nb, st = D.moving_least_squares(cloud(n, seed), 0.6, indices=some(n, 2), ctx=ctx,
                                                   return_stats=True)
    return blob(xyz, nrm, src, nb, st)


def fpfh(ctx, n, seed):
    p = cloud(n, seed)
    nrm = np.random.default_rng(seed).normal(size=(n, 3)).astype(f32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    hist, nb, st = D.fpfh_estimation(p, nrm, 0.6, indices=some(n, 4), ctx=ctx, return_stats=True)
    return blob(hist, nb, st)


def voxel(ctx, n, seed):
    xyz, cnt, voe, st = D.voxel_grid(cloud(n, seed), 0.3, indices=some(n, 2), ctx=ctx,
                                     return_stats=True)
    return blob(xyz, cnt, voe, st)


def normals(ctx, n, seed):
    return blob(D.estimate_normals(cloud(n, seed, holes=False), k=20, ctx=ctx))


CALLS = [sac_ia, icp, sor, sor_cloud, mls, fpfh, voxel, normals]
# points per call: large and small by turns, forwards and then backwards with the turns swapped
FORWARD = [3000, 700, 4096, 300, 2500, 600, 3500, 900]
BACKWARD = [450, 3600, 350, 4000, 400, 3000, 500, 2000]


def test_one_context_through_every_call_equals_a_context_each():
    steps = [(f, n, 40 + i) for i, (f, n) in enumerate(zip(CALLS, FORWARD))]
    steps += [(f, n, 60 + i) for i, (f, n) in reversed(list(enumerate(zip(CALLS, BACKWARD))))]
    shared = D.Context(0)
    got = [f(shared, n, seed) for f, n, seed in steps]
    shared.close()
    for (f, n, seed), g in zip(steps, got):
        lone = D.Context(0)
        want = f(lone, n, seed)
        lone.close()
        assert g == want, (f.__name__, n)
