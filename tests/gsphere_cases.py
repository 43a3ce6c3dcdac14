"""Inputs of the Gaussian-sphere tests (tests/test_gauss_sphere.py asserts on the CPU that every
filtered vote of every case is stable; tests/test_gauss_sphere_gpu.py compares the library with
tests/gsphere_ref.py on them).  Small clouds, num_res 0.1 or 0.05, thresholds scaled to match."""
from __future__ import annotations

import functools

import numpy as np

import gsphere_ref as R

f32 = np.float32
# config.txt's 0.01 lattice scaled to 0.05: the radii keep their size in cells
BASE = dict(num_res=0.05, std_dev_gaussian=0.05, search_radius_create_gradient=0.15,
            t_vote_num=50, radius_base=0.15, delta_radius=0.05, s_threshold=0.9,
            dev_threshold=15.0, search_radius_for_plane_seg=0.1, t_num_of_single_plane=50)


def patch(rng, n, origin, u, v, size=1.0):
    """n random points of the parallelogram origin + a u + b v, a, b in [0, size)"""
    ab = rng.random((n, 2)) * size
    return (np.asarray(origin, f32) + ab[:, :1] * np.asarray(u, f32) +
            ab[:, 1:] * np.asarray(v, f32)).astype(f32)


def const(n, v):
    return np.tile(np.asarray(v, f32), (n, 1))


def box_corner(seed=1, n=1200):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([patch(rng, n, (0, 0, 0), (0, 1, 0), (0, 0, 1)),
                          patch(rng, n, (0, 0, 0), (1, 0, 0), (0, 0, 1)),
                          patch(rng, n, (0, 0, 0), (1, 0, 0), (0, 1, 0))])
    nrm = np.concatenate([const(n, (1, 0, 0)), const(n, (0, -1, 0)), const(n, (0, 0, 1))])
    return pts, nrm


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    pts, nrm = box_corner()
    out["box_corner"] = (pts, nrm, dict(BASE))
    rng = np.random.default_rng(7)
    out["noisy"] = (pts, unit(nrm + rng.normal(0, 0.04, nrm.shape)), dict(BASE))
    # negative components and -0.0f
    n = 900
    rng = np.random.default_rng(3)
    p3 = np.concatenate([patch(rng, n, (0, 0, 0), (1, 0, 0), (0, 0.8, 0.6)),
                         patch(rng, n, (2, 0, 0), (0, 1, 0), (0, 0, 1)),
                         patch(rng, n, (0, 3, 0), (1, 0, 0), (0, 0, 1))])
    n3 = np.concatenate([const(n, (-0.0, -0.6, 0.8)), const(n, (-1.0, -0.0, 0.0)),
                         const(n, (-0.0, -1.0, -0.0))])
    out["negative"] = (p3, n3, dict(BASE))
    # non-unit normals: the query leaves the lattice's shell, the box bound fails
    n4 = nrm.copy()
    n4[::3] *= f32(0.5)
    n4[1::3] *= f32(1.7)
    out["non_unit"] = (pts, n4, dict(BASE, num_res=0.1, std_dev_gaussian=0.1,
                                     search_radius_create_gradient=0.3, radius_base=0.3,
                                     delta_radius=0.1, dev_threshold=40.0))
    # NaN and inf normals mixed in; a point with a NaN coordinate
    n5 = out["noisy"][1].copy()
    n5[5::17, 0] = np.nan
    n5[6::29, 2] = np.inf
    n5[7::31] = -np.inf
    p5 = pts.copy()
    p5[100, 1] = np.nan
    out["non_finite"] = (p5, n5, dict(BASE))
    # two coplanar patches farther apart than the radius; a second sink beside them
    rng = np.random.default_rng(11)
    p6 = np.concatenate([patch(rng, 700, (0, 0, 0), (1, 0, 0), (0, 1, 0)),
                         patch(rng, 500, (1.5, 0, 0), (1, 0, 0), (0, 1, 0)),
                         patch(rng, 600, (0, 0, 1), (0, 1, 0), (0, 0, 1))])
    n6 = np.concatenate([const(1200, (0, 0, 1)), const(600, (1, 0, 0))])
    out["coplanar_gap"] = (p6, n6, dict(BASE))
    # equal normals, offset planes: one sink
    p7 = np.concatenate([patch(rng, 700, (0, 0, 0), (1, 0, 0), (0, 1, 0)),
                         patch(rng, 700, (0, 0, 0.5), (1, 0, 0), (0, 1, 0))])
    out["offset_planes"] = (p7, const(1400, (0, 0, 1)), dict(BASE))
    # components of 26 and 25 points beside a large one: 2 m - 1 = 51, 49
    p8 = np.concatenate([patch(rng, 400, (0, 0, 0), (1, 0, 0), (0, 1, 0)),
                         patch(rng, 26, (3, 0, 0), (1, 0, 0), (0, 1, 0), 0.05),
                         patch(rng, 25, (5, 0, 0), (1, 0, 0), (0, 1, 0), 0.05)])
    n8 = const(len(p8), (0.6, 0, 0.8))
    out["size_equal_T"] = (p8, n8, dict(BASE, t_num_of_single_plane=51))     # 26 kept, 25 dropped
    out["size_below_T"] = (p8, n8, dict(BASE, t_num_of_single_plane=52))     # 51 = T - 1: dropped
    # a sink whose total is T - 1; a sink with vote_num == t_vote_num (dropped: the test is >)
    p9 = np.concatenate([patch(rng, 300, (0, 0, 0), (0, 1, 0), (0, 0, 1)),
                         patch(rng, 99, (2, 0, 0), (1, 0, 0), (0, 0, 1)),
                         patch(rng, 50, (4, 0, 0), (1, 0, 0), (0, 1, 0))])
    n9 = np.concatenate([const(300, (1, 0, 0)), const(99, (0, 1, 0)), const(50, (0, 0, 1))])
    out["sink_total_below_T"] = (p9, n9, dict(BASE, t_num_of_single_plane=100))
    # normals all over the sphere, a wide kernel: lists beyond the register sort's 256 keys
    rng = np.random.default_rng(5)
    ns = unit(rng.normal(size=(6000, 3)))
    out["sphere"] = (ns.copy(), ns, dict(BASE, num_res=0.1, std_dev_gaussian=0.3,
                                         search_radius_create_gradient=0.3, t_vote_num=20,
                                         radius_base=0.3, delta_radius=0.1, dev_threshold=40.0,
                                         t_num_of_single_plane=20))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    pts, nrm, prm = cases()[name]
    return R.run(pts, nrm, prm)
