"""CPU: the scenes of tests/pp_cases.py reach what they were built for, judged by the oracle alone
(no GPU): else tests/test_postprocess_edges_gpu.py could pass without running the branch, the
task split or the threshold it is about.
"""
import numpy as np
import pytest

import pp_cases as PC
from oracle import oracle as O
from test_postprocess import oracle_run

POP = np.array([bin(i).count("1") for i in range(1024)])


def test_oracle_parities_restate_point_in_poly():
    """orc_is_point_in_poly is the 5-of-10 vote over orc_pip_parities; orc_segs_intersect is
    callable on its own"""
    s = PC.mask_scene("l_axis")
    pl = s["planes"][1]
    ids, masks = PC.oracle_masks("l_axis")[1]
    rng = np.random.default_rng(0)
    for j in rng.choice(len(ids), 300, replace=False):
        want = O.is_point_in_poly(s["cloud"][ids[j]], pl["coeff"], pl["border"], s["t_dist"],
                                  s["seed"])
        assert want == (POP[masks[j]] >= 5)
    far = s["cloud"][:5] + np.array([0, 0, 1], np.float32)
    cand, m = O.pip_parities(far, pl["coeff"], pl["border"], s["t_dist"], s["seed"])
    assert not cand.any() and not m.any()
    # a ray along +x from (-1, 0.5, 0) crosses the edge x = 0, y in [0, 1]; from (1, 0.5, 0) not
    a, b = (0, 0, 0), (0, 1, 0)
    assert O.segs_intersect(a, b, (-1, 0.5, 0), (9999, 0.5, 0))
    assert not O.segs_intersect(a, b, (1, 0.5, 0), (10001, 0.5, 0))


@pytest.mark.parametrize("name", sorted(PC.MASK_SCENES))
def test_mask_scene_is_not_vacuous(name):
    s = PC.mask_scene(name)
    om = PC.oracle_masks(name)
    assert len(s["cloud"]) <= 10000
    pairs = sum(len(ids) * 10 * len(pl["border"]) for (ids, _), pl in zip(om, s["planes"]))
    assert pairs <= 30e6
    allm = np.concatenate([m for _, m in om])
    assert (allm == 0).any() and (allm != 0).any()
    # votes that one wrong crossing turns: 4, 5 or 6 odd rays
    # (every border but those of 1 and 2 vertices)
    area = [k for k in range(len(om)) if k not in s["tiny"]]
    if area:
        m = np.concatenate([om[k][1] for k in area])
        close = np.isin(POP[m], (4, 5, 6)).mean()
        print(name, "candidates", m.size, "close votes", close)
        assert close >= 0.05
    # the branches of the crossing test the scene is meant to reach
    tot = dict(perp=0, parallel=0, anti=0, short=0, total=0)
    for (ids, _), pl in zip(om, s["planes"]):
        c = PC.pair_classes(s["cloud"][ids], pl["coeff"], pl["border"], s["seed"])
        for k in tot:
            tot[k] += c[k]
        # every edge of the short class carries its share: none is there in name only
        for j, (dab, pairs) in c["short_by_edge"].items():
            assert pairs >= 100, (name, j, dab, pairs)
    print(name, tot)
    for k in s["hits"]:
        assert tot[k] >= 100, (k, tot)


def test_mask_scenes_cover_every_branch_and_size():
    hit = set()
    for name in PC.MASK_SCENES:
        hit |= set(PC.mask_scene(name)["hits"])
    assert hit == {"perp", "parallel", "anti", "short"}
    fv = PC.mask_scene("few_vertices")
    assert [len(p["border"]) for p in fv["planes"]] == [1, 2, 3, 3] and fv["tiny"] == (0, 1)
    for name in PC.MASK_SCENES:  # only borders of 1 and 2 vertices are spared the close votes
        assert PC.mask_scene(name)["tiny"] == ((0, 1) if name == "few_vertices" else ())
    # the collinear 3-vertex border and the triangle each have close votes of their own
    for k in (2, 3):
        assert np.isin(POP[PC.oracle_masks("few_vertices")[k][1]], (4, 5, 6)).sum() >= 100
    # the short class, edge by edge: the 1e-16 edge and the exactly-0 edge of short_edges, the
    # duplicate vertex of the L, the single vertex (edge to itself) of the 1-vertex border
    def short_edges_of(name, k):
        s = PC.mask_scene(name)
        ids = PC.oracle_masks(name)[k][0]
        pl = s["planes"][k]
        return PC.pair_classes(s["cloud"][ids], pl["coeff"], pl["border"], s["seed"])["short_by_edge"]
    for k in (0, 1):
        se = short_edges_of("short_edges", k)
        assert sorted(se) == [0, 2] and 0 < se[0][0] <= 1.0001e-16 and se[2][0] == 0.0
        assert se[0][1] >= 10000 and se[2][1] >= 10000
    assert {j: v[0] for j, v in short_edges_of("l_axis", 1).items()} == {2: 0.0}
    assert {j: v[0] for j, v in short_edges_of("few_vertices", 0).items()} == {0: 0.0}
    assert short_edges_of("few_vertices", 3) == {}
    # the 1000-gon: 600 candidates = 3 blocks, 63 tasks per block, the last of 8 edges; the
    # 16-gon is one task per block, the 17-gon a second task of one edge
    om = PC.oracle_masks("many_edges")
    counts = [len(ids) for ids, _ in om]
    assert counts == [600, 600, 600]
    cblocks, split, chunks, per_block = PC.task_split(counts, [1000, 16, 17])
    assert cblocks == 9 and chunks == [16, 16, 16] and per_block == [63, 1, 2]
    assert 1000 - 62 * 16 == 8
    # the long borders: |ab| of 4000, and candidates thousands of units from the first vertex
    s = PC.mask_scene("long_1")
    assert np.abs(s["cloud"][:, :2]).max() > 3900
    # far from the origin the coordinates are of order 1e5
    assert np.abs(PC.mask_scene("l_moved_2")["cloud"]).min(axis=0).max() > 4e4


# ---- the full entry's scenes ---------------------------------------------------------------------
def candidates(cloud, planes, co, k, t_dist=0.1, seed=12345):
    """unprocessed candidates of plane k before any absorption (what the device counts)"""
    proc = PC.nearest_marks(cloud, np.concatenate([np.asarray(p["points"]).reshape(-1, 3)
                                                   for p in planes]))
    cand, _ = O.pip_parities(cloud, co[k], planes[k]["border"], t_dist, seed)
    return cand & ~proc


@pytest.mark.parametrize("count,split,chunk", [(2100, 1, 40), (1100, 2, 20)])
def test_identical_planes_split(count, split, chunk):
    cloud, planes = PC.identical_planes(count)
    co, ab, rem = oracle_run(cloud, planes[:1], radius=0.5, tnum=0)
    c = candidates(cloud, planes[:1], co, 0)
    assert 1 <= c.sum() <= 8 and 0 < ab[0].size < c.sum()
    cb, sp, chunks, per_block = PC.task_split([int(c.sum())] * count, [40] * count)
    assert (cb, sp, chunks[0], per_block[0]) == (count, split, chunk, 40 // chunk)
    assert count > 64  # a second block of the range kernel, more than 6 plane bits in the key


def test_nan_middle_scene():
    cloud, planes = PC.nan_middle()
    for start in (0, 1):
        co, ab, rem = oracle_run(cloud, planes, start=start)
        assert np.isnan(co[1]).all() and np.isfinite(co[[0, 2, 3]]).all()
        assert ab[1].size == 0 and ab[2].size > 50 and ab[3].size > 50
        assert (ab[0].size > 50) == (start == 0)


@pytest.mark.parametrize("k", [1, 256, 257])
def test_exact_candidate_counts(k):
    cloud, planes = PC.exact_candidates(k)
    co, ab, rem = oracle_run(cloud, planes)
    assert candidates(cloud, planes, co, 0).sum() == k


def test_overlapping_planes_share_points():
    cloud, planes = PC.overlapping()
    co, ab, rem = oracle_run(cloud, planes)
    assert np.intersect1d(ab[0], ab[1]).size > 50
    assert np.setdiff1d(ab[0], ab[1]).size > 50 and np.setdiff1d(ab[1], ab[0]).size > 50


def test_degenerate_clouds():
    cloud, planes = PC.one_spot(50)
    assert (cloud.max(axis=0) == cloud.min(axis=0)).all()
    co, ab, rem = oracle_run(cloud, planes, tnum=0)
    assert np.array_equal(ab[0], np.arange(1, 50)) and rem.size == 0  # point 0: the 1-NN mark
    cloud, planes = PC.one_spot(50, inside=False)
    assert oracle_run(cloud, planes, tnum=48)[2].size == 49
    assert oracle_run(cloud, planes, tnum=49)[2].size == 0
    cloud, planes = PC.one_spot(1)
    co, ab, rem = oracle_run(cloud, planes, tnum=0)
    assert ab[0].size == 0 and rem.size == 0
    assert oracle_run(cloud, [], tnum=0)[2].size == 1


def test_nn_ties_scene():
    cloud, planes, base = PC.nn_ties()
    proc = PC.nearest_marks(cloud, planes[0]["points"])
    want = []
    for q in base:  # every repeated point: its lowest index
        same = np.nonzero((cloud.view(np.uint32) == q.view(np.uint32)).all(axis=1))[0]
        assert same.size in (3, 1000)
        want.append(same[0])
    up = np.nonzero((cloud == np.array([1, 1, 0.05], np.float32)).all(axis=1))[0]
    dn = np.nonzero((cloud == np.array([1, 1, -0.05], np.float32)).all(axis=1))[0]
    assert up.size == 1 and dn.size == 1
    want.append(min(up[0], dn[0]))  # the plane point (1, 1, 0) is midway: the lower index
    neg = np.nonzero(np.signbit(cloud[:, 0]) & (cloud[:, 0] == 0))[0]
    assert neg.size == 2
    want.append(neg[0])  # -0.0 in the cloud equals the plane point's +0.0
    assert np.array_equal(np.nonzero(proc)[0], np.sort(want))
    # the marks show in the outputs: the other copies are absorbed, the marked ones are not
    co, ab, rem = oracle_run(cloud, planes, tnum=0)
    assert not np.isin(np.nonzero(proc)[0], ab[0]).any() and not np.isin(np.nonzero(proc)[0], rem).any()
    assert max(up[0], dn[0]) in ab[0] and neg[1] in ab[0] and ab[0].size > 1000


# ---- clusterFilt ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PC.cluster_cases()))
def test_cluster_case_keeps_what_it_was_built_for(name):
    p, r, T, kept = PC.cluster_cases()[name]
    assert int(O.cluster_filter(p, r, T).sum()) == kept


def test_cluster_cases_cover_the_thresholds():
    C = PC.cluster_cases()
    for T in (0, 1, 63, 64, 255, 256):
        p, lab, sizes = PC.sized_components(T)
        keep = O.cluster_filter(p, 0.25, T)
        for j, sz in enumerate(sizes):  # size T (and below) goes, size T + 1 stays
            assert keep[lab == j].all() == (sz > T) and keep[lab == j].any() == (sz > T)
        assert T + 1 in sizes and (T in sizes or T == 0)
    assert C["duplicates_T1"][0].shape[0] == 605
    lt = C["lattices_T1499"][0]
    d = np.linalg.norm(lt[0::2].astype(np.float64) - lt[1::2], axis=1)
    assert (d > 0.25).all() and (d < 0.3).all()  # the two lattices: apart, yet in shared cells
    assert (np.floor(lt[0::2] / 0.25) == np.floor(lt[1::2] / 0.25)).all(axis=1).mean() > 0.4
