"""bench.py's plain run, --full and --dump-outputs.

A plain run (`bench.py --gpus 1 --steps N --warmup W`) times N steps and prints the result line
with nothing measured beside them; --full adds the legs that take runs of their own; and
--dump-outputs DIR writes what extract_planes returned in the last timed step, exactly, so that two
builds can be compared output for output.  The GPU tests run the benchmark itself (that is what
they are about) on a 200,000-point cloud: above the library's 131,072-point threshold for the
pruned scorer, the path the 10M-point headline takes.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--points", "200000", "--planes", "5", "--hyps", "512"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("refit_fast", "incl_index_build")  # (pruned_work, cpu_baseline, secondary: see below)


def run_bench(args):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, env=e,
                       timeout=300)
    return r


def result_line(r):
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def fake_result(n_inliers, id_max):
    rng = np.random.default_rng(7)
    return {"coeffs": rng.standard_normal((3, 4)).astype(np.float32),
            "offsets": np.array([0, 5, 9, n_inliers], np.int64),
            "inliers": rng.integers(0, id_max, n_inliers).astype(np.int32)}


@pytest.mark.parametrize("global_points,ft", [(1 << 24, np.float32), ((1 << 24) + 1, np.float64)])
def test_dump_outputs_is_exact(tmp_path, global_points, ft):
    """float32 only while every id is exact in it (below 2^24), float64 beyond."""
    import bench
    e = fake_result(1000, global_points)
    e["inliers"][0] = global_points - 1  # the largest id the cloud can hold
    bench.dump_outputs(str(tmp_path / "d"), e, global_points)
    got = {n: np.load(tmp_path / "d" / f"{n}.npy") for n in ("coeffs", "offsets", "inliers")}
    assert got["coeffs"].dtype == np.float32
    assert np.array_equal(got["coeffs"].view(np.uint32), e["coeffs"].view(np.uint32))
    assert got["offsets"].dtype == ft and got["inliers"].dtype == ft
    assert np.array_equal(got["offsets"].astype(np.int64), e["offsets"])
    assert np.array_equal(got["inliers"].astype(np.int64), e["inliers"].astype(np.int64))


def test_dump_outputs_samples_a_long_list_the_same_way_each_time(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_INLIERS", 1000)
    e = fake_result(5000, 1 << 20)
    bench.dump_outputs(str(tmp_path / "a"), e, 1 << 20)
    bench.dump_outputs(str(tmp_path / "b"), e, 1 << 20)
    a, b = np.load(tmp_path / "a" / "inliers.npy"), np.load(tmp_path / "b" / "inliers.npy")
    assert a.shape == (1000,) and np.array_equal(a, b)
    assert np.isin(a.astype(np.int32), e["inliers"]).all()


def test_steps_must_be_positive():
    r = run_bench(["--gpus", "1", "--steps", "0", "--dry-ranks"])
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_steps_outputs(gpu_ctx, tmp_path):
    import dialog_amd as D
    from dialog_amd.synth import SEED_BASE, plane_cloud
    d = tmp_path / "dump"
    out = result_line(run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", *SMALL,
                                 "--dump-outputs", str(d)]))
    for k in HEADLINE:
        assert k in out, k
    assert out["steps"] == 3 and len(out["step_ms"]) == 3 and out["warmup"] == 1
    assert out["ms_per_step"] > 0 and out["higher_is_better"] is True and out["dtype"] == "f32"
    # value is the timed steps' tests over their time (both printed to three decimals)
    rel = 0.0005 / out["ms_per_step"] + 0.0005 / out["value"] + 1e-6
    assert out["value"] == pytest.approx(out["tests_per_step"] / out["ms_per_step"] / 1e6, rel=rel)
    for k in FULL_ONLY:
        assert k not in out, k
    assert out["cpu_baseline"] is None and out["secondary"] is None
    assert "pruned_work" not in out["roofline"]
    # the dumped arrays are what a caller of the timed path receives (the bench's cloud and
    # parameters, restated)
    pts, _, _ = plane_cloud(200000, 5, seed=SEED_BASE + 3, shard=0)
    cloud = D.Cloud(gpu_ctx, pts)
    prm = D.make_params(0.02, max_iterations=511, probability=1.0, refit_mode=D.DLG_REFIT_PCL,
                        hypotheses_per_launch=512, gather_inliers=False)
    e = D.extract_planes(cloud, prm, max_planes=5, min_inliers=500)
    cloud.close()
    assert e["n_planes"] == out["config"]["planes_extracted"] == 5
    co, of, inl = (np.load(d / f"{n}.npy") for n in ("coeffs", "offsets", "inliers"))
    assert co.dtype == np.float32 and of.dtype == np.float32 and inl.dtype == np.float32
    assert np.array_equal(co.view(np.uint32), e["coeffs"].view(np.uint32))
    assert np.array_equal(of.astype(np.int64), e["offsets"])
    assert np.array_equal(inl.astype(np.int32), e["inliers"])


@pytest.mark.gpu
def test_full_run_adds_the_other_legs(tmp_path):
    out = result_line(run_bench(["--gpus", "1", "--full", "--steps", "2", "--warmup", "1", *SMALL,
                                 "--cpu-hyps", "64", "--cpu-threads", "4"]))
    for k in HEADLINE + FULL_ONLY:
        assert k in out, k
    assert out["steps"] == 2 and len(out["step_ms"]) == 2
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["single_thread"]["value"] > 0
    assert out["secondary"]["np_planes"] > 0 and out["secondary"]["chain_regulate_ms"] > 0
    assert out["roofline"]["pruned_work"]["pairs_evaluated_per_launch"] > 0
    assert out["roofline"]["memory_bound_passes"]["excluded"]["refit_walk_ms_per_step"] > 0
