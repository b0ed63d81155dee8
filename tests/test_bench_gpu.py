"""bench.py's contract with the driver: one JSON line on stdout with the agreed keys (task statement)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_json_line_with_the_contract_keys():
    """--full: the headline line plus every secondary measurement (latency, drop-in route, launch table, rooflines, CPU baseline)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "8", "--warmup", "1", "--cpu-frames", "2", "--full"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline", "latency_ms_single_stream", "latency_frames_per_s", "latency_ms_one_call", "whole_path",
              "roofline_mfma_all", "roofline_fps", "roofline_hbm", "launches"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 8 and d["warmup"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    # --steps is the number of timed steps, and ms_per_step is the timed region over them
    assert d["config"]["timed_steps"] == 8 and abs(d["ms_per_step"] - d["config"]["timed_seconds"] * 1e3 / 8) < 1e-9
    assert d["unit"] == "frames/s" and d["value"] > 1000 and d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    # the dominant launch of a coalesced call is a shared-MLP launch: bound by the fp32 matrix pipe, timed live
    assert r["bound"] == "mfma" and r["peak"] == 157.3 and r["unit"] == "TFLOP/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0.0 < r["frac"] < 1.0
    assert abs(r["achieved"] - r["executed_flops"] / (r["avg_launch_us"] * 1e-6) / 1e12) < 1e-6
    f = d["roofline_fps"]
    assert f["bound"] == "latency" and f["peak"] == 8000.0 and f["rounds"] == 1023 and 0.2 < f["us_per_round"] < 2.0
    assert d["roofline_mfma_all"]["bound"] == "mfma" and 0.0 < d["roofline_mfma_all"]["frac"] < 1.0
    assert {h["bound"] for h in d["roofline_hbm"]} == {"valu", "hbm"}
    tab = d["launches"]["table"]
    assert len(tab) >= 15 and abs(sum(t["us"] for t in tab) - d["launches"]["eager_one_stream_us"]) < 1.0
    cfg = d["config"]
    assert cfg["coalesce"] * cfg["frames_per_step"] == cfg["clouds_per_call"] and cfg["calls_in_flight"] >= 1
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port" and c["value"] > 0 and d["value"] > 10 * c["value"]


FULL_ONLY = ("latency_ms_single_stream", "latency_frames_per_s", "latency_ms_one_call", "frames_per_s_by_rank", "dropin", "roofline",
             "roofline_mfma_all", "roofline_fps", "roofline_hbm", "launches", "cpu_baseline")


def test_plain_bench_measures_the_headline_only():
    """Without --full the run sets up, warms up, times --steps steps and prints the line: the contract fields and none of the
    secondary measurements, with at most 30 s of the whole run spent outside the warm-up and timed steps."""
    steps, warmup = 8, 1
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "whole_path"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup and d["higher_is_better"] is True
    assert d["unit"] == "frames/s" and d["value"] > 1000 and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert d["config"]["timed_steps"] == steps and abs(d["ms_per_step"] - d["config"]["timed_seconds"] * 1e3 / steps) < 1e-9
    assert not set(FULL_ONLY) & set(d), set(FULL_ONLY) & set(d)
    assert d["whole_path"]["mfma_frac"] > 0 and d["whole_path"]["mfma_frac_executed"] is None
    assert wall - (steps + warmup) * d["ms_per_step"] * 1e-3 < 30.0, wall


def _one_json_line(p):
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_bench_gpus_2_launches_two_ranks_by_itself():
    """`python bench.py --gpus 2` with no launcher around it: bench.py re-executes itself under torch.distributed.run and the line
    reports TWO ranks (gloo backend: both ranks share the one GPU of this box; the data path has no collective)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "4", "--warmup", "1",
                        "--streams", "4", "--input-pool-mb", "16", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    d = _one_json_line(p)
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["value"] > 1000
    assert "world_size=2" in d["config"]["collective_backend"] and d["config"]["launcher"].startswith("self")
    assert "cpu_baseline" not in d            # reported at N = 1 only


def test_bench_refuses_a_world_size_that_is_not_gpus():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2"], capture_output=True, text=True, timeout=300,
                       cwd=ROOT, env=env)
    assert p.returncode != 0 and "WORLD_SIZE=1" in p.stderr


def test_bench_model_frame_sharded_two_ranks_by_itself():
    """scripts/bench_model.py --shard frames --gpus 2: config 4's frame sharding (all-reduce MAX + all-gather per attention round) on two
    self-launched gloo ranks sharing this box's GPU."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_model.py"), "--gpus", "2", "--backend", "gloo", "--shard", "frames",
                        "--clips-per-gpu", "1", "--T", "3", "--N", "2048", "--steps", "1", "--warmup", "1"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    d = _one_json_line(p)
    assert d["n_gpus"] == 2 and d["config"]["sharding"] == "frames" and d["config"]["finite"] is True and d["config"]["frames_local"] == 3


def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: the last timed step's outputs as DIR/<name>.npy (float32), the same as the path run directly on that step's
    inputs, which the bench draws from its seeded pool (warm-up steps, then one replay of every call, then the timed steps)."""
    steps, warmup, kco, ns, pool_mb = 3, 1, 2, 2, 16.0
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup), "--coalesce", str(kco),
                        "--streams", str(ns), "--input-pool-mb", str(pool_mb), "--no-cpu-baseline", "--no-dropin", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    d = _one_json_line(p)
    assert d["steps"] == steps and d["config"]["timed_steps"] == steps
    assert sorted(os.listdir(out)) == ["joints.npy", "sem_logits.npy", "verts.npy"]
    got = {n: np.load(out / f"{n}.npy") for n in ("sem_logits", "verts", "joints")}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from garment4d_amd import lbs as G
    dev = torch.device("cuda", 0)
    model, lbs_in, pool, pose_pool = bench.build_workload(dev, True, pool_mb)
    k = warmup + kco * ns + steps - 1
    smpl = lbs_in[1]
    betas, pose = pose_pool[k % len(pose_pool)]
    with torch.no_grad():
        logits = model.forward_fused(pool[k % pool.shape[0]].contiguous())[1]
        v, j = G.lbs(betas, pose, smpl["v_template"], smpl["shapedirs"], smpl["posedirs"], smpl["J_regressor"], smpl["parents"], smpl["lbs_weights"])
    assert got["sem_logits"].shape == (8, 8192, logits.shape[-1]) and got["verts"].shape == tuple(v.shape) and got["joints"].shape == tuple(j.shape)
    for name, want in (("sem_logits", logits), ("verts", v), ("joints", j)):
        np.testing.assert_allclose(got[name], want.float().cpu().numpy(), rtol=1e-5, atol=1e-5, err_msg=name)
