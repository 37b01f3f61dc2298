"""bench.py's launch contract on a machine without GPUs: a bare `python bench.py --gpus 2` must spawn its own two ranks
(one process per GPU through torch.distributed.run on 127.0.0.1) instead of refusing, and each rank must fail loudly --
"no GPU visible", exit code 3 -- because the engine has no CPU fallback."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def no_gpu_spawn_env():
    """The environment of a bare multi-rank launch whose every rank must reach its own device check.  torch.distributed.run stops the
    surviving ranks at its first poll after one rank exits (every 0.1 s by default): a rank that reached its check while its sibling was
    still importing torch got the sibling killed before it could say "no GPU visible" -- on a loaded machine, two launches in 24 printed
    the message once.  Polling every 30 s (PET_MONITOR_INTERVAL: torchrun's --monitor-interval) lets both ranks get there first."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["PET_MONITOR_INTERVAL"] = "30"
    return env


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check of the spawn path")
def test_bare_multi_gpu_launch_spawns_ranks():
    env = no_gpu_spawn_env()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and p.returncode != 2
    assert p.stderr.count("no GPU visible; the engine has no CPU fallback") == 2, p.stderr[-2000:]
    assert p.stdout.strip() == ""


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_single_gpu_without_device_fails_loudly():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 3 and "no CPU fallback" in p.stderr and p.stdout.strip() == ""


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check of the spawn path")
def test_config_arguments_reach_every_spawned_rank():
    """`python bench.py --config 3 --gpus 2 ...`: the self-spawn forwards the whole command line, so both ranks parse
    `--config 3` (a rank that lost it would still die on "no GPU", so the argument echo is checked through an unknown flag:
    argparse's error names it on every rank)."""
    env = no_gpu_spawn_env()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "3", "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and p.stderr.count("no GPU visible; the engine has no CPU fallback") == 2, p.stderr[-2000:]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "3", "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--substeps", "7", "--bogus-flag"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--bogus-flag" in p.stderr  # rejected before any spawn: one parser, one command line
    assert p.stdout.strip() == ""


@pytest.mark.gpu
def test_forced_single_rank_exchange_line_fields():
    """On the GPU box: the RCCL path of bench.py with ONE rank (MJB_BENCH_FORCE_GATHER=1) -- init_process_group("nccl"),
    ExternalStream interop, the side-stream all-gather / all-reduces and the final barrier all run; the line must say so."""
    import json
    env = dict(os.environ, MJB_BENCH_FORCE_GATHER="1", MASTER_PORT="29533")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--substeps", "100",
                        "--no-cpu-baseline", "--no-other-configs"], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["config"]["rccl_ranks"] == 1 and line["value"] > 0 and line["scaling"] == "weak"
    assert line["metrics"]["env_steps"] == 4096 * 100 * 4 and line["metrics"]["nenv"] == 4096  # reduced over the (one) rank
    assert "forced single-rank gather: sensordata round trip ok" in p.stderr


# ---- the N-rank control flow without GPUs: `--dry-ranks N` = rendezvous with a timeout, shard ranges, the real
# OverlappedExchange on thread streams, barrier fences, per-rank times gathered + MAX over ranks, the rank-0 line, exit codes ----
def _run_bench(*argv, timeout=300):
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=timeout)
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    return p, lines


@pytest.mark.parametrize("ranks", [1, 2, 4, 8])
def test_dry_ranks_print_one_line_from_rank_zero(ranks):
    p, lines = _run_bench("--dry-ranks", str(ranks), "--steps", "3", "--warmup", "1", "--full")
    assert p.returncode == 0, p.stderr[-3000:]
    assert len(lines) == 1 and p.stdout.count("\n") == 1      # ONE line on stdout (gloo's banners went to stderr)
    line = lines[0]
    assert line["n_gpus"] == ranks and line["dry_ranks"] == ranks and line["steps"] == 3 and line["warmup"] == 1
    assert line["exchange_ok"] is True                        # every rank's shard of the LAST launch arrived, metrics SUM / MAX right
    assert line["scaling"] == "weak" and line["higher_is_better"] is True and "DRY RUN" in line["data"]
    assert 0 < line["rank_ms_per_step"]["min"] <= line["rank_ms_per_step"]["max"] <= line["ms_per_step"] * 1.0000001
    assert line["exchange_ms"] is not None and line["exchange_ms"] >= 0
    assert abs(line["value"] - ranks * 64 * 10 * 3 / (line["ms_per_step"] * 3e-3)) < 1e-6 * line["value"]   # whole-job aggregate
    assert line["config"]["gloo_ranks"] == ranks              # what the process group says, not the environment variable
    assert line["cpu_baseline_leg"] is (ranks == 1)           # the CPU leg runs on rank 0 at N = 1 only


@pytest.mark.parametrize("ranks", [1, 2])
def test_plain_dry_run_has_no_cpu_leg(ranks):
    """Without --full the line carries the headline alone: no rank runs the CPU baselines, N = 1 included."""
    p, lines = _run_bench("--dry-ranks", str(ranks), "--steps", "3", "--warmup", "1")
    assert p.returncode == 0 and len(lines) == 1, p.stderr[-3000:]
    line = lines[0]
    assert line["n_gpus"] == ranks and line["steps"] == 3 and line["warmup"] == 1 and line["exchange_ok"] is True
    assert line["cpu_baseline_leg"] is False
    assert abs(line["value"] - ranks * 64 * 10 * 3 / (line["ms_per_step"] * 3e-3)) < 1e-6 * line["value"]


def test_world_size_mismatch_fails_the_line():
    """A launcher that started fewer ranks than --gpus / --dry-ranks asks for must not produce a line that looks like an N-rank one."""
    import json
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-ranks", "2", "--steps", "2", "--warmup", "1", "--dist-timeout", "20"],
                       env=env, capture_output=True, text=True, timeout=120)
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode != 0 and len(lines) == 1 and "error" in lines[0] and "process group has 1 rank" in lines[0]["error"]


@pytest.mark.parametrize("bad", [0, 1])
def test_a_failing_rank_ends_in_one_error_line_not_a_hang(bad):
    p, lines = _run_bench("--dry-ranks", "2", "--steps", "3", "--warmup", "1", "--dry-fail-rank", str(bad), "--dist-timeout", "20", timeout=120)
    assert p.returncode != 0
    assert len(lines) == 1 and "error" in lines[0] and lines[0]["rank"] == 0
    assert f"injected failure on rank {bad}" in lines[0]["error"]
    assert "value" not in lines[0]


# ---- --dump-outputs DIR: what the timed path computed in its last step, as DIR/<name>.npy (float64, <= 64 MB, seeded env sample beyond)
def _load_dump(d):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


@pytest.mark.parametrize("ranks", [1, 2])
def test_dry_run_dumps_the_last_step(tmp_path, ranks):
    import numpy as np
    p, lines = _run_bench("--dry-ranks", str(ranks), "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out"))
    assert p.returncode == 0 and len(lines) == 1 and lines[0]["steps"] == 3, p.stderr[-3000:]
    d = _load_dump(tmp_path / "out")
    assert set(d) == {"env_index", "sensordata", "metrics"} and all(a.dtype == np.float64 for a in d.values())
    # the stub's launch k writes 1000 k + rank into its shard: the dump holds launch W + K = 4, every rank's envs
    want = np.repeat(1000.0 * 4 + np.arange(ranks), 64)
    assert d["sensordata"].shape == (64 * ranks, 8) and np.array_equal(d["sensordata"], np.repeat(want[:, None], 8, axis=1))
    assert np.array_equal(d["env_index"], np.arange(64 * ranks)) and d["metrics"][0] == ranks * 64 * 10 * 4


def test_dump_outputs_samples_the_same_envs_within_the_budget(tmp_path):
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    a, b = np.arange(20000.0).reshape(2000, 10), -np.arange(6000.0).reshape(2000, 3)
    keep = [bench.dump_outputs(str(tmp_path / k), {"a": a, "b": b, "empty": np.zeros((2000, 0))}, {"m": np.ones(16)}, max_bytes=80000)
            for k in ("x", "y")]
    x, y = _load_dump(tmp_path / "x"), _load_dump(tmp_path / "y")
    assert keep[0] == keep[1] and 0 < keep[0] < 2000 and set(x) == {"env_index", "a", "b", "m"}
    assert sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x")) <= 80000
    i = x["env_index"].astype(int)
    assert np.array_equal(x["env_index"], y["env_index"]) and np.all(np.diff(i) > 0)     # fixed seed: the same rows every time
    assert np.array_equal(x["a"], a[i]) and np.array_equal(x["b"], b[i]) and np.array_equal(x["m"], np.ones(16))
    assert bench.dump_outputs(str(tmp_path / "z"), {"a": a}) == 2000 and np.array_equal(_load_dump(tmp_path / "z")["a"], a)


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_full_adds_the_rest():
    """A plain default run prints the headline line without the parts that take runs of their own; --full adds the roofline block
    from its own five single-launch kernel samples (the CPU baselines and other_configs are dropped here by their flags)."""
    p, lines = _run_bench("--steps", "1", "--warmup", "0", timeout=600)
    assert p.returncode == 0 and len(lines) == 1, p.stderr[-3000:]
    line = lines[0]
    assert line["metric"] == "env_steps_per_sec" and line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["config"]["envs_per_gpu"] == 4096 and line["config"]["physics_steps_per_launch"] == 1000
    assert abs(line["value"] - 4096 * 1000 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert not {"roofline", "cpu_baseline", "other_configs"} & set(line)
    p, lines = _run_bench("--steps", "1", "--warmup", "0", "--envs", "256", "--substeps", "20", "--full", "--no-cpu-baseline",
                          "--no-other-configs", timeout=600)
    assert p.returncode == 0 and len(lines) == 1, p.stderr[-3000:]
    line = lines[0]
    assert line["roofline"]["kernel_ms_samples"]["n"] == 5 and line["roofline"]["kernel_ms"] > 0
    assert not {"cpu_baseline", "other_configs"} & set(line)


@pytest.mark.gpu
def test_dump_outputs_is_the_last_timed_step_and_repeats(tmp_path):
    """Two runs with the same arguments dump the same arrays; their clock says exactly W + K launches of S physics steps ran
    (--steps sets the timed steps), and the state is what the engine computes for the same inputs outside bench.py."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from mujoco_ros_pkgs_amd import engine, mjcf
    E, S, K, W = 256, 20, 3, 1
    args = ("--steps", str(K), "--warmup", str(W), "--envs", str(E), "--substeps", str(S), "--no-cpu-baseline", "--no-other-configs")
    dumps = []
    for k in range(2):
        p, lines = _run_bench(*args, "--dump-outputs", str(tmp_path / f"run{k}"), timeout=600)
        assert p.returncode == 0 and len(lines) == 1 and lines[0]["steps"] == K and lines[0]["ms_per_step"] > 0, p.stderr[-3000:]
        dumps.append(_load_dump(tmp_path / f"run{k}"))
    a, b = dumps
    assert {"qpos", "qvel", "ctrl", "qacc", "time", "sensordata", "metrics", "env_index"} <= set(a) and set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]) or k == "metrics", k   # (metrics: an on-device reduction, summation order may vary)
    model = mjcf.load_asset("franka_like")
    assert a["qpos"].shape == (E, model["nq"]) and np.array_equal(a["env_index"], np.arange(E))
    np.testing.assert_allclose(a["time"][:, 0], (W + K) * S * model["timestep"][0], rtol=1e-12)
    model = mjcf.Model(dict(model))
    model["enableflags"] = int(model["enableflags"]) | 2
    batch = engine.Batch(engine.CompiledModel(model), E, 0)
    qpos, qvel = bench.initial_state("franka_like", model, E, seed=1000)
    batch.set("qpos", qpos)
    batch.set("qvel", qvel)
    batch.set_ctrl_noise(bench.WORKLOADS["franka_like"][1], 0.1, 12345, 0)
    for _ in range(W + K):
        batch.step(S)
    np.testing.assert_allclose(batch.get("qpos"), a["qpos"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(batch.get("qvel"), a["qvel"], rtol=0, atol=1e-10)
