"""bench.py --gpus N starts its own N ranks: the launch / rendezvous / collective / relay plumbing on
CPU (BENCH_DRYRUN=1: no device work, gloo), the same code path the GPU runs take with RCCL."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the CPU baseline leg runs in the dry run too (it never needs a GPU); a sample of a fraction of a second for the tests
SMALL_CPU_SAMPLE = dict(BENCH_CPU_BUDGET_S="0.2", BENCH_CPU_SCALAR_STEPS="200", BENCH_CPU_SCALAR_FLOOR="50")


def run_bench(*argv, env_extra=None, timeout=300):
    env = dict(os.environ, BENCH_DRYRUN="1", OMP_NUM_THREADS="1", **SMALL_CPU_SAMPLE)
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("LOCAL_RANK", None)
    env.update(env_extra or {})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, env=env,
                         timeout=timeout, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout  # exactly ONE JSON line, from rank 0
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [2, 3])
def test_bench_launches_its_own_ranks(n):
    d = run_bench("--gpus", str(n), "--steps", "3", "--warmup", "1", "--full")
    assert d["dry_run"] is True and d["value"] is None
    assert d["n_gpus"] == n and d["ranks_seen"] == n  # as many ranks answered the all-gather as were asked for
    assert len(d["per_rank_env_steps_per_s"]) == n
    assert d["episodes"]["completed"] == sum(4 * (r + 1) for r in range(n))  # every rank's statistics arrived
    assert d["config"]["parallelism"] == f"env-shard x{n}" and d["scaling"] == "weak"
    assert d["metric"].startswith("env-steps/sec whole node, 65 536 QQubeSwingUpSim")
    assert "gloo" in d["collective"]
    # the CPU baseline is in the multi-rank line too: timed by the parent that starts the ranks
    cb = d["cpu_baseline"]
    assert cb and cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] == "port" and cb["scalar_all_cores"]["value"] > 0
    assert cb["timed_by"].startswith("launcher parent")
    assert d["preroll"] == 0  # (dry run: no launches; the GPU line reports BENCH_PREROLL's 400)


def test_bench_single_rank_needs_no_launcher():
    d = run_bench("--steps", "2", "--warmup", "1", "--full")
    assert d["n_gpus"] == 1 and d["ranks_seen"] == 1 and d["collective"].startswith("none")
    assert d["cpu_baseline"]["timed_by"].startswith("rank 0") and "preroll" in d


def test_plain_bench_run_is_lean():
    """without --full the line carries the headline only: no CPU baseline is timed, the timed region is not repeated"""
    for argv in (("--steps", "2", "--warmup", "1"), ("--gpus", "2", "--steps", "2", "--warmup", "1")):
        d = run_bench(*argv)
        assert d["cpu_baseline"] is None and "vs_cpu_baseline" not in d and d["repeat_ms_per_step"] == []
        assert d["steps"] == 2 and d["warmup"] == 1 and "ms_per_step" in d
        assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"


def test_bench_as_a_rank_of_an_external_launcher():
    """the driver's form: torchrun sets RANK / WORLD_SIZE and bench.py is a rank, not a launcher"""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, BENCH_DRYRUN="1", OMP_NUM_THREADS="1", **SMALL_CPU_SAMPLE)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                          "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2",
                          "--warmup", "1", "--full"], capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["timed_by"].startswith("rank 0")


def test_usable_cores_and_byte_models():
    sys.path.insert(0, ROOT)
    import bench

    assert 1 <= bench.usable_cores() <= len(os.sched_getaffinity(0))
    qq = bench.DIMS["qq-su"]
    assert bench.bytes_single_step(qq) == 117
    assert abs(bench.bytes_fused_step(qq, 100, 1) - (32.125 + 113 / 100)) < 1e-9
    assert abs(bench.bytes_fused_step(qq, 100, 2) - (52.125 + 113 / 100)) < 1e-9


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_bit_for_bit(tmp_path):
    """--dump-outputs: the last timed launch's records (a seeded lane sample) and the per-env buffers, float32 / float64,
    at most 64 MB, the same from run to run with the same arguments"""
    import numpy as np

    def run(d):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                              "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        return json.loads(lines[0])

    a, b = tmp_path / "a", tmp_path / "b"
    line = run(a)
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0 and line["cpu_baseline"] is None
    assert "large_n" not in line["roofline"] and "configs" not in line["roofline"]  # (the legs of --full)
    run(b)
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir())
    assert {"state.npy", "obs.npy", "rew.npy", "done.npy", "record_obs.npy", "record_act.npy", "record_rew.npy",
            "record_done.npy"} <= set(names)
    total = 0
    for name in names:
        x, y = np.load(a / name), np.load(b / name)
        assert x.dtype in (np.float32, np.float64), name
        total += x.nbytes
        assert np.array_equal(x, y, equal_nan=True), name
    assert total <= 64 * 2 ** 20
    n_lanes = np.load(a / "record_lanes.npy").size
    assert np.load(a / "record_obs.npy").shape == (400, n_lanes, 6) and np.load(a / "record_rew.npy").shape == (400, n_lanes)
    assert np.load(a / "state.npy").shape == (65536, 4)
