"""CPU: bench.py's multi-GPU harness (VERDICT r1 missing #2). `python bench.py --gpus N` started by
hand launches the N ranks itself (enf_launch.py: torch.distributed.run child processes, before
anything touches a device); each rank times its share, the wall time is the max over ranks and
`value` aggregates all ranks' samples. Exercised here with gloo and a CPU stand-in step
(--selftest-cpu); on the GPU box the same harness runs on RCCL with the enf_flow_apply step."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def run_bench(*args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                            "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--selftest-cpu", "--no-cpu", "--steps", "3",
                        "--warmup", "1", "--N", "1000", *args], capture_output=True, text=True, timeout=240, env=env,
                       cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_single_rank_line():
    out = run_bench()
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 1
    # the settle phase is reported in the line (the CPU stand-in step never settles a GPU clock)
    assert out["settle"]["launches"] == 0 and "steady clock" in out["settle"]["why"]
    assert out["distributed"]["world_size"] == 1 and len(out["distributed"]["per_rank_kernel_ms"]) == 1
    assert out["value"] == pytest.approx(1000 * 3 / (out["ms_per_step"] * 3 / 1e3), rel=1e-6)
    # a plain run (no --full) measures the headline only: no leg beside it
    assert out["train"] is None and out["cpu_baseline"] is None and out["warm"] is None
    assert out["roofline"]["copy_ceiling"] is None and out["valu"] is None


def test_bench_dump_columns_are_fixed_and_bounded():
    """--dump-outputs: all columns while Y and ladj fit the dump's byte bound, else a sample of distinct columns,
    ascending, identical from call to call, whose Y and ladj stay within the bound (far under 64 MB)."""
    import numpy as np

    import bench

    assert bench.dump_columns(1000, 32, 4) is None
    assert bench.DUMP_BYTES <= 64 * 10**6
    for D, esz in ((32, 4), (32, 8), (2, 8)):
        a, b = bench.dump_columns(10_000_000, D, esz), bench.dump_columns(10_000_000, D, esz)
        assert np.array_equal(a, b) and np.all(np.diff(a) > 0) and 0 <= a[0] and a[-1] < 10_000_000
        assert a.size * (D + 1) * esz <= bench.DUMP_BYTES < (a.size + 1) * (D + 1) * esz


@pytest.mark.gpu
def test_bench_dump_outputs_match_oracle(gpu, oracle, tmp_path):
    """A plain run with --dump-outputs on the GPU: --steps sets the timed steps, the line carries ms_per_step and
    no leg beside the headline, and DIR/Y.npy (D x N) / DIR/ladj.npy (N) hold what the timed path computed (the
    oracle on the same seeded inputs, tests/parity.py's fp32 criterion); a second run writes the same values.
    N = 4099: several blocks and a column tail; a set this small is timed over the rotating buffer sets as one
    graph replay, so the dump reads the set of the last captured launch."""
    import numpy as np
    import torch

    import bench
    import parity

    D, N = 32, 4099
    outs = []
    for d in ("a", "b"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup",
                            "1", "--N", str(N), "--settle-ms", "0", "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=240, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
        assert line["value"] == pytest.approx(N * 3 / (line["ms_per_step"] * 3 / 1e3), rel=1e-6)
        assert line["train"] is None and line["cpu_baseline"] is None and line["roofline"]["copy_ceiling"] is None
        assert sorted(os.listdir(tmp_path / d)) == ["Y.npy", "ladj.npy"]
        outs.append((np.load(tmp_path / d / "Y.npy"), np.load(tmp_path / d / "ladj.npy")))
    (Y, L), (Y2, L2) = outs
    assert Y.dtype == np.float32 and L.dtype == np.float32 and Y.shape == (D, N) and L.shape == (N,)
    assert np.array_equal(Y, Y2) and np.array_equal(L, L2)
    g = torch.Generator(device=gpu).manual_seed(0x5EED)
    X = torch.randn((N, D), generator=g, device=gpu, dtype=torch.float32).cpu().numpy().T
    parity.check_vs_oracle(oracle, bench.build_flow(D, 4, np.float32), np.asfortranarray(X), Y, L, np.float32,
                           what="bench --dump-outputs")


def test_bench_launches_two_ranks():
    out = run_bench("--gpus", "2", "--full")  # (--full: the config-5 leg beside the headline)
    assert out["n_gpus"] == 2
    d = out["distributed"]
    assert d["world_size"] == 2 and d["backend"] == "gloo" and d["data_path_collective"] is None
    assert len(d["per_rank_kernel_ms"]) == 2 and all(v > 0 for v in d["per_rank_kernel_ms"])
    # whole-job aggregate: both ranks' samples over the max-over-ranks wall time
    assert out["value"] == pytest.approx(2 * 1000 * 3 / (out["ms_per_step"] * 3 / 1e3), rel=1e-6)
    assert out["scaling"] == "weak" and out["config"]["N_total"] == 2000
    # the config-5 leg at N = 2: minibatch shares tile every batch, the ranks agree, and the step the GPU
    # run times is the graph-captured libenf RCCL (EnfComm) data-parallel step
    t = out["train"]
    assert t["n_gpus"] == 2 and t["ranks_agree"] and len(t["per_rank_s"]) == 2
    assert "EnfComm" in t["step"] and "captured in the HIP graph" in t["step"]


@pytest.mark.parametrize("gpus", [1, 2, 3])
def test_bench_strong_scaling_line(gpus):
    """--scaling strong: the N = 1000 columns are split over the ranks in contiguous shards
    (1000 = 333 + 333 + 334 at three ranks), value = N x steps / the max-over-ranks time, "scaling": "strong"."""
    out = run_bench("--gpus", str(gpus), "--scaling", "strong", "--no-train")
    assert out["n_gpus"] == gpus and out["scaling"] == "strong"
    c = out["config"]
    assert c["N_total"] == 1000 and c["N_per_gpu"] == 1000 // gpus  # (rank 0: [0, 1000 // gpus))
    assert "in all, split over" in c["workload"]
    assert out["value"] == pytest.approx(1000 * 3 / (out["ms_per_step"] * 3 / 1e3), rel=1e-6)


def test_bench_world_mismatch_is_an_error():
    env = {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--selftest-cpu", "--gpus", "2", "--no-cpu"],
                       capture_output=True, text=True, timeout=120, env={**os.environ, **env}, cwd=ROOT)
    assert p.returncode != 0 and "WORLD_SIZE=1" in (p.stderr + p.stdout)


def run_bench_train(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                            "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench_train.py"), "--selftest-cpu", "--steps", "7",
                        "--N", "1003", "--nbatches", "4", *args], capture_output=True, text=True, timeout=240, env=env,
                       cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("gpus", [1, 2, 3])
def test_bench_train_launches_ranks(gpus):
    """bench_train.py --gpus N starts N ranks itself; the ranks' minibatch shares tile every batch
    (asserted inside each rank) and all ranks apply the same update."""
    out = run_bench_train("--gpus", str(gpus))
    assert out["n_gpus"] == gpus and len(out["per_rank_s"]) == gpus
    assert out["ranks_agree"] and out["config"]["parallelism"] == f"dp{gpus}"
