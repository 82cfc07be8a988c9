"""bench.py on the GPU box: as a plain process and as a rank under torch.distributed.run (a world of one still makes
the RCCL process group, so init, barrier and the found-record all-reduce on device tensors run on hardware)."""
import json
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
# --full for the stage-2 pass to --b2; the extras and the CPU baseline stay off
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--b1", "20000", "--b2", "400000", "--curves", "256", "--no-extras",
        "--no-cpu-baseline", "--full"]


def _line(cmd):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return lines[0]


def test_bench_line_has_the_contract_s_fields():
    d = _line([sys.executable, "bench.py"] + ARGS)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["unit"] == "curves/s" and d["value"] > 0
    assert d["config"]["curves_per_gpu"] == 256 and d["config"]["lanes_per_curve"] == 32
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms_avg")) <= set(d["roofline"])
    assert d["stage2"]["B2"] == 400000 and d["stage2"]["seconds"] > 0


def test_plain_bench_times_the_steps_asked_for_and_dumps_the_last_step_s_outputs(tmp_path):
    """without --full: the headline only (no stage 2, no CPU baseline, no extras), exactly --steps timed steps; the dumped
    points are the engine's own after warm-up + timed stage-1 passes on the same batch, and a second run dumps the same"""
    import numpy as np
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--b1", "20000", "--curves", "256"]
    runs = []
    for k in range(2):
        out = tmp_path / ("run%d" % k)
        d = _line([sys.executable, "bench.py"] + args + ["--dump-outputs", str(out)])
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
        assert not set(d) & {"stage2", "cpu_baseline", "saturated", "config2", "bits624", "config4", "special_form"}
        arrs = {n: np.load(out / (n + ".npy")) for n in ("X", "Z", "factor_flag", "curve", "found")}
        assert all(a.dtype == np.float64 for a in arrs.values())
        runs.append(arrs)
    assert all(np.array_equal(runs[0][n], runs[1][n]) for n in runs[0])
    X, Z = runs[0]["X"], runs[0]["Z"]
    assert X.shape == Z.shape and X.shape[0] == 256 and list(runs[0]["curve"]) == list(range(256))
    assert runs[0]["found"][0] == runs[0]["factor_flag"].sum()
    import pyecm
    n = random.Random(415).getrandbits(415) | (1 << 414) | 1
    eng = pyecm.Engine(n, digitbits=52, device=0)
    eng.build_curves(list(range(1000, 1000 + 256)))
    eng.set_lanes_per_curve(0)
    for _ in range(1 + 3):
        eng.stage1(20000)
    ex, ez = eng.download_points_plain()
    eng.close()
    val = lambda row: sum(int(v) << (52 * j) for j, v in enumerate(row))
    assert [val(r) for r in X] == ex and [val(r) for r in Z] == ez


def test_bench_as_a_rank_under_torch_distributed_run():
    d = _line([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
               "--master-port", "29541", "bench.py"] + ARGS)
    assert d["n_gpus"] == 1 and "RCCL" in d["config"]["parallelism"] and d["value"] > 0
    # the found-record all-reduce really ran, over RCCL, on a device tensor: once per step, warm-up included
    r = d["ranks"]
    assert r["process_group"] == "nccl" and r["world_size_reported_by_process_group"] == 1
    assert r["found_record_allreduces_per_rank_timed_and_warmup"] == [3]
    assert r["per_rank"][0]["global_curves"] == [0, 256] and r["per_rank"][0]["kernel_ms_avg"] > 0


def test_bench_two_ranks_with_engines_on_one_gpu():
    """`--gpus 2` from a plain process: the launcher starts two ranks; on a one-GPU box both engines sit on device 0
    (the rank's device is LOCAL_RANK modulo the visible devices) and the collectives go over gloo — RCCL does not put
    two ranks on one device.  The line counts both ranks' curves."""
    d = _line([sys.executable, "bench.py", "--gpus", "2", "--backend", "gloo"] + ARGS[2:])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["value"] > 0
    assert d["config"]["curves_per_gpu"] == 256
    assert "gloo" in d["config"]["parallelism"]
    r = d["ranks"]
    assert r["world_size_reported_by_process_group"] == 2 and r["curves_total"] == 512
    assert [x["global_curves"] for x in r["per_rank"]] == [[0, 256], [256, 512]]
    assert r["found_record_allreduces_per_rank_timed_and_warmup"] == [3, 3]
    one = _line([sys.executable, "bench.py"] + ARGS)
    assert d["config"]["curves_with_factor_last_step"] >= 0 and one["n_gpus"] == 1


def test_bench_four_ranks_rehearsal_on_one_gpu():
    """the driver's multi-GPU launch rehearsed on the box's one GPU: four ranks (the box allows six processes on the
    card), each with its own engine and its own 128 curves on device LOCAL_RANK modulo the visible devices, collectives
    over gloo.  The line adds up the ranks' curves and shows every rank's range and kernel time."""
    d = _line([sys.executable, "bench.py", "--gpus", "4", "--backend", "gloo", "--steps", "2", "--warmup", "1", "--b1", "20000",
               "--b2", "0", "--curves", "128", "--no-extras", "--no-cpu-baseline"])
    r = d["ranks"]
    assert d["n_gpus"] == 4 and r["world_size_reported_by_process_group"] == 4 and r["curves_total"] == 512
    assert [x["global_curves"] for x in r["per_rank"]] == [[128 * k, 128 * (k + 1)] for k in range(4)]
    assert all(x["kernel_ms_avg"] > 0 for x in r["per_rank"])
    assert r["kernel_ms_avg_min_over_ranks"] <= r["kernel_ms_avg_max_over_ranks"]
    assert abs(d["value"] - 512 * d["steps"] / (d["ms_per_step"] * 1e-3 * d["steps"])) < 1e-6 * d["value"]
