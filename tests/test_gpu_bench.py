"""bench.py's multi-rank path as the driver's N-GPU run exercises it: ``--gpus N``
without a launcher spawns N rank processes (one per GPU), each sweeps its own reference
views, and rank 0 prints one JSON line with n_gpus = N and the aggregate over all ranks.

On a one-GPU box the ranks share the card under AARMVS_SHARED_GPU=1 (gloo for the timing
collectives, since RCCL refuses two ranks on one device); without the switch ``--gpus 2``
must refuse to oversubscribe (exit 2).
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--config", "dtu_eval_800x600_n5_d256", "--planes", "2", "--steps", "1", "--warmup", "1",
         "--no-cpu", "--no-e2e", "--no-fusion", "--no-train", "--no-kernel-timing"]


def _bench(args, extra_env=None, timeout=300):
    env = dict(os.environ, **(extra_env or {}))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                          capture_output=True, text=True, timeout=timeout, cwd=ROOT)


def _line(out: str) -> dict:
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_bench_two_ranks_report_the_aggregate():
    one = _bench(["--gpus", "1"] + SMALL)
    assert one.returncode == 0, one.stderr[-3000:]
    two = _bench(["--gpus", "2"] + SMALL, {"AARMVS_SHARED_GPU": "1"})
    assert two.returncode == 0, two.stderr[-3000:]
    l1, l2 = _line(one.stdout), _line(two.stdout)
    assert l1["n_gpus"] == 1 and l2["n_gpus"] == 2
    assert l2["config"]["global_batch"] == 2 * l1["config"]["global_batch"]
    # value = hypotheses of all ranks over the max-over-ranks time
    hyp2 = 2 * 600 * 800 * 2
    assert abs(l2["value"] * l2["ms_per_step"] / 1e3 - hyp2) / hyp2 < 1e-2


def test_bench_refuses_to_oversubscribe_one_gpu():
    if torch.cuda.device_count() >= 2:
        pytest.skip("two or more GPUs visible: --gpus 2 is a real two-GPU run here")
    r = _bench(["--gpus", "2"] + SMALL)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])


PLAIN = ["--gpus", "1", "--config", "plumbing_160x128_n3_d48", "--steps", "2", "--warmup", "1"]
EXTRAS = ("roofline", "cpu_baseline", "parity", "fusion", "e2e", "train")


def test_bench_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    """A plain run reports the headline figure alone (everything else needs ``--full``), and
    ``--dump-outputs`` writes the last timed step's depth and confidence maps as float32 .npy:
    the inputs are seeded, the sweep is deterministic, so two runs write identical arrays."""
    import numpy as np
    runs = []
    for name in ("a", "b"):
        r = _bench(PLAIN + ["--dump-outputs", str(tmp_path / name)])
        assert r.returncode == 0, r.stderr[-3000:]
        runs.append(_line(r.stdout))
    for ln in runs:
        assert ln["full"] is False and ln["steps"] == 2 and ln["ms_per_step"] > 0
        assert ln["unit"] == "depth-hypotheses/s" and ln["higher_is_better"] is True
        assert all(ln[k] is None for k in EXTRAS) and ln["kernels"] == {}
        hyp = 128 * 160 * 48
        assert abs(ln["value"] * ln["ms_per_step"] / 1e3 - hyp) / hyp < 1e-2
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["conf.npy", "depth.npy"]
    for f in ("depth.npy", "conf.npy"):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and a.shape == (1, 128, 160)
        assert np.isfinite(a).all() and np.array_equal(a, b)
    d = np.load(tmp_path / "a" / "depth.npy")
    assert 425.0 <= d.min() and d.max() <= 935.0   # the hypotheses' range


def test_bench_full_reports_the_other_figures():
    """``--full`` adds the kernel-timing pass (per-kernel table, roofline) and the CPU baseline
    with its parity leg; the heavy legs are switched off here to keep the test short.  The parity bounds are smoke()'s."""
    r = _bench(PLAIN + ["--full", "--cpu-planes", "1", "--no-fusion", "--no-e2e", "--no-train"])
    assert r.returncode == 0, r.stderr[-3000:]
    ln = _line(r.stdout)
    assert ln["full"] is True and ln["kernels"] and ln["roofline"]["kernel"] in ln["kernels"]
    assert ln["cpu_baseline"]["value"] > 0
    assert ln["parity"]["cost_max_abs_err"] < 1e-4 and ln["parity"]["depth_rel_l1"] <= 1e-3


TRAIN = ["--train", "--train-planes", "4", "--steps", "2", "--warmup", "1", "--no-cpu", "--no-kernel-timing"]


def test_bench_train_mode_one_and_two_ranks():
    """``--train`` (config 4's DDP step, train.py:172, 288-307): one JSON line per run with
    n_gpus = N, samples/s = N x steps over the max-over-ranks time, finite loss and gradients,
    and (N > 1) the gradient all-reduce timed beside it."""
    one = _bench(["--gpus", "1"] + TRAIN)
    assert one.returncode == 0, one.stderr[-3000:]
    two = _bench(["--gpus", "2"] + TRAIN, {"AARMVS_SHARED_GPU": "1"}, timeout=600)
    assert two.returncode == 0, two.stderr[-3000:]
    l1, l2 = _line(one.stdout), _line(two.stdout)
    for ln, n in ((l1, 1), (l2, 2)):
        assert ln["n_gpus"] == n and ln["unit"] == "samples/s"
        assert ln["config"]["global_batch"] == n and ln["config"]["parallelism"] == f"ddp x{n}"
        assert ln["loss_and_grads_finite"]
        assert abs(ln["value"] * ln["ms_per_step"] / 1e3 - n) < 1e-2 * n
    assert l2["allreduce"]["params"] == l1["allreduce"]["params"] > 0
    assert l2["allreduce"]["ms"] > 0 and l2["allreduce"]["backend"] == "gloo"
