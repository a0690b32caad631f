"""bench.py's command line: --dump-outputs (what it writes, its size limit) and --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_writes_float_arrays_and_samples_large_ones(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    big = torch.arange(100000, dtype=torch.float32)  # 400 KB: over its share of 64 KB
    small = torch.tensor([[1.5, 2.0]], dtype=torch.float64)
    half = torch.tensor([0.25, -3.0], dtype=torch.bfloat16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small, "half": half})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "half.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 10
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert got["small"].dtype == np.float64 and got["small"].tolist() == [[1.5, 2.0]]
    assert got["half"].dtype == np.float32 and got["half"].tolist() == [0.25, -3.0]
    s = got["big"]
    assert s.dtype == np.float32 and 4000 < s.size < 100000
    assert np.all(np.diff(s) > 0) and s.max() > 90000  # distinct elements, from the whole array
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))  # the same sample every time


@pytest.mark.gpu
def test_bench_dump_outputs_is_the_trainers_state(gpu, tmp_path):
    """A plain run with --full --dump-outputs: the result line says what was timed, and the
    dumped arrays are bit for bit what the same number of steps leave in a trainer built
    from the same seeds (so two builds can be compared through the files)."""
    from distributedtensorflowexample_amd.data.synthetic import mnist_like_device
    from distributedtensorflowexample_amd.models.mlp import init_params
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                          "--steps", "20", "--warmup", "5", "--full",
                          "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert r["steps"] == 20 and r["global_step"] == r["pre_timing_steps"] + 20
    assert r["ms_per_step"] > 0 and r["unit"] == "samples/sec" and r["dtype"] == "fp32"
    assert abs(r["value"] - 100 * 1e3 / r["ms_per_step"]) <= 1e-3 * r["value"]
    assert sorted(os.listdir(tmp_path)) == ["loss_acc.npy", "params.npy"]
    params, loss_acc = np.load(tmp_path / "params.npy"), np.load(tmp_path / "loss_acc.npy")
    assert params.dtype == np.float32 and loss_acc.dtype == np.float32
    assert loss_acc.shape == (20, 2)
    assert abs(float(loss_acc[-1, 0]) - r["final_loss"]) < 1e-4

    n = r["global_step"]
    x, y = mnist_like_device(55000, seed=100, device=gpu)
    tr = FusedMLPTrainer(init_params(gpu, seed=1234), x, y, batch_size=100, learning_rate=0.001)
    tr.run(n)
    assert np.array_equal(tr.flush().cpu().numpy(), params)
    assert np.array_equal(tr.stats_range(n - 20, n).numpy(), loss_acc)
