"""Cost of the per-epoch reshuffle of the device-resident pipeline (FusedMLPTrainer(shuffle=True),
csrc/kernels/shuffle.hip) at the workload's size: 55,000 x 784 f32 rows, batch 100, the
graph-replay ``run()`` path, K steps covering >= 8 epochs.

Shuffle off and on are timed interleaved in ONE process (>= 5 pairs); the gather alone is timed
per call and as GB/s (read + written bytes), next to a plain ``dst.copy_(src)`` of the same
bytes in the same process as the yardstick.  Prints one JSON line.

    python tools/probes/shuffle_cost.py [--epochs 10] [--pairs 5] [--rows 55000]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from distributedtensorflowexample_amd.data.synthetic import mnist_like_device  # noqa: E402
from distributedtensorflowexample_amd.models.mlp import init_params  # noqa: E402
from distributedtensorflowexample_amd.ops.shuffle import shuffle_rows_  # noqa: E402
from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer  # noqa: E402


def event_us(fn, reps):
    """Mean device time of ``fn`` over ``reps`` back-to-back calls (one untimed call first)."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def timed_run(tr, k):
    tr.prepare(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.run(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=55000)
    ap.add_argument("--batch_size", type=int, default=100)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    x, y = mnist_like_device(a.rows, seed=100, device=dev)
    y = y.int()
    p = init_params(dev, seed=0)
    trs = {m: FusedMLPTrainer(p, x, y, batch_size=a.batch_size, learning_rate=0.001,
                              shuffle=(m == "on"), shuffle_seed=1) for m in ("off", "on")}
    k = a.epochs * trs["off"].nbatches
    for tr in trs.values():  # warm: one eager step (a pending update), then every graph once
        tr.run(1, use_graph=False)
        tr.run(2 * tr.nbatches)
    us = {"off": [], "on": []}
    for _ in range(a.pairs):
        for m in ("off", "on"):
            us[m].append(timed_run(trs[m], k))
    # the gather alone, and a plain copy of the same bytes
    dx, dy = torch.empty_like(x), torch.empty_like(y)
    epoch = [0]

    def gather():
        epoch[0] += 1
        shuffle_rows_(dx, dy, x, y, 1, epoch[0])

    g_us = event_us(gather, a.reps)
    c_us = event_us(lambda: dx.copy_(x), a.reps)
    nbytes = 2 * (x.numel() * 4 + y.numel() * 4)
    med = {m: sorted(v)[len(v) // 2] for m, v in us.items()}
    nb = trs["off"].nbatches
    print(json.dumps({
        "rows": a.rows, "batch": a.batch_size, "steps_per_run": k, "epochs_per_run": a.epochs,
        "us_per_step_off": [round(v, 4) for v in us["off"]],
        "us_per_step_on": [round(v, 4) for v in us["on"]],
        "median_us_per_step": {m: round(v, 4) for m, v in med.items()},
        "overhead_pct": round(100.0 * (med["on"] / med["off"] - 1.0), 3),
        "gather_us_per_call": round(g_us, 2),
        "gather_GBs": round(nbytes / g_us / 1e3, 1),
        "copy_us_per_call": round(c_us, 2),
        "copy_GBs": round(2 * x.numel() * 4 / c_us / 1e3, 1),
        "gather_over_copy": round((nbytes / g_us) / (2 * x.numel() * 4 / c_us), 3),
        "derived_unoverlapped_pct": round(100.0 * g_us / (nb * med["off"]), 3),
    }), flush=True)


if __name__ == "__main__":
    main()
