"""Cost of the layer-wise optimizers (FusedMLPTrainer(optimizer="lars" | "lamb"), the two-launch
kernels of csrc/kernels/optim.hip) over ``adam`` on the same engine: us per step of the
graph-replay ``run()`` path at B = 100 and B = 4096 (f32) on a resident dataset of 65,536 rows.

adam, lars and lamb are interleaved in ONE process, ``--windows`` (5) windows each, a window sized
to about ``--window`` seconds from a calibration run; all three are warmed first.  At B = 100 adam
runs the two-launch pipelined step (its update is inside the first launch) while lars / lamb run
the gradient-buffer engine, so that row compares engines as well as rules; at B = 4096 all three
run the large-batch engine and differ in the apply launches alone.  Prints one JSON line; run it
from two fresh processes and take the medians (profiles/layerwise/README.md).

    python tools/probes/layerwise_cost.py [--windows 5] [--window 0.25]
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
from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer  # noqa: E402

KINDS = ("adam", "lars", "lamb")


def timed(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--sizes", default="100,4096")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    x, y = mnist_like_device(a.rows, seed=100, device=dev)
    y = y.int()
    p = init_params(dev, seed=0)
    rows = []
    for B in (int(s) for s in a.sizes.split(",")):
        trs = {k: FusedMLPTrainer(p, x, y, batch_size=B, learning_rate=1e-3, optimizer=k,
                                  weight_decay=0.01) for k in KINDS}
        for t in trs.values():
            t.run(1, use_graph=False)
            t.run(2 * t.nbatches)  # every graph once
        k = {n: max(20, int(a.window * 1e6 / timed(t.run, 50))) for n, t in trs.items()}
        us = {n: [] for n in KINDS}
        for _ in range(a.windows):
            for n in KINDS:
                us[n].append(timed(trs[n].run, k[n]))
        med = {n: sorted(v)[len(v) // 2] for n, v in us.items()}
        rows.append({
            "batch": B, "engine": {n: "two_launch" if t.pipelined else "gradient_buffer"
                                   for n, t in trs.items()},
            "steps_per_window": k,
            "us_per_step": {n: [round(v, 2) for v in us[n]] for n in KINDS},
            "median_us_per_step": {n: round(v, 2) for n, v in med.items()},
            "us_over_adam": {n: round(med[n] - med["adam"], 2) for n in KINDS[1:]},
            "loss": {n: round(t.stats()[0], 4) for n, t in trs.items()},
        })
    print(json.dumps({"rows": a.rows, "windows": a.windows, "sizes": rows}), flush=True)


if __name__ == "__main__":
    main()
