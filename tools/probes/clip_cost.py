"""Cost of clipping by the global norm (FusedMLPTrainer(clip_norm=...), csrc/kernels/optim.hip's
gnorm_partials / clip_scale and the CLIP reduce launch of mlp_large_batch.hip): us per step of the
graph-replay ``run()`` path with ``adam`` at B = 4096 and B = 100 (f32) on a resident dataset of
65,536 rows, with and without ``clip_norm``.

The two trainers are interleaved in ONE process, ``--windows`` (5) windows each, a window sized to
about ``--window`` seconds from a calibration run; both are warmed first.  At B = 4096 both run the
large-batch engine and differ in the reduce instantiation and in clip_scale standing where scale
stood: no launch added.  At B = 100 adam without clipping runs the two-launch pipelined step while
clipping selects the gradient-buffer engine (``step_grad``, ``gnorm_partials``, ``clip_scale``,
``adam_``), so that row compares engines as well.  Prints one JSON line; run it from two fresh
processes and take the medians (profiles/clip/README.md).

    python tools/probes/clip_cost.py [--windows 5] [--window 0.25]
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

KINDS = {"adam": dict(optimizer="adam"), "adam_clip": dict(optimizer="adam", clip_norm=1.0)}


def timed(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--sizes", default="4096,100")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    x, y = mnist_like_device(a.rows, seed=100, device=dev)
    y = y.int()
    p = init_params(dev, seed=0)
    rows = []
    for B in (int(s) for s in a.sizes.split(",")):
        trs = {n: FusedMLPTrainer(p, x, y, batch_size=B, learning_rate=1e-3, **kw)
               for n, kw in KINDS.items()}
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
            "clip_minus_adam_us": round(med["adam_clip"] - med["adam"], 2),
            "grad_norm": round(float(trs["adam_clip"].grad_norm.item()), 4),
            "loss": {n: round(t.stats()[0], 4) for n, t in trs.items()},
        })
    print(json.dumps({"rows": a.rows, "windows": a.windows, "sizes": rows}), flush=True)


if __name__ == "__main__":
    main()
