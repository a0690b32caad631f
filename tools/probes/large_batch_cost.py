"""Cost of the large-batch engine (FusedMLPTrainer(batch_size > 256), csrc/kernels/
mlp_large_batch.hip): us per step and samples/s of the graph-replay ``run()`` path at B = 256 (the
existing two-launch step), 512, 1024, 4096 and 16384 on a resident dataset of 65,536 rows.

In the same process, interleaved with it (>= 5 pairs per batch size), the only other GPU route to
such a batch: ``models.dense.DenseClassifier(hidden=(100,), activation="sigmoid").grads`` (the
generic GEMM + autograd path, which reads loss and accuracy back every step) plus ``optim.sgd_``
on every variable.  A timed window is sized to about ``--window`` seconds from a calibration run;
both sides are warmed first.  Above 256 rows a third trainer, ``compute_dtype="bf16"``
(mlp_large_batch_bf16.hip), is interleaved with the two in the same windows: its figure is compared
with the f32 engine of the same process only (``bf16_over_f32`` > 1: bf16 is slower).  Prints one
JSON line.

    python tools/probes/large_batch_cost.py [--pairs 5] [--window 0.25]
    python tools/probes/large_batch_cost.py --trace_batch 1024   # only run(); for rocprofv3
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from distributedtensorflowexample_amd.data.synthetic import mnist_like_device  # noqa: E402
from distributedtensorflowexample_amd.models.dense import DenseClassifier  # noqa: E402
from distributedtensorflowexample_amd.models.mlp import init_params  # noqa: E402
from distributedtensorflowexample_amd.ops import mlp_step, optim  # noqa: E402
from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer  # noqa: E402

LR = 0.001


def timed(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / k


class Generic:
    """The generic path at batch ``B``: autograd gradients in TF layout, sgd_ on TF-layout copies of
    the variables, and the replica reloaded from them (what a worker's sync does)."""

    def __init__(self, p, x, y, B):
        self.model = DenseClassifier(hidden=(100,), activation="sigmoid")
        W1t, b1, W2t, b2 = mlp_step.unflatten(p)
        self.tf = [W1t.t().contiguous(), b1.clone(), W2t.t().contiguous(), b2.clone()]
        self.local = self.model.new_local(p.device)
        self.model.load_local(self.local, self.tf)
        self.x, self.y, self.B, self.pos, self.nb = x, y.long(), B, 0, x.shape[0] // B
        self.loss = float("nan")

    def run(self, k):
        for _ in range(k):
            sl = slice(self.pos * self.B, (self.pos + 1) * self.B)
            self.pos = (self.pos + 1) % self.nb
            gs, self.loss, _ = self.model.grads(self.local, self.x[sl], self.y[sl])
            for t, g in zip(self.tf, gs):
                optim.sgd_(t, g, LR)
            self.model.load_local(self.local, self.tf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--sizes", default="256,512,1024,4096,16384")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--trace_batch", type=int, default=0)
    ap.add_argument("--trace_dtype", default="fp32", choices=["fp32", "bf16"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    x, y = mnist_like_device(a.rows, seed=100, device=dev)
    y = y.int()
    p = init_params(dev, seed=0)
    if a.trace_batch:
        tr = FusedMLPTrainer(p, x, y, batch_size=a.trace_batch, learning_rate=LR,
                             compute_dtype=a.trace_dtype)
        tr.run(8)
        tr.run(200)
        torch.cuda.synchronize()
        print(json.dumps({"trace_batch": a.trace_batch, "loss": tr.stats()[0]}), flush=True)
        return
    rows = []
    for B in (int(s) for s in a.sizes.split(",")):
        tr = FusedMLPTrainer(p, x, y, batch_size=B, learning_rate=LR)
        gen = Generic(p, x, y, B)
        trh = (FusedMLPTrainer(p, x, y, batch_size=B, learning_rate=LR, compute_dtype="bf16")
               if tr.large else None)
        for t in (tr, trh):
            if t is not None:
                t.run(1, use_graph=False)
                t.run(2 * t.nbatches)  # every graph once
        gen.run(5)
        k = {"fused": max(20, int(a.window * 1e6 / timed(tr.run, 50))),
             "generic": max(10, int(a.window * 1e6 / timed(gen.run, 10)))}
        us = {"fused": [], "generic": []}
        if trh is not None:
            k["fused_bf16"], us["fused_bf16"] = k["fused"], []
        for _ in range(a.pairs):
            us["fused"].append(timed(tr.run, k["fused"]))
            if trh is not None:
                us["fused_bf16"].append(timed(trh.run, k["fused_bf16"]))
            us["generic"].append(timed(gen.run, k["generic"]))
        med = {m: sorted(v)[len(v) // 2] for m, v in us.items()}
        rows.append({
            "batch": B, "engine": "large_batch" if tr.large else "two_launch",
            "steps_per_window": k,
            "us_per_step": {m: [round(v, 2) for v in us[m]] for m in us},
            "median_us_per_step": {m: round(v, 2) for m, v in med.items()},
            "samples_per_s": {m: round(B / v * 1e6) for m, v in med.items()},
            "generic_over_fused": round(med["generic"] / med["fused"], 2),
            "loss": {"fused": round(tr.stats()[0], 4), "generic": round(gen.loss, 4)},
        })
        if trh is not None:
            rows[-1]["bf16_over_f32"] = round(med["fused_bf16"] / med["fused"], 3)
            rows[-1]["loss"]["fused_bf16"] = round(trh.stats()[0], 4)
    print(json.dumps({"rows": a.rows, "pairs": a.pairs, "sizes": rows}), flush=True)


if __name__ == "__main__":
    main()
