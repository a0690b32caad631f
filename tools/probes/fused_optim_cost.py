"""What momentum and Adam cost inside the fused two-launch MLP step: us per step of sgd,
momentum and adam at batch 100, through ``FusedMLPTrainer.run()`` (hipGraph replay) and
``run_launched()`` (the C++ host loop), the kinds interleaved window by window in ONE process.

A window is ``--steps`` steps between two device synchronisations (wall time / steps); every
trainer runs one untimed window per mode first (graph capture, code objects, caches).  The
windows go round ``--reps`` times -- sgd run, sgd launched, momentum run, ... -- and the medians
are reported with the spread.  ``--kinds sgd`` runs on a tree without the optimizer variants too
(the sgd trainer is built without optimizer arguments); with ``DTFX_PROBE_ROOT`` naming another
built checkout the package is imported from there, which is how the parent commit's sgd figure
is taken with the same probe (a second process, alternated with this tree's by the caller).

    python tools/probes/fused_optim_cost.py [--out profiles/fused_optim] [--name cost.json]
                                            [--reps 9] [--steps 5000] [--kinds sgd,momentum,adam]

Writes ``--name`` into ``--out`` and prints the JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.environ.get("DTFX_PROBE_ROOT") or os.path.dirname(os.path.dirname(
    os.path.dirname(os.path.abspath(__file__)))))

from distributedtensorflowexample_amd.data.synthetic import mnist_like_device  # noqa: E402
from distributedtensorflowexample_amd.models.mlp import init_params  # noqa: E402
from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer  # noqa: E402

B, NBATCH, LR = 100, 55, 0.001


def window_us(tr, mode, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if mode == "run":
        tr.run(steps)
    else:
        tr.run_launched(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "fused_optim"))
    ap.add_argument("--name", default="cost.json")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--kinds", default="sgd,momentum,adam")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    p = init_params(dev, seed=0)
    x, y = mnist_like_device(NBATCH * B, seed=100, device=dev)
    kinds = [k for k in a.kinds.split(",") if k]
    trainers = {k: FusedMLPTrainer(p, x, y, B, LR, **({} if k == "sgd" else {"optimizer": k}))
                for k in kinds}
    modes = ("run", "launched")
    for k in kinds:  # untimed: graph capture, first use of every code object
        for m in modes:
            window_us(trainers[k], m, a.steps)
    t = {k: {m: [] for m in modes} for k in kinds}
    for _ in range(a.reps):
        for k in kinds:  # interleaved
            for m in modes:
                t[k][m].append(window_us(trainers[k], m, a.steps))
    rows = {}
    for k in kinds:
        rows[k] = {}
        for m in modes:
            v = t[k][m]
            rows[k][m] = {"median": round(med(v), 3), "min": round(min(v), 3),
                          "max": round(max(v), 3), "windows": [round(u, 3) for u in v]}
            if k != "sgd" and "sgd" in kinds:
                rows[k][m]["over_sgd"] = round(med(v) - med(t["sgd"][m]), 3)
    for tr in trainers.values():
        tr.flush()
    torch.cuda.synchronize()
    out = {"probe": "fused_optim_cost", "device": torch.cuda.get_device_name(0), "batch": B,
           "steps_per_window": a.steps, "reps": a.reps, "unit": "us per step (wall)",
           "global_step": {k: trainers[k].global_step() for k in kinds}, "kinds": rows}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
