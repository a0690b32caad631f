"""What the hidden activation costs inside the fused two-launch MLP step: us per step at batch 100
through ``run_launched()`` (the C++ host loop) for sigmoid, relu and tanh trainers, interleaved
window by window in ONE process.

A window is ``--steps`` steps between two device synchronisations (wall time / steps); every
trainer runs one untimed window first (code objects, caches).  The windows go round ``--reps``
times -- sigmoid, relu, tanh, sigmoid, ... -- and the fastest window and the median are reported
per variant.  ``--acts sigmoid`` runs on a tree without the argument too (the trainer is then built
without it); with ``DTFX_PROBE_ROOT`` naming another built checkout the package is imported from
there, which is how the parent commit's sigmoid figure is taken with the same probe in the same
session.

    python tools/probes/activation_cost.py [--out profiles/activation] [--name cost.json]
                                           [--reps 9] [--steps 5000] [--acts sigmoid,relu,tanh]

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


def window_us(tr, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.run_launched(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "activation"))
    ap.add_argument("--name", default="cost.json")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--acts", default="sigmoid,relu,tanh")
    ap.add_argument("--tag", default="", help="free text copied into the output (which build)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    p = init_params(dev, seed=0)
    x, y = mnist_like_device(NBATCH * B, seed=100, device=dev)
    acts = [k for k in a.acts.split(",") if k]

    def build(act):
        kw = {} if act == "sigmoid" else {"activation": act}
        return FusedMLPTrainer(p, x, y, B, LR, **kw)

    trainers = {k: build(k) for k in acts}
    for k in acts:  # untimed: first use of every code object
        window_us(trainers[k], a.steps)
    t = {k: [] for k in acts}
    for _ in range(a.reps):
        for k in acts:  # interleaved
            t[k].append(window_us(trainers[k], a.steps))
    rows = {}
    for k in acts:
        v = t[k]
        row = {"median": round(med(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
               "windows": [round(u, 3) for u in v]}
        if k != "sigmoid" and "sigmoid" in t:
            row["over_sigmoid"] = round(med(v) - med(t["sigmoid"]), 3)
        trainers[k].flush()
        row["last_loss"] = round(trainers[k].stats()[0], 4)
        rows[k] = row
    torch.cuda.synchronize()
    out = {"probe": "activation_cost", "tag": a.tag, "device": torch.cuda.get_device_name(0),
           "batch": B, "steps_per_window": a.steps, "reps": a.reps, "mode": "run_launched",
           "unit": "us per step (wall)", "activations": rows}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
