"""What hidden-layer dropout costs inside the fused two-launch MLP step: us per step at batch 100
through ``run_launched()`` (the C++ host loop), dropout rates 0 and 0.5 for sgd, momentum and
adam, interleaved window by window in ONE process.

A window is ``--steps`` steps between two device synchronisations (wall time / steps); every
trainer runs one untimed window first (code objects, caches).  The windows go round ``--reps``
times -- sgd 0, sgd 0.5, momentum 0, ... -- and the medians are reported with the spread.
``--rates 0 --kinds sgd`` runs on a tree without dropout too (the trainer is then built without
the argument); with ``DTFX_PROBE_ROOT`` naming another built checkout the package is imported
from there, which is how the parent commit's sgd figure is taken with the same probe in the same
session, and how a build with the other Philox placement (``-DDTFX_MLP_DROP_PLACE=0|2``: the rounds
pinned ahead of the first slab use, or after the slab sum) is measured against this one.

    python tools/probes/dropout_cost.py [--out profiles/dropout] [--name cost.json] [--reps 9]
                                        [--steps 5000] [--kinds sgd,momentum,adam] [--rates 0,0.5]

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
    ap.add_argument("--out", default=os.path.join("profiles", "dropout"))
    ap.add_argument("--name", default="cost.json")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--kinds", default="sgd,momentum,adam")
    ap.add_argument("--rates", default="0,0.5")
    ap.add_argument("--tag", default="", help="free text copied into the output (which build)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    p = init_params(dev, seed=0)
    x, y = mnist_like_device(NBATCH * B, seed=100, device=dev)
    kinds = [k for k in a.kinds.split(",") if k]
    rates = [float(r) for r in a.rates.split(",") if r]
    cases = [(k, r) for k in kinds for r in rates]

    def build(k, r):
        kw = {} if k == "sgd" else {"optimizer": k}
        if r:
            kw.update(dropout=r, dropout_seed=5)
        return FusedMLPTrainer(p, x, y, B, LR, **kw)

    trainers = {c: build(*c) for c in cases}
    for c in cases:  # untimed: first use of every code object
        window_us(trainers[c], a.steps)
    t = {c: [] for c in cases}
    for _ in range(a.reps):
        for c in cases:  # interleaved
            t[c].append(window_us(trainers[c], a.steps))
    rows = {}
    for k, r in cases:
        v = t[(k, r)]
        row = {"median": round(med(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
               "windows": [round(u, 3) for u in v]}
        if r and (k, 0.0) in t:
            row["over_rate_0"] = round(med(v) - med(t[(k, 0.0)]), 3)
        rows.setdefault(k, {})["rate_%g" % r] = row
    for tr in trainers.values():
        tr.flush()
    torch.cuda.synchronize()
    out = {"probe": "dropout_cost", "tag": a.tag, "device": torch.cuda.get_device_name(0),
           "batch": B, "steps_per_window": a.steps, "reps": a.reps, "mode": "run_launched",
           "unit": "us per step (wall)", "kinds": rows}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
