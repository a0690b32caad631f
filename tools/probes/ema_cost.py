"""What the moving average of the parameters costs inside the fused two-launch MLP step: us per
step at batch 100 through ``run_launched()`` (the C++ host loop), for sgd, momentum and adam
without and with the shadow plane (``ema_decay`` 0 and 0.999, and 0.999 with ``num_updates``),
interleaved window by window in ONE process.

A window is ``--steps`` steps between two device synchronisations (wall time / steps); every
trainer runs one untimed window first (code objects, caches).  The windows go round ``--reps``
times -- sgd 0, sgd ema, momentum 0, ... -- and the medians are reported with the spread.
``--variants 0`` runs on a tree without the feature too (the trainers are then built without the
arguments); with ``DTFX_PROBE_ROOT`` naming another built checkout the package is imported from
there, which is how the parent commit's sgd, momentum and adam figures are taken with the same
probe in the same session.  The ``ema_decay=0`` variants launch the parent's kernels
(profiles/ema/code_object_diff.txt), so they belong inside the parent's own spread.

    python tools/probes/ema_cost.py [--out profiles/ema] [--name cost.json] [--reps 9]
        [--steps 5000] [--kinds sgd,momentum,adam] [--variants 0,ema,ema_nu]

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

B, NBATCH, LR, DECAY = 100, 55, 0.001, 0.999
VARIANTS = {"0": {}, "ema": dict(ema_decay=DECAY),
            "ema_nu": dict(ema_decay=DECAY, ema_num_updates=True)}


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
    ap.add_argument("--out", default=os.path.join("profiles", "ema"))
    ap.add_argument("--name", default="cost.json")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--kinds", default="sgd,momentum,adam")
    ap.add_argument("--variants", default="0,ema,ema_nu")
    ap.add_argument("--tag", default="", help="free text copied into the output (which build)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    p = init_params(dev, seed=0)
    x, y = mnist_like_device(NBATCH * B, seed=100, device=dev)
    kinds = [k for k in a.kinds.split(",") if k]
    variants = [v for v in a.variants.split(",") if v]
    cases = [(k, v) for k in kinds for v in variants]

    def build(k, v):
        kw = {} if k == "sgd" else {"optimizer": k}
        kw.update(VARIANTS[v])
        return FusedMLPTrainer(p, x, y, B, LR, **kw)

    trainers = {c: build(*c) for c in cases}
    for c in cases:  # untimed: first use of every code object
        window_us(trainers[c], a.steps)
    t = {c: [] for c in cases}
    for _ in range(a.reps):
        for c in cases:  # interleaved
            t[c].append(window_us(trainers[c], a.steps))
    rows = {}
    for k, v in cases:
        w = t[(k, v)]
        row = {"median": round(med(w), 3), "min": round(min(w), 3), "max": round(max(w), 3),
               "windows": [round(u, 3) for u in w]}
        if v != "0" and (k, "0") in t:
            row["over_variant_0"] = round(med(w) - med(t[(k, "0")]), 3)
        rows.setdefault(k, {})[v] = row
    for tr in trainers.values():
        tr.flush()
    torch.cuda.synchronize()
    out = {"probe": "ema_cost", "tag": a.tag, "device": torch.cuda.get_device_name(0),
           "batch": B, "ema_decay": DECAY, "steps_per_window": a.steps, "reps": a.reps,
           "mode": "run_launched", "unit": "us per step (wall)", "kinds": rows}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
