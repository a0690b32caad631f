"""What a learning-rate schedule evaluated on the device costs inside the fused two-launch MLP
step: us per step at batch 100 of sgd, momentum and adam, each at the constant rate (the
unscheduled kernels) and scheduled (exponential decay, non-staircase, with warm-up: the
scheduled instantiations), through ``run_launched()`` (the C++ host loop) and ``run()`` (hipGraph
replay), the six variants interleaved window by window in ONE process.

A window is ``--steps`` steps between two device synchronisations (wall time / steps); every
trainer runs one untimed window per mode first (graph capture, code objects, caches).  The
windows go round ``--reps`` times -- sgd launched, sgd run, sgd+schedule launched, ... -- and the
medians are reported with the spread and each scheduled variant's difference to its constant one.
There is no pass / fail threshold.

    python tools/probes/lr_schedule_cost.py [--out profiles/lr_schedule] [--name cost.json]
                                            [--reps 9] [--steps 5000]

Writes ``--name`` into ``--out`` and prints the JSON line.
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
from distributedtensorflowexample_amd.ops.lr_schedule import LRSchedule  # noqa: E402
from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer  # noqa: E402

B, NBATCH, LR = 100, 55, 0.001
KINDS = ("sgd", "momentum", "adam")
MODES = ("launched", "run")


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
    ap.add_argument("--out", default=os.path.join("profiles", "lr_schedule"))
    ap.add_argument("--name", default="cost.json")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=5000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    p = init_params(dev, seed=0)
    x, y = mnist_like_device(NBATCH * B, seed=100, device=dev)
    sch = LRSchedule("exponential", 1000, 0.96, False, 500)
    variants = [(k, s) for k in KINDS for s in (False, True)]
    name = lambda k, s: k + ("+schedule" if s else "")  # noqa: E731
    trainers = {}
    for k, s in variants:
        kw = {} if k == "sgd" else {"optimizer": k}
        if s:
            kw["lr_schedule"] = sch
        trainers[name(k, s)] = FusedMLPTrainer(p, x, y, B, LR, **kw)
    for tr in trainers.values():  # untimed: graph capture, first use of every code object
        for m in MODES:
            window_us(tr, m, a.steps)
    t = {n: {m: [] for m in MODES} for n in trainers}
    for _ in range(a.reps):
        for n, tr in trainers.items():  # interleaved
            for m in MODES:
                t[n][m].append(window_us(tr, m, a.steps))
    rows = {}
    for k, s in variants:
        n = name(k, s)
        rows[n] = {}
        for m in MODES:
            v = t[n][m]
            rows[n][m] = {"median": round(med(v), 3), "min": round(min(v), 3),
                          "max": round(max(v), 3), "windows": [round(u, 3) for u in v]}
            if s:
                rows[n][m]["over_constant"] = round(med(v) - med(t[k][m]), 3)
    for tr in trainers.values():
        tr.flush()
    torch.cuda.synchronize()
    last = {n: (tr.learning_rate() if tr.sched is not None else LR)
            for n, tr in trainers.items()}
    out = {"probe": "lr_schedule_cost", "device": torch.cuda.get_device_name(0), "batch": B,
           "steps_per_window": a.steps, "reps": a.reps, "unit": "us per step (wall)",
           "schedule": repr(sch), "global_step": {n: tr.global_step() for n, tr in trainers.items()},
           "last_rate": last, "variants": rows}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
