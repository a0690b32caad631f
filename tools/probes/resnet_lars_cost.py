"""Cost of ResNet-50's LARS step (ResNetTrainer(optimizer="lars"), the two launches of
csrc/kernels/lars_mixed.hip) beside the momentum step it stands in for (sgd_momentum_mixed with
the split-K segments), at batch 256 on one GPU.

Two trainers, momentum and lars, live in ONE process and are interleaved: ``--windows`` (5)
windows of ``--steps`` graph-replayed training steps each, then the optimizer alone -- the
model's ``sgd_step`` / ``lars_step`` on the gradients of the last step, ``--reps`` eager calls
between two device events, interleaved the same way (the lars figure is the pair of launches;
their split comes from a kernel trace of this script, a run of its own).  The bytes each design
has to move are counted from the model's tables, so the times can be set against the achieved
bandwidth of the existing kernel.  Prints one JSON line; run it from fresh processes and take the
medians (profiles/resnet_lars/README.md).

    python tools/probes/resnet_lars_cost.py [--batch 256] [--windows 5] [--steps 20] [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from distributedtensorflowexample_amd.train.resnet_trainer import ResNetTrainer  # noqa: E402

KINDS = ("momentum", "lars")


def step_bytes(model):
    """Bytes per optimizer step, from the tables: today's one launch, and the LARS pair with the
    plane sum stored by launch 1 (chosen) or summed again by launch 2."""
    n = model.params.numel
    rows = model.lars_tensors()
    folded = sum(r[6] for r in rows if len(r) > 3)             # elements covered by planes
    planes = sum(r[5] * r[6] for r in rows if len(r) > 3)      # plane elements
    adapted = sum(r[1] for r in rows if r[2])
    grad = (n - folded) + planes                               # one pass over every gradient
    update = 3 * n + 2 * n + n // 2                            # p, g, v in; p, v, bf16 out (x4 B)
    sgd = 4 * (grad + 2 * n + 2 * n) + 2 * n
    norms = 4 * (adapted + (grad - (n - adapted)))             # p and G of the adapted tensors
    return {"elements": n, "folded_elements": folded, "plane_elements": planes,
            "mean_planes": round(planes / max(folded, 1), 2),
            "sgd_momentum_mixed": sgd,
            "lars_store": norms + 4 * folded + 4 * update,
            "lars_resum": norms + 4 * (update - n + grad)}


def timed_steps(tr, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.run(k, use_graph=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / k


def timed_optimizer(tr, kind, reps):
    m = tr.model
    fn = ((lambda: m.lars_step(0.0, tr.momentum, tr.wd, tr.lars_eta)) if kind == "lars"
          else (lambda: m.sgd_step(0.0, tr.momentum, tr.wd)))  # (rate 0: the parameters stay put)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resnet_lars_cost: needs a GPU (nothing here is measured on a CPU)")
    dev = torch.device("cuda:0")
    trs = {k: ResNetTrainer(a.batch, dev, optimizer=k) for k in KINDS}
    for tr in trs.values():
        tr.run(3, use_graph=True)  # eager warm-up, capture, one replay
    ms = {k: [] for k in KINDS}
    for _ in range(a.windows):
        for k in KINDS:
            ms[k].append(timed_steps(trs[k], a.steps))
    us = {k: [] for k in KINDS}
    for _ in range(a.windows):
        for k in KINDS:
            us[k].append(timed_optimizer(trs[k], k, a.reps))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    by = step_bytes(trs["lars"].model)
    bw = by["sgd_momentum_mixed"] / (med(us["momentum"]) * 1e-6)
    print(json.dumps({
        "batch": a.batch, "windows": a.windows, "steps_per_window": a.steps, "reps": a.reps,
        "ms_per_step": {k: [round(v, 3) for v in ms[k]] for k in KINDS},
        "median_ms_per_step": {k: round(med(ms[k]), 3) for k in KINDS},
        "images_per_s": {k: round(a.batch / med(ms[k]) * 1e3, 1) for k in KINDS},
        "optimizer_us": {k: [round(v, 1) for v in us[k]] for k in KINDS},
        "median_optimizer_us": {k: round(med(us[k]), 1) for k in KINDS},
        "bytes": by,
        "sgd_momentum_mixed_TBps": round(bw / 1e12, 3),
        "lars_us_at_that_bandwidth": {"store": round(by["lars_store"] / bw * 1e6, 1),
                                      "resum": round(by["lars_resum"] / bw * 1e6, 1)},
        "loss": {k: round(tr.stats()[0], 4) for k, tr in trs.items()},
    }), flush=True)


if __name__ == "__main__":
    main()
