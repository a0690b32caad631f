"""Cost of one test-set evaluation of the reference MLP: the fused one-launch kernel
(ops/mlp_eval.py, csrc/kernels/mlp_eval.hip) against the path it replaced, timed interleaved
in ONE process at n = 100, 10,000 and 55,000 rows.

The replaced path is kept here as code (it no longer exists in train/): two generic
``nn.gemm`` launches (the first writes the n x 100 hidden matrix), ``argmax``, a compare and a
mean through ATen.  Two figures per path and size:

* ``device``: device time per evaluation, events around back-to-back calls, nothing read back
  (both paths leave their result on the device);
* ``call``: wall time per evaluation as a caller sees it, the result read back to a Python
  float after every call (a device synchronise per call).

Every window is sized to >= ``--window_ms`` of work after one untimed warm-up call per path
and size; the two paths alternate for ``--pairs`` rounds and the medians are reported with
the spread.  Both paths' accuracies are compared first (same rows, same parameters).

    python tools/probes/eval_cost.py [--out profiles/eval] [--pairs 7] [--window_ms 200]

Writes ``eval_cost.json`` and ``README.md`` into ``--out`` and prints the JSON line.
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
from distributedtensorflowexample_amd.ops import mlp_eval, mlp_step, nn  # noqa: E402

SIZES = (100, 10000, 55000)


def parent_device(p, x, y):
    """The replaced evaluation, result left on the device (train/worker.py's form)."""
    W1t, b1, W2t, b2 = mlp_step.unflatten(p)
    h = nn.gemm(x, W1t, trans_b=True, bias=b1, act="sigmoid")
    logits = nn.gemm(h, W2t, trans_b=True, bias=b2)
    return (logits.argmax(1) == y).float().mean()


def new_device(p, x, y):
    return mlp_eval.evaluate(p, x, y)


def device_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def call_us(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e6 / reps


def reps_for(timer, fn, window_ms):
    one = max(timer(fn, 20), 1e-3)
    return max(20, int(window_ms * 1e3 / one))


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "eval"))
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--window_ms", type=float, default=200.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    p = init_params(dev, seed=0)
    rows = []
    for n in SIZES:
        x, y = mnist_like_device(n, seed=100, device=dev)
        y64, y32 = y.long(), y.int()
        paths = {
            "parent": (lambda: parent_device(p, x, y64),
                       lambda: float(parent_device(p, x, y64))),
            "fused": (lambda: new_device(p, x, y32),
                      lambda: new_device(p, x, y32).accuracy),
        }
        acc = {k: float(f[1]()) for k, f in paths.items()}  # warm-up, and the same answer
        if abs(acc["parent"] - acc["fused"]) > 2.0 / n + 1e-6:
            raise SystemExit("the two paths disagree at n=%d: %r" % (n, acc))
        reps = {k: (reps_for(device_us, f[0], a.window_ms), reps_for(call_us, f[1], a.window_ms))
                for k, f in paths.items()}
        t = {k: {"device": [], "call": []} for k in paths}
        for _ in range(a.pairs):
            for k, f in paths.items():  # interleaved: parent, fused, parent, ...
                t[k]["device"].append(device_us(f[0], reps[k][0]))
                t[k]["call"].append(call_us(f[1], reps[k][1]))
        row = {"n": n, "accuracy": acc, "reps": reps}
        for k in paths:
            for m in ("device", "call"):
                v = t[k][m]
                row["%s_%s_us" % (k, m)] = {"median": round(med(v), 2), "min": round(min(v), 2),
                                            "max": round(max(v), 2)}
        row["speedup_device"] = round(med(t["parent"]["device"]) / med(t["fused"]["device"]), 2)
        row["speedup_call"] = round(med(t["parent"]["call"]) / med(t["fused"]["call"]), 2)
        # the kernel's arithmetic: f32 MFMA work with the hidden width padded to 112
        flop = 2.0 * n * 784 * 112 + 2.0 * n * 112 * 16
        row["fused_mfma_tflops"] = round(flop / med(t["fused"]["device"]) / 1e6, 1)
        rows.append(row)
    out = {"probe": "eval_cost", "device": torch.cuda.get_device_name(0), "pairs": a.pairs,
           "window_ms": a.window_ms, "sizes": rows}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "eval_cost.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(readme(out))
    print(json.dumps(out), flush=True)


def readme(out):
    def cell(r, key):
        v = r[key]
        return "%.1f (%.1f-%.1f)" % (v["median"], v["min"], v["max"])

    lines = [
        "# Test-set evaluation: fused kernel against the replaced path",
        "",
        "Written by `tools/probes/eval_cost.py` on %s: both paths in one process, alternating, "
        "%d rounds, every window >= %.0f ms after a warm-up call; median (min-max) in "
        "microseconds per evaluation.  `parent` is the replaced path (two `nn.gemm` launches, "
        "`argmax`, compare, mean through ATen; kept as code in the probe), `fused` is "
        "`ops.mlp_eval.evaluate` (one memset node + one kernel).  `device`: events around "
        "back-to-back calls, nothing read back.  `call`: wall time with the result read back "
        "to a Python float after every call." % (out["device"], out["pairs"], out["window_ms"]),
        "",
        "| n | parent device | fused device | x | parent call | fused call | x | fused f32 MFMA TF/s |",
        "|---|---|---|---|---|---|---|---|",
    ]
    for r in out["sizes"]:
        lines.append("| %d | %s | %s | %.2f | %s | %s | %.2f | %.1f |" % (
            r["n"], cell(r, "parent_device_us"), cell(r, "fused_device_us"), r["speedup_device"],
            cell(r, "parent_call_us"), cell(r, "fused_call_us"), r["speedup_call"],
            r["fused_mfma_tflops"]))
    lines += [
        "",
        "The MFMA rate counts 2 n (784 x 112 + 112 x 16) FLOP (hidden width padded to 112, classes "
        "to 16) over the fused path's device time, memset node included; the f32 MFMA peak is "
        "157 TF/s.  The split's own floor (one wave = 16 rows x 7 hidden tiles = 1372 MFMAs of 32 "
        "cycles) is 18.3 us at 2.4 GHz for any n up to 16,384 rows (one wave per SIMD).",
        "",
        "Raw numbers: `eval_cost.json`.",
        "",
    ]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
