"""CPU tier of the fused MLP evaluation: the CPU path of ops/mlp_eval.py against a numpy
float64 computation written out here (masked labels, the lowest-index tie rule on exact ties,
the confusion matrix), and ``main.py --job_name eval --device cpu`` on a checkpoint written
from known parameters.

Tolerances (the project's own): predictions on every row whose float64 top-2 gap exceeds
1e-3 (tests/test_mlp_rowmajor_gpu.py), mean loss within 1e-4 * max(1, |ref|)
(tests/test_shuffle_gpu.py), probabilities within 1e-4 absolute."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributedtensorflowexample_amd.data.mnist import read_test_set
from distributedtensorflowexample_amd.models.mlp import init_params
from distributedtensorflowexample_amd.ops import mlp_eval, mlp_step
from distributedtensorflowexample_amd.train.saver import FastSaver
from distributedtensorflowexample_amd.train.worker import flat_to_tf_vars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 1e-3


def scaled_params(seed):
    """init_params with W1 scaled by 0.05 and N(0, 0.5) biases: unsaturated hidden units."""
    p = init_params("cpu", seed=seed)
    W1t, b1, W2t, b2 = mlp_step.unflatten(p)
    W1t.mul_(0.05)
    g = torch.Generator().manual_seed(1000 + seed)
    b1.copy_(torch.randn(b1.shape, generator=g) * 0.5)
    b2.copy_(torch.randn(b2.shape, generator=g) * 0.5)
    return p


def ref64(p, x, labels=None):
    """numpy float64: (logits, probs, pred with the lowest-index rule, top-2 gap, and with
    labels: mean loss over the counted rows, count, correct, confusion [label][predicted])."""
    p = p.double().numpy()
    x = x.double().numpy()
    W1t = p[:78400].reshape(100, 784)
    b1 = p[78400:78500]
    W2t = p[78500:79500].reshape(10, 100)
    b2 = p[79500:]
    h = 1.0 / (1.0 + np.exp(-(x @ W1t.T + b1)))
    logits = h @ W2t.T + b2
    m = logits.max(1, keepdims=True)
    e = np.exp(logits - m)
    probs = e / e.sum(1, keepdims=True)
    pred = np.array([int(np.flatnonzero(r == r.max())[0]) for r in logits])
    s = np.sort(logits, 1)
    gap = s[:, -1] - s[:, -2]
    out = dict(logits=logits, probs=probs, pred=pred, gap=gap)
    if labels is not None:
        lab = labels.numpy().astype(np.int64)
        keep = (lab >= 0) & (lab < 10)
        lse = m[:, 0] + np.log(e.sum(1))
        rows = lse[keep] - logits[keep, lab[keep]]
        conf = np.zeros((10, 10), np.int64)
        np.add.at(conf, (lab[keep], pred[keep]), 1)
        out.update(loss=float(rows.mean()) if keep.any() else float("nan"),
                   count=int(keep.sum()), correct=int((pred[keep] == lab[keep]).sum()), conf=conf)
    return out


def test_cpu_path_matches_float64():
    p = scaled_params(1)
    g = torch.Generator().manual_seed(7)
    n = 203
    x = torch.rand(n, 784, generator=g)
    y = torch.randint(0, 10, (n,), generator=g).int()
    y[[0, 5, 64, n - 1]] = -1   # masked
    y[[9, 100]] = 10            # out of range: masked too
    ref = ref64(p, x, y)
    assert int((ref["gap"] <= GAP).sum()) == 0   # (the reference alone: no ambiguous row)
    res = mlp_eval.evaluate(p, x, y, predictions=True, probs=True)
    assert res.pred.dtype == torch.int32 and tuple(res.pred.shape) == (n,)
    assert np.array_equal(res.pred.numpy(), ref["pred"])   # masked rows included
    assert np.abs(res.probs.numpy() - ref["probs"]).max() <= 1e-4
    assert res.count == ref["count"] == n - 6
    assert res.correct == ref["correct"]
    assert abs(res.loss - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"]))
    assert res.accuracy == ref["correct"] / ref["count"]
    assert np.array_equal(res.confusion.numpy(), ref["conf"])
    assert int(res.confusion.sum()) == res.count
    # predict(): the same classes, no accumulator
    assert np.array_equal(mlp_eval.predict(p, x).numpy(), ref["pred"])
    only = mlp_eval.evaluate(p, x)
    assert only.acc is None and np.array_equal(only.pred.numpy(), ref["pred"])
    with pytest.raises(ValueError):
        only.loss
    # a caller's accumulator is reused (and re-zeroed) with labels, untouched without
    acc = torch.full((mlp_eval.ACC_WORDS,), 77, dtype=torch.int32)
    mlp_eval.evaluate(p, x, None, acc=acc)
    assert int((acc != 77).sum()) == 0
    again = mlp_eval.evaluate(p, x, y, acc=acc)
    assert again.acc is acc and torch.equal(acc, res.acc)


def test_lowest_index_on_exact_ties():
    x = torch.rand(5, 784, generator=torch.Generator().manual_seed(3))
    y = torch.tensor([3, 7, 0, 3, 9], dtype=torch.int32)
    # all-zero parameters: ten equal logits -> class 0
    p = torch.zeros(mlp_step.NPARAM)
    res = mlp_eval.evaluate(p, x, y, predictions=True)
    assert res.pred.tolist() == [0] * 5 and res.correct == 1
    assert abs(res.loss - float(np.log(10.0))) <= 1e-4 * max(1.0, float(np.log(10.0)))
    # classes 3 and 7 share one weight row (the same f32 sums: an exact tie) above the rest
    W1t, b1, W2t, b2 = mlp_step.unflatten(p)
    W2t[3].fill_(0.25)
    W2t[7].fill_(0.25)
    res = mlp_eval.evaluate(p, x, y, predictions=True, probs=True)
    assert torch.equal(res.probs[:, 3], res.probs[:, 7])
    assert res.pred.tolist() == [3] * 5 and res.correct == 2
    conf = np.zeros((10, 10), np.int64)
    for lab in y.tolist():
        conf[lab, 3] += 1
    assert np.array_equal(res.confusion.numpy(), conf)


def test_input_checks_cpu():
    p = init_params("cpu", seed=0)
    x = torch.rand(8, 784)
    y = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(ValueError):
        mlp_eval.evaluate(p, x.t().contiguous().t(), y)          # not contiguous
    with pytest.raises(ValueError):
        mlp_eval.evaluate(p, x, y.long())                        # int64 labels
    with pytest.raises(ValueError):
        mlp_eval.evaluate(p, x, y[:7])                           # wrong label count
    with pytest.raises(ValueError):
        mlp_eval.evaluate(p[:-1], x, y)                          # not the flat buffer
    with pytest.raises(ValueError):
        mlp_eval.evaluate(p, x.double(), y)


# -- the eval job ---------------------------------------------------------------------------
def _run_eval(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--job_name", "eval",
                           "--device", "cpu"] + args, cwd=ROOT, capture_output=True, text=True,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="4"),
                          timeout=300)


def _save(logdir, tf_vars, step):
    v = {k: t.contiguous() for k, t in tf_vars.items()}
    v["global/global_step"] = torch.tensor(step, dtype=torch.int32)
    FastSaver({k: None for k in v}).save(None, os.path.join(logdir, "model.ckpt"),
                                          global_step=step, variables=v)


def test_eval_job_cpu(tmp_path):
    p = scaled_params(2)
    logdir = str(tmp_path / "run")
    _save(logdir, flat_to_tf_vars(p), 1234)
    out = str(tmp_path / "pred.npy")
    r = _run_eval(["--logdir", logdir, "--eval_output", out])
    assert r.returncode == 0, r.stdout + r.stderr

    test = read_test_set()
    x = torch.from_numpy(np.ascontiguousarray(test.images, np.float32))
    y = torch.from_numpy(np.asarray(test.labels).astype(np.int32))
    ref = ref64(p, x, y)
    amb = int((ref["gap"] <= GAP).sum())
    assert amb <= 10                               # (0.1 % of the rows; the reference alone)
    here = mlp_eval.evaluate(p, x, y, predictions=True)

    assert re.search(r"^global_step: 1234$", r.stdout, re.M), r.stdout
    acc = float(re.search(r"^test accuracy: (\S+)$", r.stdout, re.M).group(1))
    loss = float(re.search(r"^test loss: (\S+)$", r.stdout, re.M).group(1))
    assert acc == here.accuracy                    # the same op on the same data
    assert abs(acc * 10000 - ref["correct"]) <= amb
    assert abs(loss - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"]))
    lines = r.stdout.splitlines()
    k = next(i for i, l in enumerate(lines) if l.startswith("confusion matrix"))
    conf = np.array([[int(v) for v in l.split()] for l in lines[k + 1:k + 11]])
    assert conf.shape == (10, 10) and np.array_equal(conf, here.confusion.numpy())
    assert int(conf.sum()) == 10000
    pred = np.load(out)
    assert pred.dtype == np.int32 and pred.shape == (10000,)
    assert np.array_equal(pred, here.pred.numpy())
    clear = ref["gap"] > GAP
    assert np.array_equal(pred[clear], ref["pred"][clear])


def test_eval_job_refuses_missing_and_foreign_checkpoints(tmp_path):
    empty = tmp_path / "empty"
    empty.mkdir()
    r = _run_eval(["--logdir", str(empty)])
    assert r.returncode != 0
    assert "no checkpoint" in (r.stdout + r.stderr)
    # a 784-50-10 model: refused, naming the variable
    other = str(tmp_path / "other")
    _save(other, {"global/dense/kernel": torch.zeros(784, 50), "global/dense/bias": torch.zeros(50),
                  "global/dense_1/kernel": torch.zeros(50, 10),
                  "global/dense_1/bias": torch.zeros(10)}, 5)
    r = _run_eval(["--logdir", other])
    assert r.returncode != 0
    assert "global/dense/kernel" in (r.stdout + r.stderr)
