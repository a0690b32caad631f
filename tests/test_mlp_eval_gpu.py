"""Fused MLP evaluation kernel (csrc/kernels/mlp_eval.hip) through ops/mlp_eval.py, the
trainer's ``evaluate()`` and the mirrored loop's ``--eval_summaries``.

Sizes: 1, 15, 16, 17 (one 16-row wave tile and its edges), 63, 64, 65 (the 64-row workgroup
tile T, read from the module, and its edges), 2 T + 3 (three workgroups with a tail), 200,
1000.  Two parameter sets: ``init_params`` as it is (saturated hidden units, large logits)
and the same with W1 scaled by 0.05 and N(0, 0.5) biases (unsaturated: a wrong bias or
sigmoid shows).

Tolerances, the project's own: predictions equal the float64 arg-max on every row whose
float64 top-2 gap exceeds 1e-3 (tests/test_mlp_rowmajor_gpu.py); mean loss within
1e-4 * max(1, |ref|) (tests/test_shuffle_gpu.py); probabilities within 1e-4 absolute.
Rows under the gap may be left out of the prediction comparison: at most 0.1 % of the rows,
none for n <= 1000, asserted on the reference alone before the GPU result is looked at.
The float64 reference of each parameter set is computed once and shared."""
import functools
import glob
import types

import numpy as np
import pytest
import torch

from distributedtensorflowexample_amd.models.mlp import init_params
from distributedtensorflowexample_amd.ops import mlp_eval, mlp_step

pytestmark = pytest.mark.gpu

GAP = 1e-3
NMAX = 1000


def _tile():
    from distributedtensorflowexample_amd.ops._ext import hip

    return int(hip().mlp_eval_row_tile())


def _sizes():
    try:
        T = _tile()
    except RuntimeError:  # (collection without the built module: the tests then fail loudly)
        T = 64
    return sorted({1, 15, 16, 17, 63, 64, 65, 200, 1000, T - 1, T, T + 1, 2 * T + 3})


def _params(kind, seed=0):
    p = init_params("cpu", seed=seed)
    if kind == "scaled":
        W1t, b1, W2t, b2 = mlp_step.unflatten(p)
        W1t.mul_(0.05)
        g = torch.Generator().manual_seed(1000 + seed)
        b1.copy_(torch.randn(b1.shape, generator=g) * 0.5)
        b2.copy_(torch.randn(b2.shape, generator=g) * 0.5)
    return p


def forward64(p, x):
    """numpy float64: logits, probabilities, lowest-index arg-max, top-2 gap, log-sum-exp."""
    p = p.double().numpy()
    x = x.double().numpy()
    W1t, b1 = p[:78400].reshape(100, 784), p[78400:78500]
    W2t, b2 = p[78500:79500].reshape(10, 100), p[79500:]
    h = 1.0 / (1.0 + np.exp(-(x @ W1t.T + b1)))
    logits = h @ W2t.T + b2
    m = logits.max(1, keepdims=True)
    e = np.exp(logits - m)
    s = np.sort(logits, 1)
    return dict(logits=logits, probs=e / e.sum(1, keepdims=True),
                pred=(logits == m).argmax(1), gap=s[:, -1] - s[:, -2],
                lse=m[:, 0] + np.log(e.sum(1)))


def counts64(ref, labels, n=None):
    """Mean loss, count, correct and confusion [label][predicted] of the first n rows."""
    lab = np.asarray(labels, np.int64)[:n]
    keep = (lab >= 0) & (lab < 10)
    idx = np.flatnonzero(keep)
    rows = ref["lse"][idx] - ref["logits"][idx, lab[idx]]
    conf = np.zeros((10, 10), np.int64)
    np.add.at(conf, (lab[idx], ref["pred"][idx]), 1)
    return dict(loss=float(rows.mean()) if len(idx) else float("nan"), count=len(idx),
                correct=int((ref["pred"][idx] == lab[idx]).sum()), conf=conf)


@functools.lru_cache(maxsize=None)
def _uniform_case(kind):
    """(params, x [NMAX, 784], labels, float64 forward) of one parameter set: computed once."""
    p = _params(kind)
    g = torch.Generator().manual_seed(11)
    x = torch.rand(NMAX, 784, generator=g)
    y = torch.randint(0, 10, (NMAX,), generator=g).int()
    return p, x, y, forward64(p, x)


@functools.lru_cache(maxsize=None)
def _device_case(kind):
    p, x, y, ref = _uniform_case(kind)
    return p.cuda(), x.cuda(), y.cuda()


def _loss_ok(got, ref):
    return abs(got - ref) <= 1e-4 * max(1.0, abs(ref))


# -- 1. against float64 ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["raw", "scaled"])
@pytest.mark.parametrize("n", _sizes())
def test_against_float64(gpu, kind, n):
    p, x, y, ref = _uniform_case(kind)
    amb = int((ref["gap"][:n] <= GAP).sum())
    assert amb == 0, "ambiguous reference rows at n <= 1000"
    exp = counts64(ref, y.numpy(), n)
    pd, xd, yd = _device_case(kind)
    res = mlp_eval.evaluate(pd, xd[:n], yd[:n], predictions=True, probs=True)
    pred, probs = res.pred.cpu().numpy(), res.probs.cpu().numpy()
    print("n", n, kind, "loss", res.loss, "ref", exp["loss"], "correct", res.correct,
          exp["correct"], "max prob err", np.abs(probs - ref["probs"][:n]).max())
    assert pred.shape == (n,) and probs.shape == (n, 10)
    assert np.array_equal(pred, ref["pred"][:n])
    assert np.abs(probs - ref["probs"][:n]).max() <= 1e-4
    assert res.count == n and int(res.confusion.sum()) == n
    assert _loss_ok(res.loss, exp["loss"])
    assert res.correct == exp["correct"]
    # (at most two cells per ambiguous row; there is none)
    assert int(np.abs(res.confusion.numpy() - exp["conf"]).sum()) <= 2 * amb
    assert res.accuracy == exp["correct"] / n


# -- 2. placement, exact in integers --------------------------------------------------------
def test_placement_exact(gpu):
    n = 2 * 784 + 13
    i = torch.arange(n)
    x = torch.zeros(n, 784)
    x[i, i % 784] = 1.0
    p = torch.zeros(mlp_step.NPARAM)
    W1t, b1, W2t, b2 = mlp_step.unflatten(p)
    f, j = torch.arange(784), torch.arange(100)
    W1t.copy_(torch.where(j[:, None] == (f % 100)[None, :], 30.0, -30.0))
    W2t.copy_(torch.where(torch.arange(10)[:, None] == (j % 10)[None, :], 10.0, 0.0))
    y = (i % 10).int()
    want = ((i % 784) % 100) % 10
    conf = np.zeros((10, 10), np.int64)
    np.add.at(conf, (y.numpy().astype(np.int64), want.numpy()), 1)
    res = mlp_eval.evaluate(p.cuda(), x.cuda(), y.cuda(), predictions=True)
    assert np.array_equal(res.pred.cpu().numpy(), want.numpy())
    assert res.count == n
    assert res.correct == int((want == y).sum())
    assert np.array_equal(res.confusion.numpy(), conf)


# -- 3. masking and predict-only -------------------------------------------------------------
def test_masking_and_predict_only(gpu):
    n = 200
    p, x, y, ref = _uniform_case("scaled")
    pd, xd, yd = _device_case("scaled")
    full = mlp_eval.evaluate(pd, xd[:n], yd[:n], predictions=True, probs=True)
    ym = y[:n].clone()
    masked = [0, 15, 16, 63, 64, 130, n - 1]
    ym[masked] = -1
    ym[77] = 10  # out of range on the other side
    exp = counts64(ref, ym.numpy(), n)
    res = mlp_eval.evaluate(pd, xd[:n], ym.cuda(), predictions=True, probs=True)
    assert torch.equal(res.pred, full.pred) and torch.equal(res.probs, full.probs)
    assert res.count == n - len(masked) - 1 == exp["count"]
    assert res.correct == exp["correct"]
    assert np.array_equal(res.confusion.numpy(), exp["conf"])
    assert _loss_ok(res.loss, exp["loss"])
    # every row masked: nothing is counted
    none = mlp_eval.evaluate(pd, xd[:n], torch.full((n,), -1, dtype=torch.int32, device=gpu))
    assert none.count == 0 and none.correct == 0 and int(none.confusion.sum()) == 0
    assert none.loss_sum == 0.0
    # predict only: the same classes, and a caller's accumulator is left alone
    sentinel = torch.full((mlp_eval.ACC_WORDS,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
    only = mlp_eval.evaluate(pd, xd[:n], None, acc=sentinel, predictions=True, probs=True)
    assert only.acc is None and torch.equal(only.pred, full.pred)
    assert torch.equal(only.probs, full.probs)
    assert torch.equal(mlp_eval.predict(pd, xd[:n]), full.pred)
    torch.cuda.synchronize()
    assert int((sentinel != 0x5A5A5A5A).sum()) == 0


# -- 4. reproducibility and graph capture ------------------------------------------------------
def test_bitwise_reproducible_and_capturable(gpu):
    n = 1000
    pd, xd, yd = _device_case("raw")
    a = mlp_eval.evaluate(pd, xd[:n], yd[:n])
    b = mlp_eval.evaluate(pd, xd[:n], yd[:n])
    assert torch.equal(a.acc, b.acc)
    acc = mlp_eval.new_acc(gpu)
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            mlp_eval.evaluate(pd, xd[:n], yd[:n], acc=acc)
    torch.cuda.current_stream(gpu).wait_stream(s)
    for _ in range(3):  # the zeroing node travels with the graph: no replay adds to the last
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(acc, a.acc)


# -- 5. input checks -------------------------------------------------------------------------
def test_input_checks(gpu):
    pd, xd, yd = _device_case("raw")
    n = 32
    x, y = xd[:n], yd[:n]
    before = mlp_eval.new_acc(gpu)
    with pytest.raises(ValueError):
        mlp_eval.evaluate(pd, xd[:2 * n:2], y, acc=before)              # not contiguous
    flat = torch.zeros(n * 784 + 1, device=gpu)
    with pytest.raises(ValueError):
        mlp_eval.evaluate(pd, flat[1:].view(n, 784), y, acc=before)     # misaligned
    with pytest.raises(ValueError):
        mlp_eval.evaluate(pd, x, y.long(), acc=before)                  # int64 labels
    with pytest.raises(ValueError):
        mlp_eval.evaluate(pd, x, yd[:n - 1], acc=before)                # wrong label count
    with pytest.raises(ValueError):
        mlp_eval.evaluate(pd.cpu(), x, y, acc=before)                   # parameters elsewhere
    torch.cuda.synchronize()
    assert int((before != 0).sum()) == 0                                # nothing was launched


# -- 6. real data -----------------------------------------------------------------------------
def test_mnist_test_set(gpu):
    from distributedtensorflowexample_amd.data.mnist import read_test_set

    test = read_test_set()
    x = torch.from_numpy(np.ascontiguousarray(test.images, np.float32))
    y = np.asarray(test.labels).astype(np.int32)
    p = init_params("cpu", seed=0)
    ref = forward64(p, x)
    amb = int((ref["gap"] <= GAP).sum())
    assert amb <= 10  # (0.1 % of 10,000 rows: the cap, on the reference alone)
    exp = counts64(ref, y)
    res = mlp_eval.evaluate(p.cuda(), x.cuda(), torch.from_numpy(y).cuda(), predictions=True)
    pred = res.pred.cpu().numpy()
    print("mnist: correct", res.correct, "ref", exp["correct"], "ambiguous", amb, "loss",
          res.loss, "ref", exp["loss"])
    assert res.count == 10000 and int(res.confusion.sum()) == 10000
    clear = ref["gap"] > GAP
    assert np.array_equal(pred[clear], ref["pred"][clear])
    assert abs(res.correct - exp["correct"]) <= amb
    assert int(np.abs(res.confusion.numpy() - exp["conf"]).sum()) <= 2 * amb
    assert _loss_ok(res.loss, exp["loss"])


# -- 7. trainer ------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "three-launch"])
def test_trainer_evaluate(gpu, pipeline):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    B, lr = 16, 0.05
    n = 5 * B + 7
    g = torch.Generator().manual_seed(5)
    x = torch.rand(n, 784, generator=g)
    y = torch.randint(0, 10, (n,), generator=g).int()
    xe = torch.rand(70, 784, generator=g)
    ye = torch.randint(0, 10, (70,), generator=g).int()
    p0 = _params("scaled", seed=3)
    tr = FusedMLPTrainer(p0.cuda(), x.cuda(), y.cuda(), batch_size=B, learning_rate=lr,
                         pipeline=pipeline)
    # float64 SGD over reference_step: per-step losses and the parameters after 3 steps
    p = p0.double()
    losses, p3 = [], None
    for s in range(7):
        k = s % 5
        gr, loss, _ = mlp_step.reference_step(p, x[k * B:(k + 1) * B].double(),
                                              y[k * B:(k + 1) * B])
        p = p - lr * gr
        losses.append(float(loss))
        if s == 2:
            p3 = p.clone()
    tr.run(3, use_graph=False)
    assert tr.pending == pipeline  # (the pipelined step leaves its last update pending)
    xed, yed = xe.cuda(), ye.cuda()
    res = tr.evaluate(xed, yed, predictions=True)
    assert tr.global_step() == 3
    again = mlp_eval.evaluate(tr.snapshot(), xed, yed, predictions=True)
    assert torch.equal(res.acc, again.acc) and torch.equal(res.pred, again.pred)
    assert tr.global_step() == 3
    # the parameters evaluated are those after all 3 steps (the pending update included)
    exp = counts64(forward64(p3.float(), xe), ye.numpy())
    assert res.count == 70 and _loss_ok(res.loss, exp["loss"])
    tr.run(4, use_graph=False)
    got = tr.stats_range(0, 7)[:, 0].tolist()
    assert tr.global_step() == 7
    for a, b in zip(got, losses):
        assert _loss_ok(a, b), (got, losses)


# -- 8. the mirrored loop -----------------------------------------------------------------------
def test_mirrored_loop_eval_summaries(gpu, tmp_path, monkeypatch):
    from distributedtensorflowexample_amd.data.mnist import DataSet, DataSets
    from distributedtensorflowexample_amd.train.mirrored_mlp import train_mirrored
    from distributedtensorflowexample_amd.utils.summary import read_events

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    B, steps = 16, 10
    n = 5 * B + 7
    g = torch.Generator().manual_seed(3)
    x = torch.rand(n, 784, generator=g).numpy()
    y = torch.randint(0, 10, (n,), generator=g).numpy().astype(np.uint8)
    test = DataSet(x[:40], y[:40], one_hot=False)
    ds = DataSets(train=DataSet(x, y, one_hot=False), validation=test, test=test,
                  synthetic_train=True)

    def run(tag, **kw):
        fl = types.SimpleNamespace(batch_size=B, learning_rate=0.05, training_steps=steps,
                                   logdir=str(tmp_path / tag), log_every=5, eval_every=5,
                                   save_model_secs=1000.0, save_summaries_secs=1000.0,
                                   use_locking=False, seed=0, device="cuda", **kw)
        logs = []
        _, params = train_mirrored(fl, ds, log=logs.append)
        scalars = {}
        for path in glob.glob(fl.logdir + "_0/*tfevents*"):
            for ev in read_events(path):
                for tag_, v in (ev.get("scalars") or {}).items():
                    scalars.setdefault(tag_, {})[int(ev["step"])] = float(v)
        return logs, scalars, params

    logs, scalars, params = run("on", eval_summaries=True)
    accs = [float(l.split(": ")[1]) for l in logs if l.startswith("test accuracy: ")]
    assert len(accs) == 2
    assert sorted(scalars["test_loss"]) == [5, 10] and sorted(scalars["test_accuracy"]) == [5, 10]
    assert [scalars["test_accuracy"][s] for s in (5, 10)] == pytest.approx(accs, abs=1e-6)
    # the last evaluation is of the returned parameters
    exp = counts64(forward64(params.cpu(), torch.from_numpy(x[:40])), y[:40])
    assert _loss_ok(scalars["test_loss"][10], exp["loss"])
    assert "loss" in scalars and "accuracy" in scalars
    logs, scalars, _ = run("off")
    assert len([l for l in logs if l.startswith("test accuracy: ")]) == 2
    assert "test_loss" not in scalars and "test_accuracy" not in scalars
    assert "loss" in scalars
