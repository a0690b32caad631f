"""Hidden activations of the MNIST MLP (``ops/hidden_act.py``: sigmoid, relu, tanh) on the CPU:
``activation_reference`` against torch autograd in float64, the CPU paths that gained
``activation=`` (``MnistMLP``, ``ops.mlp_eval.evaluate``, ``reference_forward`` /
``reference_step``), the mirrored CPU loop, the eval job, ``main.py``'s validation, unchanged
defaults, and the float64 figures the GPU tests rely on."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import activation_reference as ar
import dropout_reference as dr
from distributedtensorflowexample_amd import flags as F
from distributedtensorflowexample_amd.ops import hidden_act, mlp_eval, mlp_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = ar.ACTS


# ---- the definition ------------------------------------------------------------------------------
def test_names_ids_and_check():
    assert hidden_act.NAMES == ("sigmoid", "relu", "tanh") == ACTS
    assert [hidden_act.act_id(n) for n in ACTS] == [0, 1, 2]
    assert hidden_act.check(None) == "sigmoid" == hidden_act.DEFAULT
    for bad in ("gelu", "", "ReLU", 1, "none"):
        with pytest.raises(ValueError, match="unknown hidden activation"):
            hidden_act.check(bad)


def _torch_act(z, act):
    return {"sigmoid": torch.sigmoid, "relu": torch.relu, "tanh": torch.tanh}[act](z)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("B, rate", [(1, 0.0), (17, 0.5), (100, 0.0), (100, 0.1)])
def test_reference_is_torch_autograd_in_float64(B, rate, act):
    """The forward and every gradient of ``activation_reference.step`` against autograd of the
    same network written with torch's own activations: 1e-12."""
    p, x, y = dr.data(B)
    keep = scale = None
    if rate:
        keep, (_, scale) = dr.keep_mask(dr.SEED, 2, 0, B, rate), dr.threshold(rate)
    ref = ar.step(p, x[:B], y[:B], act, keep, scale or 1.0)
    q = p.double().clone().requires_grad_(True)
    W1t, b1, W2t, b2 = mlp_step.unflatten(q)
    h = _torch_act(x[:B].double() @ W1t.t() + b1, act)
    h.retain_grad()
    hd = h if keep is None else h * (keep.double() * scale)
    logits = hd @ W2t.t() + b2
    logits.retain_grad()
    loss = torch.nn.functional.cross_entropy(logits, y[:B].long())
    loss.backward()
    assert float((ref["h"] - h.detach()).abs().max()) <= 1e-12
    assert float((ref["logits"] - logits.detach()).abs().max()) <= 1e-12
    assert abs(float(ref["loss"]) - float(loss.detach())) <= 1e-12
    assert float((ref["dl"] - logits.grad).abs().max()) <= 1e-12
    assert float((ref["grad"] - q.grad).abs().max()) <= 1e-12
    # (hidden_act's own float64 definition is the same function)
    assert torch.equal(hidden_act.forward(ref["z1"], act), ref["h"])
    assert torch.equal(hidden_act.derivative(ref["h"], act), ar.act_derivative(ref["h"], act))


def test_relu_at_zero():
    z = torch.tensor([-1.0, -0.0, 0.0, 1e-300, 2.0], dtype=torch.float64)
    for fwd, der in ((ar.act_forward, ar.act_derivative),
                     (hidden_act.forward, hidden_act.derivative)):
        h = fwd(z, "relu")
        assert h.tolist() == [0.0, 0.0, 0.0, 1e-300, 2.0]
        assert not bool(torch.signbit(h).any())  # z = -0 gives h = +0
        assert der(h, "relu").tolist() == [0.0, 0.0, 0.0, 1.0, 1.0]  # 0 at exactly 0
    q = z.clone().requires_grad_(True)
    torch.relu(q).sum().backward()
    assert q.grad.tolist() == [0.0, 0.0, 0.0, 1.0, 1.0]


# ---- the CPU paths -------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("B", [1, 17, 100])
def test_reference_step_and_forward_take_the_activation(B, act):
    p, x, y = dr.data(B)
    ref = ar.step(p, x[:B], y[:B], act)
    h, logits = mlp_step.reference_forward(p.double(), x[:B].double(), activation=act)
    assert float((h - ref["h"]).abs().max()) <= 1e-12
    assert float((logits - ref["logits"]).abs().max()) <= 1e-12
    g, loss, acc = mlp_step.reference_step(p.double(), x[:B].double(), y[:B], activation=act)
    assert float((g - ref["grad"]).abs().max()) <= 1e-12
    assert abs(float(loss) - float(ref["loss"])) <= 1e-12
    assert float(acc) == float(ref["correct"].double().mean())


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("B, rate", [(17, 0.0), (100, 0.5)])
def test_mnist_mlp_takes_the_activation(B, rate, act):
    from distributedtensorflowexample_amd.models.mlp import MnistMLP

    p, x, y = dr.data(B)
    kw, keep, scale = {}, None, 1.0
    if rate:
        keep, (_, scale) = dr.keep_mask(dr.SEED, 4, 0, B, rate), dr.threshold(rate)
        kw = dict(keep=keep, scale=scale)
    ref = ar.step(p, x[:B], y[:B], act, keep, scale)
    model = MnistMLP(flat=p.double().clone(), activation=act)
    loss, acc = model.loss(x[:B].double(), y[:B], **kw)
    loss.backward()
    assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-12
    assert float(acc.detach()) == float(ref["correct"].float().mean())
    assert float((model.flat.grad - ref["grad"]).abs().max()) <= 1e-12
    probs, logits = model.forward(x[:B].double())
    assert float((logits.detach() - ar.forward(p, x[:B], act)[3]).abs().max()) <= 1e-12
    with pytest.raises(ValueError, match="unknown hidden activation"):
        MnistMLP(flat=p.clone(), activation="gelu")


@pytest.mark.parametrize("act", ACTS)
def test_evaluate_cpu_takes_the_activation(act):
    """The CPU path of ``ops.mlp_eval.evaluate`` in f32 against float64: the suite's evaluation
    bounds (mean loss 1e-4 max(1, |ref|), probabilities 1e-4, predictions on rows whose float64
    top-2 gap exceeds 1e-3)."""
    n = 200
    p, x, y = dr.data(100)
    x, y = x[:n].contiguous(), y[:n].contiguous()
    ref = ar.step(p, x, y, act)
    res = mlp_eval.evaluate(p, x, y, predictions=True, probs=True, activation=act)
    clear = ref["gap"] > 1e-3
    assert int((~clear).sum()) <= 2
    assert res.count == n
    assert abs(res.loss - float(ref["loss"])) <= 1e-4 * max(1.0, abs(float(ref["loss"])))
    assert float((res.probs.double() - ref["prob"]).abs().max()) <= 1e-4
    assert torch.equal(res.pred.long()[clear], ref["logits"].argmax(1)[clear])
    assert abs(res.correct - int(ref["correct"].sum())) <= int((~clear).sum())
    if act != "sigmoid":  # (another model than the sigmoid one on the same parameters)
        sig = mlp_eval.evaluate(p, x, y)
        assert abs(sig.loss - res.loss) > 1e-3
    with pytest.raises(ValueError, match="unknown hidden activation"):
        mlp_eval.evaluate(p, x, y, activation="gelu")


# ---- defaults unchanged --------------------------------------------------------------------------
def test_defaults_are_the_sigmoid_functions():
    """Every function that gained the argument gives the same bits without it and with
    ``"sigmoid"``, in f32 and in float64."""
    from distributedtensorflowexample_amd.models.mlp import MnistMLP

    B = 17
    p, x, y = dr.data(B)
    x, y = x[:B].contiguous(), y[:B].contiguous()
    for dt in (torch.float32, torch.float64):
        a = mlp_step.reference_forward(p.to(dt), x.to(dt))
        b = mlp_step.reference_forward(p.to(dt), x.to(dt), "sigmoid")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(a[0], torch.sigmoid(x.to(dt) @ mlp_step.unflatten(p.to(dt))[0].t()))
        a = mlp_step.reference_step(p.to(dt), x.to(dt), y)
        b = mlp_step.reference_step(p.to(dt), x.to(dt), y, activation="sigmoid")
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    a = mlp_eval.evaluate(p, x, y, predictions=True, probs=True)
    b = mlp_eval.evaluate(p, x, y, predictions=True, probs=True, activation="sigmoid")
    assert torch.equal(a.acc, b.acc) and torch.equal(a.pred, b.pred)
    assert torch.equal(a.probs, b.probs)
    la = MnistMLP(flat=p.clone()).loss(x, y)
    lb = MnistMLP(flat=p.clone(), activation="sigmoid").loss(x, y)
    assert torch.equal(la[0].detach(), lb[0].detach()) and torch.equal(la[1], lb[1])
    assert MnistMLP(flat=p.clone()).activation == "sigmoid"


# ---- flags and refusals --------------------------------------------------------------------------
def test_flags_default_and_values():
    fv = F.FlagValues()
    F.define_reference_flags(fv)
    fv(["main.py"])
    assert fv.activation == "sigmoid"
    fv.reset()
    fv(["main.py", "--activation", "tanh"])
    assert fv.activation == "tanh"
    assert hidden_act.from_flags(fv) == "tanh"
    assert hidden_act.from_flags(types.SimpleNamespace()) == "sigmoid"  # (a namespace without it)
    with pytest.raises(ValueError, match="--activation: unknown hidden activation"):
        hidden_act.from_flags(types.SimpleNamespace(activation="gelu"))
    with pytest.raises(ValueError, match="--activation tanh: the worker has no tanh variant"):
        hidden_act.from_flags(fv, allowed=("sigmoid", "relu"), what="the worker")
    hidden_act.refuse(types.SimpleNamespace(activation="sigmoid"), "--model bert")
    with pytest.raises(ValueError, match="--activation relu: --model bert has no relu variant"):
        hidden_act.refuse(types.SimpleNamespace(activation="relu"), "--model bert")


def _wflags(**kw):
    d = dict(batch_size=100, learning_rate=0.05, training_steps=10, logdir="unused",
             use_locking=False, seed=0, ps_device="cpu", num_workers=1, sync_replicas=False,
             optimizer="sgd")
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_ps_async_worker_refuses_tanh(tmp_path, monkeypatch):
    from distributedtensorflowexample_amd.train.worker import Worker

    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="--activation tanh: --strategy ps_async"):
        Worker("worker", 0, None, _wflags(activation="tanh"), device="cpu")
    assert os.listdir(str(tmp_path)) == []


def test_bert_and_resnet_refuse(tmp_path, monkeypatch):
    from distributedtensorflowexample_amd.train.mirrored_models import train_model_mirrored

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    for model in ("bert", "resnet50"):
        with pytest.raises(ValueError, match="--activation relu: --model %s" % model):
            train_model_mirrored(_wflags(model=model, device="cpu", activation="relu",
                                         logdir=str(tmp_path / "m")))
    assert os.listdir(str(tmp_path)) == []


def test_main_validates_the_flag_once(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="4")
    no = str(tmp_path / "no")

    def main(args):
        return subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, env=env,
                              cwd=ROOT, capture_output=True, text=True, timeout=240)

    r = main(["--strategy", "ps_async", "--job_name", "worker", "--activation", "tanh",
              "--logdir", no])
    assert r.returncode != 0 and "--activation tanh: --strategy ps_async" in r.stderr, r.stderr
    for model in ("bert", "resnet50"):
        r = main(["--strategy", "mirrored", "--model", model, "--activation", "relu", "--device",
                  "cpu", "--logdir", no])
        assert r.returncode != 0 and "--activation relu: --model %s" % model in r.stderr, r.stderr
    for job in (["--strategy", "mirrored", "--device", "cpu"], ["--job_name", "eval"],
                ["--strategy", "ps_async", "--job_name", "worker"]):
        r = main(job + ["--activation", "gelu", "--logdir", no])
        assert r.returncode != 0 and "unknown hidden activation 'gelu'" in r.stderr, r.stderr
    assert not os.path.exists(no)
    # the eval job accepts the three names: it fails on the missing checkpoint, not on the flag
    r = main(["--job_name", "eval", "--activation", "tanh", "--device", "cpu", "--logdir",
              str(tmp_path / "empty")])
    assert r.returncode != 0 and "no checkpoint" in r.stderr and "--activation" not in r.stderr


def test_trainer_refuses_before_touching_anything():
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = torch.zeros(mlp_step.NPARAM), torch.zeros(300, 784), torch.zeros(300).int()
    for act in ("relu", "tanh"):
        with pytest.raises(ValueError, match="activation %s: the exchange engines" % act):
            FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, fused_comm=object(), activation=act)
        with pytest.raises(ValueError, match="activation %s: the exchange engines" % act):
            FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, factor_comm=object(), activation=act)
        with pytest.raises(ValueError, match="runs on the GPU"):  # (the usual CPU refusal)
            FusedMLPTrainer(p, x, y, 100, 0.1, activation=act)
    with pytest.raises(ValueError, match="unknown hidden activation"):
        FusedMLPTrainer(p, x, y, 100, 0.1, activation="gelu")


# ---- the mirrored CPU loop and the eval job ------------------------------------------------------
B, STEPS, LR = 16, 6, 0.05
N = 5 * B + 7


def _dataset():
    from distributedtensorflowexample_amd.data.mnist import DataSet, DataSets

    g = torch.Generator().manual_seed(3)
    x = torch.rand(N, 784, generator=g).numpy()
    y = torch.randint(0, 10, (N,), generator=g).numpy().astype(np.uint8)
    test = DataSet(x[:8], y[:8], one_hot=False)
    return DataSets(train=DataSet(x, y, one_hot=False), validation=test, test=test,
                    synthetic_train=True)


def _run(tmp_path, tag, steps=STEPS, **kw):
    from distributedtensorflowexample_amd.train.mirrored_mlp import train_mirrored

    fl = types.SimpleNamespace(batch_size=B, learning_rate=LR, training_steps=steps,
                               logdir=str(tmp_path / tag), log_every=1, eval_every=3,
                               save_model_secs=1000.0, save_summaries_secs=1000.0,
                               use_locking=False, seed=0, device="cpu", **kw)
    return train_mirrored(fl, _dataset(), log=lambda *_: None)


def test_mirrored_cpu_loop_honours_the_flag(tmp_path, monkeypatch):
    """``train_mirrored`` with ``device="cpu"``: relu and tanh end at parameters other than the
    sigmoid run's (the flag used to be ignored here), the default is the sigmoid run bit for bit,
    and the relu run is the float64 loop of ``activation_reference.step`` within 1e-4 -- 6 steps
    at lr 0.05 whose f32 gradient elements (sums over 16 rows of 784 products of N(0, 1)
    parameters, |g| of a few units) carry errors of about 1e-5."""
    from distributedtensorflowexample_amd.models import mlp as mlp_model

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    _, sig = _run(tmp_path, "sig", activation="sigmoid")
    _, dflt = _run(tmp_path, "dflt")
    _, relu = _run(tmp_path, "relu", activation="relu")
    _, tanh = _run(tmp_path, "tanh", activation="tanh")
    assert torch.equal(sig, dflt)
    assert float((relu - sig).abs().max()) > 1e-3
    assert float((tanh - sig).abs().max()) > 1e-3
    assert float((tanh - relu).abs().max()) > 1e-3
    ds = _dataset()
    x = torch.from_numpy(ds.train.images).double()
    y = torch.from_numpy(ds.train.labels).int()
    for act, got in (("relu", relu), ("tanh", tanh)):
        p = mlp_model.init_params("cpu", seed=0).double()
        nb = N // B
        for s in range(STEPS):
            sl = slice((s % nb) * B, (s % nb + 1) * B)
            p = p - float(np.float32(LR)) * ar.step(p, x[sl], y[sl], act)["grad"]
        err = float((got.double() - p).abs().max())
        print("%s: max |p - p64| after %d steps %.3e" % (act, STEPS, err))
        assert err <= 1e-4
    with pytest.raises(ValueError, match="unknown hidden activation"):
        _run(tmp_path, "bad", activation="gelu")


def test_eval_job_evaluates_with_the_flag(tmp_path):
    """``eval_job`` on a checkpoint with ``--activation relu --device cpu`` reports the relu
    model's figures (the op's own on the same data), which are not the sigmoid model's."""
    from distributedtensorflowexample_amd.data.mnist import read_test_set
    from distributedtensorflowexample_amd.train.eval_job import eval_job
    from distributedtensorflowexample_amd.train.saver import FastSaver
    from distributedtensorflowexample_amd.train.worker import flat_to_tf_vars

    p = dr.data(100)[0]
    logdir = str(tmp_path / "run")
    v = {k: t.contiguous() for k, t in flat_to_tf_vars(p).items()}
    v["global/global_step"] = torch.tensor(77, dtype=torch.int32)
    FastSaver({k: None for k in v}).save(None, os.path.join(logdir, "model.ckpt"),
                                          global_step=77, variables=v)
    test = read_test_set()
    x = torch.from_numpy(np.ascontiguousarray(test.images, np.float32))
    y = torch.from_numpy(np.asarray(test.labels).astype(np.int32))
    seen = {}
    for act in (None, "relu", "tanh"):
        lines = []
        fl = types.SimpleNamespace(logdir=logdir, device="cpu", data_dir="", eval_output="")
        if act is not None:
            fl.activation = act
        assert eval_job(fl, log=lines.append) == 0
        out = dict(l.split(": ", 1) for l in lines if ": " in l)
        want = mlp_eval.evaluate(p, x, y, activation=act or "sigmoid")
        assert out["global_step"] == "77"
        assert float(out["test accuracy"]) == want.accuracy
        assert float(out["test loss"]) == want.loss
        assert out.get("activation") == act
        seen[act] = float(out["test loss"])
    ref = ar.step(p, x, y, "relu")
    assert abs(seen["relu"] - float(ref["loss"])) <= 1e-4 * max(1.0, abs(float(ref["loss"])))
    assert abs(seen["relu"] - seen[None]) > 1e-3 and abs(seen["tanh"] - seen[None]) > 1e-3
    with pytest.raises(SystemExit, match="unknown hidden activation"):
        eval_job(types.SimpleNamespace(logdir=logdir, device="cpu", data_dir="",
                                       activation="gelu"))


# ---- the figures the GPU tests rely on -----------------------------------------------------------
@pytest.mark.parametrize("size", dr.SIZES)
def test_float64_preconditions_of_the_gpu_tests(size):
    """At the initial parameters of ``dropout_reference.data``: the units within 1e-4 of ReLU's
    kink are at most 0.1 % of B x 100 (0 / 1 / 0 / 0 / 3 of 300 / 5,100 / 30,000 / 33,900 /
    76,800 over the three batches of B = 1 / 17 / 100 / 113 / 256), and rows with a top-2 logit
    gap of 1e-3 or less at most 1 %, for relu and tanh."""
    p, x, y = dr.data(size)
    z1 = ar.forward(p, x, "relu")[0]
    near = int(ar.near_kink(z1).sum())
    print("B=%d: %d of %d units with |z1| <= 1e-4, min |z1| %.2e"
          % (size, near, z1.numel(), float(z1.abs().min())))
    assert near == {1: 0, 17: 1, 100: 0, 113: 0, 256: 3}[size]
    assert near <= 0.001 * z1.numel()
    assert int(ar.near_kink(z1[:size]).sum()) <= 0.001 * size * 100  # (the head tests' batch)
    for act in ("relu", "tanh"):
        for rate in (0.0, 0.5):
            keep = dr.keep_mask(dr.SEED, 0, 0, size, rate) if rate else None
            r = ar.step(p, x[:size], y[:size], act, keep, 2.0 if rate else 1.0)
            amb = int((r["gap"] <= 1e-3).sum())
            print("B=%d %s dropout %g: %d rows with a top-2 gap <= 1e-3" % (size, act, rate, amb))
            assert amb <= 0.01 * size
