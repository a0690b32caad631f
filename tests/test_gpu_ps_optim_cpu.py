"""CPU tier of the GPU parameter store's stateful optimizers (``--optimizer momentum | adam``):
the f32 ``apply_reference`` of parallel/gpu_ps_optim.py against the float64 torch.optim
references of tests/optim_reference.py (the project's own bound for these formulas), the flags,
the Worker's refusals, and checkpoints that carry slot variables."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import optim_reference as R
from distributedtensorflowexample_amd import flags as F
from distributedtensorflowexample_amd import variables as vs
from distributedtensorflowexample_amd.data.mnist import read_test_set
from distributedtensorflowexample_amd.models.dense import make_ps_model
from distributedtensorflowexample_amd.models.mlp import init_params
from distributedtensorflowexample_amd.ops import mlp_eval, mlp_step
from distributedtensorflowexample_amd.parallel import gpu_ps_optim as O
from distributedtensorflowexample_amd.train.saver import FastSaver, Saver
from distributedtensorflowexample_amd.train.worker import (REFERENCE_MLP_NAMES, Worker,
                                                           build_worker_variables,
                                                           flat_to_tf_vars, restricted_assign)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = "global/global_step"
LR = 1e-3  # the reference's learning rate


def test_names_and_hyper_words():
    assert O.num_slots("sgd") == 0 and O.num_slots("momentum") == 1 and O.num_slots("adam") == 2
    assert O.slot_names("momentum", ["global/dense/kernel"]) == [["global/dense/kernel/Momentum"]]
    assert O.slot_names("adam", ["a", "b"]) == [["a/Adam", "b/Adam"], ["a/Adam_1", "b/Adam_1"]]
    assert O.hyper_args("sgd") == ()
    assert O.hyper_args("momentum", momentum=0.5) == (0.5, 0.0, 0.0)
    assert O.hyper_args("adam") == (0.9, 0.999, 1e-8)
    with pytest.raises(ValueError, match="--optimizer"):
        O.check_kind("rmsprop")


@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("t0", [1, 1001])
@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam"])
def test_apply_reference_against_float64(kind, t0, fma):
    """Three consecutive applies from make_case data, starting at t = 1 and t = 1001: the f32
    evaluation stays within optim_reference.bound of torch.optim in float64."""
    n = 4099
    p0, g, m0, v0, regions = R.make_case(n, seed=11)
    hyper = O.hyper_args(kind, momentum=0.9)
    slots32 = {"sgd": [], "momentum": [m0.numpy()], "adam": [m0.numpy(), v0.numpy()]}[kind]
    p32 = p0.numpy()
    p64, m64, v64 = p0.double(), m0.double(), v0.double()
    for k in range(3):
        t = t0 + k
        p32, slots32 = O.apply_reference(kind, p32, g.numpy(), slots32, LR, t, hyper, fma=fma)
        assert p32.dtype == np.float32 and all(s.dtype == np.float32 for s in slots32)
        if kind == "adam":
            p64, m64, v64 = R.adam_step(p64, g, m64, v64, LR, t, adamw=False, wd=0.0)
            want = [m64, v64]
        else:
            p64, buf = R.sgd_step(p64, g, LR, mu=hyper[0] if hyper else 0.0,
                                  buf=m64 if kind == "momentum" else None)
            m64 = buf if kind == "momentum" else m64
            want = [m64] if kind == "momentum" else []
        R.assert_close("%s p (t=%d)" % (kind, t), torch.from_numpy(p32), p64, k + 1, regions)
        for name, got, ref in zip(O.SLOT_NAMES[kind], slots32, want):
            R.assert_close("%s %s (t=%d)" % (kind, name, t), torch.from_numpy(got), ref, k + 1,
                           regions)


def test_apply_reference_exact_data_and_mean():
    """Integer data and power-of-two scalars: the plain and the fused evaluation agree bitwise;
    the mean gradient is the ticket-order sum times an f32 1 / R."""
    n = 1025
    i = np.arange(n, dtype=np.int64)
    p = ((i * 37) % 129 - 64).astype(np.float32)
    gs = [((i * 7 + k * 3) % 17 - 8).astype(np.float32) for k in range(4)]
    gbar = O.mean_gradient(gs)
    assert np.array_equal(gbar, (gs[0] + gs[1] + gs[2] + gs[3]) * np.float32(0.25))
    third = O.mean_gradient(gs[:3])
    assert np.array_equal(third, ((gs[0] + gs[1]) + gs[2]) * (np.float32(1) / np.float32(3)))
    acc = np.zeros(n, np.float32)
    for _ in range(3):
        a = O.apply_reference("momentum", p, gbar, [acc], 0.5, 1, (0.5, 0, 0))
        b = O.apply_reference("momentum", p, gbar, [acc], 0.5, 1, (0.5, 0, 0), fma=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1][0], b[1][0])
        assert np.array_equal(a[1][0], np.float32(0.5) * acc + gbar)
        p, (acc,) = a
    with pytest.raises(ValueError, match="slot arrays"):
        O.apply_reference("adam", p, gbar, [acc], 0.5, 1, (0.9, 0.999, 1e-8))


def test_flags_defaults_and_values():
    fv = F.FlagValues()
    F.define_reference_flags(fv)
    fv(["main.py"])
    assert fv.optimizer == "sgd" and fv.momentum == 0.9
    assert fv.adam_beta1 == 0.9 and fv.adam_beta2 == 0.999 and fv.adam_epsilon == 1e-8
    fv.reset()
    fv(["main.py", "--job_name", "worker", "--ps_device", "gpu", "--optimizer", "adam",
        "--adam_beta1=0.8", "--adam_beta2", "0.99", "--adam_epsilon", "1e-6", "--momentum=0.5"])
    assert fv.optimizer == "adam" and fv.ps_device == "gpu" and fv.momentum == 0.5
    assert (fv.adam_beta1, fv.adam_beta2, fv.adam_epsilon) == (0.8, 0.99, 1e-6)


def test_sync_rounds_pass_the_hyper_words():
    """The host protocol appends the optimizer's hyper-parameter words to every sync_begin, and
    none for sgd (the call the rounds always made)."""
    from distributedtensorflowexample_amd.parallel.gpu_ps_sync import JOINED, SyncRounds

    class Stub:
        def __init__(self):
            self.calls = []

        def sync_begin(self, *args):
            self.calls.append(args)
            return JOINED, args[2], 0, []

        def sync_poll(self, stream):
            return len(self.calls), 0

    for kind, extra in (("sgd", ()), ("momentum", (0.5, 0.0, 0.0)), ("adam", (0.9, 0.999, 1e-8))):
        st = Stub()
        r = SyncRounds(st, 1, hyper=O.hyper_args(kind, momentum=0.5))
        assert r.push(1234, 0.25, 0) == (1, True, [])
        assert st.calls == [(1234, 0.25, 0, 0, 0, 0) + extra]


def _flags(**kw):
    d = dict(batch_size=100, learning_rate=LR, training_steps=10, logdir="unused",
             use_locking=False, seed=0, ps_device="cpu", num_workers=1, sync_replicas=False,
             optimizer="sgd")
    d.update(kw)
    return types.SimpleNamespace(**d)


@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_worker_refusals(kind, tmp_path, monkeypatch):
    """Both refusals come before any device, server or file is touched: the Worker is given
    no server at all and a log directory that must not appear."""
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="TCP ps applies gradient descent only"):
        Worker("worker", 0, None, _flags(optimizer=kind, ps_device="cpu"), device="cpu")
    with pytest.raises(ValueError, match="use_locking"):
        Worker("worker", 0, None, _flags(optimizer=kind, ps_device="gpu", use_locking=True),
               device="cpu")
    with pytest.raises(ValueError, match="--optimizer"):
        Worker("worker", 0, None, _flags(optimizer="adagrad", ps_device="gpu"), device="cpu")
    assert O.validate("sgd", "cpu", True) == "sgd" and O.validate(kind, "gpu", False) == kind
    assert not list(tmp_path.iterdir())


def _var_names(kind):
    gv, tv = build_worker_variables(make_ps_model("mlp", "", None), vs.VariableRegistry(),
                                    optimizer=kind)
    assert [v.name for v in tv] == list(REFERENCE_MLP_NAMES)  # slots are not trainable
    return [v.name for v in gv], gv


def test_registry_declares_the_slots():
    names, gv = _var_names("sgd")
    assert names == list(REFERENCE_MLP_NAMES) + [STEP]
    names, gv = _var_names("momentum")
    assert names == list(REFERENCE_MLP_NAMES) + [STEP] + [k + "/Momentum"
                                                          for k in REFERENCE_MLP_NAMES]
    assert gv[5].name == "global/dense/kernel/Momentum" and gv[5].shape == (784, 100)
    assert not gv[5].trainable and not gv[5].initial_value(0, 5).any()
    names, _ = _var_names("adam")
    assert names[5:] == ([k + "/Adam" for k in REFERENCE_MLP_NAMES]
                         + [k + "/Adam_1" for k in REFERENCE_MLP_NAMES])


def test_graph_emits_the_optimizers_apply_nodes():
    from distributedtensorflowexample_amd.utils.graph import reference_mlp_graph

    ops = {}
    for kind in ("sgd", "momentum", "adam"):
        _, gv = _var_names(kind)
        g = reference_mlp_graph(gv, gv[:4], optimizer=kind)
        ops[kind] = {n[1]: n for n in g.nodes}
        assert g.to_bytes() and g.to_pbtxt()
    assert "ApplyGradientDescent" in ops["sgd"] and "ApplyMomentum" not in ops["sgd"]
    assert "ApplyGradientDescent" not in ops["momentum"] and "ApplyGradientDescent" not in ops["adam"]
    name, _, inputs, device, _ = ops["momentum"]["ApplyMomentum"]
    assert name == "local/Momentum/update_global/dense_1/bias/ApplyMomentum"
    assert inputs[:2] == ["global/dense_1/bias", "global/dense_1/bias/Momentum"]
    assert len(inputs) == 5 and device == "/job:ps/task:0"
    _, _, inputs, _, _ = ops["adam"]["ApplyAdam"]
    assert inputs[:3] == ["global/dense_1/bias", "global/dense_1/bias/Adam",
                          "global/dense_1/bias/Adam_1"]
    assert inputs[3:5] == ["local/Adam/beta1_power", "local/Adam/beta2_power"]
    assert len(inputs) == 10


def _run_eval(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--job_name", "eval",
                           "--device", "cpu"] + args, cwd=ROOT, capture_output=True, text=True,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="4"),
                          timeout=300)


def test_checkpoint_with_slots_on_the_cpu(tmp_path):
    """A bundle holding the five reference variables plus Adam's slots: the eval job evaluates
    it, an sgd-configured restore takes the five and ignores the slots, an adam-configured one
    takes all thirteen, a momentum-configured one raises the saver's KeyError."""
    p = init_params("cpu", seed=3)
    mlp_step.unflatten(p)[0].mul_(0.05)
    names, _ = _var_names("adam")
    values = {k: t.contiguous() for k, t in flat_to_tf_vars(p).items()}
    gen = torch.Generator().manual_seed(5)
    for k in names[5:]:
        values[k] = torch.rand(values[k.rsplit("/", 1)[0]].shape, generator=gen)
    values[STEP] = torch.tensor(77, dtype=torch.int32)
    logdir = str(tmp_path / "run")
    prefix = Saver({k: None for k in names}).save(
        None, os.path.join(logdir, "model.ckpt"), global_step=77, write_meta_graph=False,
        variables=values)

    r = _run_eval(["--logdir", logdir])
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^global_step: 77$", r.stdout, re.M), r.stdout
    test = read_test_set()
    here = mlp_eval.evaluate(p, torch.from_numpy(np.ascontiguousarray(test.images, np.float32)),
                             torch.from_numpy(np.asarray(test.labels).astype(np.int32)))
    assert float(re.search(r"^test accuracy: (\S+)$", r.stdout, re.M).group(1)) == here.accuracy

    for kind, count in (("sgd", 5), ("adam", 13)):
        got = {}
        want, _ = _var_names(kind)
        FastSaver({k: None for k in want}, assign=restricted_assign(got.update, want)).restore(
            None, prefix)
        assert sorted(got) == sorted(want) and len(got) == count
        assert all(torch.equal(got[k], values[k]) for k in got)
    want, _ = _var_names("momentum")
    with pytest.raises(KeyError, match="/Momentum"):
        FastSaver({k: None for k in want}, assign=restricted_assign(dict().update, want)).restore(
            None, prefix)
