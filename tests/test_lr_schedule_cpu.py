"""Learning-rate schedules (``ops/lr_schedule.py``, ``--lr_schedule``), CPU tier: the float64
oracle against the TF definitions, the f32 emulation of the device arithmetic against its derived
bound and its exact cases, flags / validation / refusals, the mirrored CPU loop and resume."""
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from distributedtensorflowexample_amd import flags as F
from distributedtensorflowexample_amd.ops import lr_schedule, mlp_step, optim
from distributedtensorflowexample_amd.ops.lr_schedule import LRSchedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAY_STEPS = (1, 3, 7, 1000)
WARMUPS = (0, 5)


def _steps(ds, warm):
    """Stair edges of ``ds`` (k ds - 1, k ds, k ds + 1), the warm-up edge and a few far steps."""
    s = {0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14, 15, 20, 21, 22, 100}
    for k in (1, 2, 3, 10):
        s.update({k * ds - 1, k * ds, k * ds + 1})
    if warm:
        s.update({warm - 2, warm - 1, warm, warm + 1})
    return sorted(v for v in s if v >= 0)


# ---- the oracle ------------------------------------------------------------------------------------
def _tf_exponential_decay(lr, step, decay_steps, rate, staircase):
    p = step / decay_steps
    if staircase:
        p = math.floor(p)
    return lr * math.pow(rate, p)


def _tf_inverse_time_decay(lr, step, decay_steps, rate, staircase):
    p = step / decay_steps
    if staircase:
        p = math.floor(p)
    return lr / (1.0 + rate * p)


@pytest.mark.parametrize("kind", ["exponential", "inverse_time"])
@pytest.mark.parametrize("staircase", [False, True])
def test_value_is_the_tf_definition(kind, staircase):
    tf = _tf_exponential_decay if kind == "exponential" else _tf_inverse_time_decay
    lr0, rate, n = 0.3, 0.9, 0
    for ds in DECAY_STEPS:
        for warm in WARMUPS:
            sch = LRSchedule(kind, ds, rate, staircase, warm)
            for s in _steps(ds, warm):
                want = tf(lr0, s, ds, rate, staircase)
                if warm:
                    want *= min(1.0, (s + 1) / warm)
                got = sch.value(lr0, s)
                assert abs(got - want) <= 4 * 2.0 ** -53 * want, (kind, staircase, ds, warm, s)
                n += 1
    assert n > 100
    # constant: the rate, and the warm-up alone
    assert LRSchedule().value(0.3, 12345) == 0.3
    assert [LRSchedule("constant", warmup_steps=5).value(1.0, s) for s in range(7)] == [
        0.2, 0.4, 0.6, 0.8, 1.0, 1.0, 1.0]


# ---- the emulation's bound -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exponential", "inverse_time"])
@pytest.mark.parametrize("staircase", [False, True])
def test_value_f32_within_the_derived_bound(kind, staircase):
    """x = q log2(rate) is formed with three f32 roundings (l2r, float(s) * inv, the product):
    relative error of decay <= ln 2 * 3 * 2^-24 |x|; exp2 adds an ulp, the remaining
    multiplications a few 2^-24.  Bound: 2^-22 (4 + |x|) (about 2x the derivation), |x| <= 24
    on the whole grid (asserted, so the bound is never vacuous); inverse time: |x| = 0."""
    lr0, worst = 0.3, 0.0
    for rate in (0.96, 0.5, 0.1, 1.5):
        for ds in DECAY_STEPS:
            for warm in WARMUPS:
                sch = LRSchedule(kind, ds, rate, staircase, warm)
                for s in _steps(ds, warm) + [997, 2000, 5003]:
                    q = (s // ds) if staircase else s / ds
                    x = abs(q * math.log2(rate)) if kind == "exponential" else 0.0
                    if x > 24:  # (outside the grid the bound is stated for)
                        continue
                    assert x <= 24
                    want = sch.value(lr0, s)
                    got = sch.value_f32(lr0, s)
                    assert isinstance(got, np.float32)
                    rel = abs(float(got) - want) / want
                    worst = max(worst, rel / (2.0 ** -22 * (4 + x)))
                    assert rel <= 2.0 ** -22 * (4 + x), (kind, staircase, rate, ds, warm, s, rel)
    print(kind, staircase, "largest error / bound %.3f" % worst)
    assert worst > 0  # (the grid exercises inexact cases too)


def test_grid_of_the_bound_reaches_large_exponents():
    """The grid above is not trimmed to nothing: |x| up to ~24 is in it."""
    xs = [abs((s / ds) * math.log2(rate)) for rate in (0.96, 0.5, 0.1, 1.5) for ds in DECAY_STEPS
          for s in _steps(ds, 0) + [997, 2000, 5003]]
    assert max(x for x in xs if x <= 24) > 20


# ---- exact cases -----------------------------------------------------------------------------------
def test_exact_cases_bit_for_bit():
    lr0 = np.float32(0.3)
    for ds in DECAY_STEPS:
        for staircase in (False, True):
            one = LRSchedule("exponential", ds, 1.0, staircase, 0)
            for s in _steps(ds, 0):
                assert one.value_f32(0.3, s) == lr0
    # a staircase longer than the run, and the constant kind: the identity as well
    for s in range(40):
        assert LRSchedule("exponential", 1000, 0.5, True, 0).value_f32(0.3, s) == lr0
        assert LRSchedule("inverse_time", 1000, 0.5, True, 0).value_f32(0.3, s) == lr0
        assert LRSchedule("constant").value_f32(0.3, s) == lr0
    # halving staircase: lr0 * 2^-(s // ds), exactly -- what floorf(float(s) * f32(1 / ds)) misses
    for ds in (3, 7):
        sch = LRSchedule("exponential", ds, 0.5, True, 0)
        for s in range(0, 12 * ds + 2):
            want = np.float32(np.float64(lr0) * 2.0 ** -(s // ds))  # (a power of two: exact)
            assert sch.value_f32(0.3, s) == want, (ds, s)


def test_args_are_the_device_words():
    flags, ds, a, inv, invw = LRSchedule("exponential", 7, 0.96, False, 5).args()
    assert (flags, ds) == (1, 7)
    assert np.float32(a) == np.float32(math.log2(0.96)) and np.float32(inv) == np.float32(1 / 7)
    assert np.float32(invw) == np.float32(0.2)
    flags, ds, a, _, invw = LRSchedule("inverse_time", 3, 0.5, True, 0).args()
    assert (flags, ds, a, invw) == (2 | 4, 3, 0.5, 0.0)
    w = LRSchedule("inverse_time", 3, 0.5, True, 0).block_words()
    assert w.dtype == np.int32 and w.shape == (8,) and list(w[:4]) == [0, 0, 6, 3]
    assert w[4:7].view(np.float32).tolist() == [0.5, float(np.float32(1 / 3)), 0.0]


# ---- flags, validation, refusals -------------------------------------------------------------------
def test_flags_defaults_and_values():
    fv = F.FlagValues()
    F.define_reference_flags(fv)
    fv(["main.py"])
    assert fv.lr_schedule == "constant" and fv.lr_warmup_steps == 0 and fv.lr_staircase is False
    assert lr_schedule.from_flags(fv) is None
    fv.reset()
    fv(["main.py", "--lr_schedule", "exponential", "--lr_decay_steps=7", "--lr_decay_rate", "0.5",
        "--lr_staircase", "--lr_warmup_steps", "5"])
    s = lr_schedule.from_flags(fv)
    assert (s.kind, s.decay_steps, s.decay_rate, s.staircase, s.warmup_steps) == (
        "exponential", 7, 0.5, True, 5)
    fv.reset()
    fv(["main.py", "--lr_warmup_steps", "3"])  # warm-up alone is a schedule
    assert lr_schedule.from_flags(fv).kind == "constant"
    assert lr_schedule.from_flags(types.SimpleNamespace()) is None


@pytest.mark.parametrize("kw, needle", [
    (dict(kind="cosine"), "--lr_schedule must be one of"),
    (dict(kind="exponential", decay_steps=0), "--lr_decay_steps"),
    (dict(kind="exponential", decay_rate=0.0), "--lr_decay_rate"),
    (dict(kind="inverse_time", decay_rate=-1.0), "--lr_decay_rate"),
    (dict(kind="constant", warmup_steps=-1), "--lr_warmup_steps"),
])
def test_validation(kw, needle):
    with pytest.raises(ValueError, match=needle):
        LRSchedule(**kw)


def test_trainer_refuses_before_touching_anything():
    """The constructor's refusals come first: the parameters are CPU tensors and the
    communicator is a plain object, neither is looked at."""
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = torch.zeros(mlp_step.NPARAM), torch.zeros(300, 784), torch.zeros(300).int()
    sch = LRSchedule("exponential", 7, 0.96, False, 5)
    with pytest.raises(ValueError, match="lr_schedule: the exchange engines"):
        FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, fused_comm=object(), lr_schedule=sch)
    with pytest.raises(ValueError, match="lr_schedule: the exchange engines"):
        FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, factor_comm=object(), lr_schedule=sch)
    with pytest.raises(ValueError, match="pipeline=False"):
        FusedMLPTrainer(p, x, y, 100, 0.1, pipeline=False, lr_schedule=sch)
    with pytest.raises(ValueError, match="must be an ops.lr_schedule.LRSchedule"):
        FusedMLPTrainer(p, x, y, 100, 0.1, lr_schedule="exponential")
    # the constant schedule is no schedule: the usual CPU refusal, not a schedule one
    with pytest.raises(ValueError, match="runs on the GPU"):
        FusedMLPTrainer(p, x, y, 100, 0.1, pipeline=False, lr_schedule=LRSchedule())


def test_select_keeps_the_allreduce_engine():
    from distributedtensorflowexample_amd.parallel.select import pick_mlp_engine

    comm = object()
    sch = LRSchedule("inverse_time", 3, 0.5)
    assert pick_mlp_engine(None, None, None, 100, 0.1, comm, 4, 0, "cpu", mode="fused2",
                           lr_schedule=sch) == ("allreduce", comm, None)
    assert pick_mlp_engine(None, None, None, 100, 0.1, comm, 4, 0, "cpu", mode="auto",
                           optimizer="adam") == ("allreduce", comm, None)


def _wflags(**kw):
    d = dict(batch_size=100, learning_rate=0.05, training_steps=10, logdir="unused",
             use_locking=False, seed=0, ps_device="cpu", num_workers=1, sync_replicas=False,
             optimizer="sgd", lr_schedule="exponential", lr_decay_steps=7, lr_decay_rate=0.96,
             lr_staircase=False, lr_warmup_steps=0)
    d.update(kw)
    return types.SimpleNamespace(**d)


@pytest.mark.parametrize("ps_device", ["cpu", "gpu"])
def test_ps_async_worker_refuses(ps_device, tmp_path, monkeypatch):
    from distributedtensorflowexample_amd.train.worker import Worker

    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="ps_async.*--strategy mirrored"):
        Worker("worker", 0, None, _wflags(ps_device=ps_device), device="cpu")
    assert os.listdir(str(tmp_path)) == []


def test_mirrored_models_and_zero1_refuse(tmp_path, monkeypatch):
    from distributedtensorflowexample_amd.train.mirrored_mlp import train_mirrored
    from distributedtensorflowexample_amd.train.mirrored_models import train_model_mirrored

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    for model in ("bert", "resnet50"):
        with pytest.raises(ValueError, match="--model %s.*--strategy mirrored" % model):
            train_model_mirrored(_wflags(model=model, device="cpu", logdir=str(tmp_path / "m")))
    with pytest.raises(ValueError, match="--zero1.*--strategy mirrored"):
        train_mirrored(_wflags(device="cpu", zero1=True, logdir=str(tmp_path / "z")), None)
    assert os.listdir(str(tmp_path)) == []


def _main(args, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, env=env,
                          cwd=ROOT, capture_output=True, text=True, timeout=timeout)


def test_cli_refuses_ps_async(tmp_path):
    r = _main(["--strategy", "ps_async", "--job_name", "worker", "--lr_schedule", "exponential",
               "--logdir", str(tmp_path / "no")])
    assert r.returncode != 0
    assert "--lr_schedule exponential" in r.stderr and "--strategy mirrored" in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "no"))


# ---- the mirrored CPU loop -------------------------------------------------------------------------
B, STEPS, LR = 16, 12, 0.3
N = 5 * B + 7
SCHED = dict(lr_schedule="exponential", lr_decay_steps=7, lr_decay_rate=0.96, lr_staircase=False,
             lr_warmup_steps=5)


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
                               logdir=str(tmp_path / tag), log_every=1, eval_every=10 ** 9,
                               save_model_secs=1000.0, save_summaries_secs=1000.0,
                               use_locking=False, seed=0, device="cpu", **kw)
    return train_mirrored(fl, _dataset(), log=lambda *_: None)


def test_mirrored_cpu_loop_uses_value_f32(tmp_path, monkeypatch):
    """12 sgd steps with the exponential schedule and warm-up equal a hand-written loop of
    ``reference_step`` + ``sgd_`` at ``value_f32(lr0, step)`` (two f32 operation sequences for
    the gradient: 1e-5 on the parameters, as tests/test_fused_optim_cpu.py allows), and differ
    from the constant-rate run by far more."""
    from distributedtensorflowexample_amd.models import mlp as mlp_model

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    ds = _dataset()
    x = torch.from_numpy(ds.train.images).float()
    y = torch.from_numpy(ds.train.labels).int()
    p = mlp_model.init_params("cpu", seed=0).clone()
    sch = LRSchedule("exponential", 7, 0.96, False, 5)
    nb = N // B
    for s in range(STEPS):
        sl = slice((s % nb) * B, (s % nb + 1) * B)
        g, _, _ = mlp_step.reference_step(p, x[sl], y[sl])
        optim.sgd_(p, g, float(sch.value_f32(LR, s)))
    hist, got = _run(tmp_path, "sched", **SCHED)
    _, const = _run(tmp_path, "const")
    assert [h[0] for h in hist] == list(range(1, STEPS + 1))
    print("max |dp| vs the hand-written loop", float((got - p).abs().max()),
          "vs the constant run", float((got - const).abs().max()))
    assert float((got - p).abs().max()) <= 1e-5
    assert float((got - const).abs().max()) > 1e-3


def test_resume_continues_on_the_curve(tmp_path, monkeypatch):
    """A checkpoint written at step 5 and restored continues with lr(5), not lr(0): the continued
    run is the uninterrupted one bit for bit (the schedule is a pure function of global_step)."""
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    _, full = _run(tmp_path, "full", 10, **SCHED)
    _run(tmp_path, "part", 5, **SCHED)
    hist, cont = _run(tmp_path, "part", 10, **SCHED)
    assert [h[0] for h in hist] == [6, 7, 8, 9, 10]
    assert torch.equal(full, cont)
    # a run that restarted the curve at the restore would not be
    sch = LRSchedule("exponential", 7, 0.96, False, 5)
    assert sch.value_f32(LR, 5) != sch.value_f32(LR, 0)
