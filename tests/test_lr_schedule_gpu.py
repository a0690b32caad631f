"""Learning-rate schedules evaluated on the device (``FusedMLPTrainer(lr_schedule=...)``, the
scheduled instantiations of ``mlp_lean_fwdapply``, ``mlp_lr_sched``): the identity schedule is
the unscheduled trainer's bits, the published rate is exact where it can be and within the
derived bound elsewhere, the rate reported is the rate applied, float64 trajectories, the
all-reduce engine, graph replay across reshuffled epochs and the refusals.

Every dataset has 3 batches (so ``x_prev`` wraps) unless a test says otherwise; batch sizes 1
(single row), 17 (generic NGT = 0 tail), 100 (the NGT = 7 instantiation), 113 (the first size
past it) and 256 (B > 128: phase B's late row tiles)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import optim_reference as oref
from distributedtensorflowexample_amd.ops import mlp_step
from distributedtensorflowexample_amd.ops.lr_schedule import LRSchedule
from distributedtensorflowexample_amd.parallel import gpu_ps_optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 17, 100, 113, 256]
KINDS = ["sgd", "momentum", "adam"]
MODES = ["step", "graph", "launched"]
NB = 3
LR0 = {"sgd": 0.3, "momentum": 0.05, "adam": 1e-3}
EPS = 1e-3  # Adam's epsilon in the trajectory tests (tests/test_fused_optim_gpu.py explains)

EXP_WARM = LRSchedule("exponential", 7, 0.96, False, 5)
INV_WARM = LRSchedule("inverse_time", 7, 0.5, False, 5)


def halving(ds):
    return LRSchedule("exponential", ds, 0.5, True, 0)


def _data(B, nb=NB, seed=0, extra=0):
    """CPU f32 (p, x, y): the same values wherever they are generated."""
    g = torch.Generator().manual_seed(1000 * seed + B)
    p = 0.1 * torch.randn(mlp_step.NPARAM, generator=g)
    p[mlp_step.OFF_B1:mlp_step.OFF_W2].zero_()
    p[mlp_step.OFF_B2:].zero_()
    x = torch.rand(nb * B + extra, 784, generator=g)
    y = torch.randint(0, 10, (nb * B + extra,), generator=g).int()
    return p, x, y


def _trainer(gpu, B, lr, data=None, **kw):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = data if data is not None else _data(B)
    return FusedMLPTrainer(p.to(gpu), x.to(gpu), y.to(gpu), B, lr, **kw)


def _advance(tr, mode, n):
    if mode == "step":
        for _ in range(n):
            tr.step()
    elif mode == "graph":
        tr.max_graph_steps = 3
        tr.run(n)
    else:
        tr.run_launched(n)


def _finish(tr, mode):
    if mode == "launched":
        tr.run_launched(0, flush=True)
    else:
        tr.flush()


def _bound(sch, s):
    """Relative error allowed between the device's rate and ``value()`` (derived in
    tests/test_lr_schedule_cpu.py): 2^-22 (4 + |x|), x = q log2(decay_rate) for the exponential
    kind, 0 for inverse time."""
    x = 0.0
    if sch.kind == "exponential":
        q = (s // sch.decay_steps) if sch.staircase else s / sch.decay_steps
        x = abs(q * math.log2(sch.decay_rate))
    assert x <= 24
    return 2.0 ** -22 * (4 + x)


# ---- 1. the identity schedule is the parent's bits ---------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", SIZES)
def test_identity_schedule_is_the_unscheduled_trainer_bit_for_bit(gpu, B, kind, mode):
    """7 steps + flush, then 8 more + flush (both buffer parities, a re-primed pipeline): a
    trainer with decay_rate 1 and one whose staircase is longer than the run run the scheduled
    instantiations and must give the unscheduled trainer's parameters, slots and stats."""
    kw = dict(optimizer=kind)
    trs = [_trainer(gpu, B, LR0[kind], **kw),
           _trainer(gpu, B, LR0[kind], lr_schedule=LRSchedule("exponential", 5, 1.0, False, 0),
                    **kw),
           _trainer(gpu, B, LR0[kind], lr_schedule=LRSchedule("exponential", 1000, 0.5, True, 0),
                    **kw)]
    assert trs[0].sched is None and trs[1].sched is not None and trs[2].sched is not None
    done = 0
    for n in (7, 8):
        for tr in trs:
            if mode == "launched" and n == 8:  # the flush issued by the same C++ call
                tr.run_launched(n, flush=True)
            else:
                _advance(tr, mode, n)
                assert tr.pending
                _finish(tr, mode)
        done += n
        torch.cuda.synchronize()
        ref = trs[0]
        for tr in trs[1:]:
            assert tr.global_step() == ref.global_step() == done
            assert torch.equal(tr.params, ref.params)
            assert len(tr.slots) == len(ref.slots)
            for a, b in zip(tr.slots, ref.slots):
                assert torch.equal(a, b)
            assert torch.equal(tr.stats_range(0, done), ref.stats_range(0, done))
            want = torch.full((done,), float(np.float32(LR0[kind])))
            assert torch.equal(tr.learning_rates(0, done), want)


# ---- 2. the reported rate is exact where it can be -----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ds", [3, 7])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [17, 100])
def test_halving_staircase_rate_is_exact(gpu, B, kind, ds, mode):
    """lr0 2^-(s // decay_steps), bit for bit, across a mid-run flush, a flush issued by the C++
    call and a seek: which step word every launch reads, the integer division, and (graph mode)
    that no rate is baked into a captured graph."""
    lr0 = 0.3
    tr = _trainer(gpu, B, lr0, optimizer=kind, lr_schedule=halving(ds))

    def want(a, b):
        return torch.tensor([np.float32(lr0) * np.float32(2.0 ** -(s // ds)) for s in range(a, b)],
                            dtype=torch.float32)

    _advance(tr, mode, 4)
    tr.flush()  # mid-run
    if mode == "launched":
        tr.run_launched(6, flush=True)
    else:
        _advance(tr, mode, 6)
    _advance(tr, mode, 5)
    _finish(tr, mode)
    torch.cuda.synchronize()
    assert tr.global_step() == 15
    got = tr.learning_rates(0, 15)
    print("B", B, kind, ds, mode, got.tolist())
    assert torch.equal(got, want(0, 15))
    assert tr.learning_rate() == float(want(14, 15)[0]) == tr.learning_rate(14)
    tr.seek(10)
    tr.opt.rates.zero_()
    _advance(tr, mode, 3)
    assert torch.equal(tr.learning_rates(10, 13), want(10, 13))
    assert tr.global_step() == 13


# ---- 3. the reported rate against float64 ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sch", [EXP_WARM, INV_WARM], ids=["exponential", "inverse_time"])
def test_rate_within_the_bound_of_float64(gpu, sch, mode):
    B, lr0 = 100, 0.3
    tr = _trainer(gpu, B, lr0, lr_schedule=sch)
    worst = 0.0
    for start in (0, 1000):
        if start:
            tr.seek(start)
        _advance(tr, mode, 16)
        got = tr.learning_rates(start, start + 16).double().tolist()
        for i, r in enumerate(got):
            s = start + i
            ref = sch.value(lr0, s)
            rel = abs(r - ref) / ref
            worst = max(worst, rel / _bound(sch, s))
            assert rel <= _bound(sch, s), (s, r, ref, rel)
    print(sch, mode, "largest error / bound %.3f" % worst)


# ---- 4. the rate reported is the rate applied ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["step", "launched"])
@pytest.mark.parametrize("sch", [EXP_WARM, halving(3)], ids=["exponential", "halving"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [17, 100])
def test_reported_rate_is_the_applied_rate(gpu, B, kind, sch, mode):
    """An unscheduled trainer -- the constant-rate kernels -- whose host ``lr`` is set before
    every launch to the f32 rate the scheduled trainer reported for the step that launch
    applies, run one step at a time: the same parameters, slots and stats, bit for bit."""
    n = 12
    kw = dict(optimizer=kind, epsilon=EPS)
    data = _data(B)
    tr = _trainer(gpu, B, LR0[kind], data, lr_schedule=sch, **kw)
    if mode == "step":
        _advance(tr, mode, n)
        tr.flush()
    else:
        tr.run_launched(n)
        tr.run_launched(0, flush=True)
    rates = tr.learning_rates(0, n).tolist()
    oracle = _trainer(gpu, B, LR0[kind], data, **kw)
    for k in range(n):
        oracle.lr = rates[k - 1] if k else 0.0  # (launch k applies step k - 1; launch 0 nothing)
        if mode == "step":
            oracle.step()
        else:
            oracle.run_launched(1)
    oracle.lr = rates[n - 1]
    _finish(oracle, mode)
    torch.cuda.synchronize()
    assert oracle.global_step() == tr.global_step() == n
    assert torch.equal(tr.params, oracle.params)
    for a, b in zip(tr.slots, oracle.slots):
        assert torch.equal(a, b)
    assert torch.equal(tr.stats_range(0, n), oracle.stats_range(0, n))
    assert len(set(rates)) > 3  # (the rate did move)


@pytest.mark.gpu
@pytest.mark.parametrize("sch", [EXP_WARM, halving(3)], ids=["exponential", "halving"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [17, 100])
def test_graph_replay_is_the_step_mode_run(gpu, B, kind, sch):
    """Graph mode: the parameters within the suite's 1e-5 of the step-mode run, the rate ring
    equal."""
    n, out = 12, []
    for mode in ("step", "graph"):
        tr = _trainer(gpu, B, LR0[kind], optimizer=kind, epsilon=EPS, lr_schedule=sch)
        _advance(tr, mode, n)
        tr.flush()
        torch.cuda.synchronize()
        out.append((tr.params.clone(), tr.learning_rates(0, n)))
    assert (out[0][0] - out[1][0]).abs().max().item() < 1e-5
    assert torch.equal(out[0][1], out[1][1])


# ---- 5. trajectories --------------------------------------------------------------------------------
TRAJ_STEPS = 12


def trajectory(kind, B, dtype, sch=EXP_WARM):
    """12 steps on the CPU in ``dtype``: float64 -> reference_step + optim_reference at
    ``value()`` (the oracle); float32 -> reference_step + gpu_ps_optim.apply_reference at
    ``value_f32()`` (the f32 yardstick)."""
    p, x, y = _data(B)
    lr0 = LR0[kind]
    hyper = gpu_ps_optim.hyper_args(kind, epsilon=EPS)
    p, x = p.to(dtype), x.to(dtype)
    slots = [torch.zeros_like(p) for _ in range(gpu_ps_optim.num_slots(kind))]
    for s in range(TRAJ_STEPS):
        sl = slice((s % NB) * B, (s % NB + 1) * B)
        g, _, _ = mlp_step.reference_step(p, x[sl], y[sl])
        if dtype == torch.float64:
            lr = sch.value(lr0, s)
            if kind == "sgd":
                p, _ = oref.sgd_step(p, g, lr)
            elif kind == "momentum":
                p, buf = oref.sgd_step(p, g, lr, mu=0.9, buf=slots[0])
                slots = [buf]
            else:
                p, m, v = oref.adam_step(p, g, slots[0], slots[1], lr, s + 1, eps=EPS, wd=0.0,
                                         adamw=False)
                slots = [m, v]
        else:
            pn, sn = gpu_ps_optim.apply_reference(kind, p.numpy(), g.numpy(),
                                                  [t.numpy() for t in slots],
                                                  sch.value_f32(lr0, s), s + 1, hyper)
            p, slots = torch.from_numpy(pn), [torch.from_numpy(t) for t in sn]
    return p


# max |p_f32 - p_f64| of the two CPU trajectories above after 12 steps (measured once on the CPU)
CPU_GAP = {
    ("sgd", 1): 2.200e-07, ("sgd", 17): 1.016e-07, ("sgd", 100): 9.867e-08,
    ("sgd", 113): 1.054e-07, ("sgd", 256): 9.295e-08,
    ("momentum", 1): 8.925e-08, ("momentum", 17): 8.223e-08, ("momentum", 100): 9.568e-08,
    ("momentum", 113): 1.014e-07, ("momentum", 256): 1.032e-07,
    ("adam", 1): 8.820e-08, ("adam", 17): 9.599e-08, ("adam", 100): 1.020e-07,
    ("adam", 113): 9.278e-08, ("adam", 256): 9.459e-08,
}


def traj_tol(kind, B):
    return 4.0 * CPU_GAP[(kind, B)]


@pytest.fixture(scope="module")
def traj64():
    cache = {}

    def get(kind, B):
        if (kind, B) not in cache:
            cache[(kind, B)] = trajectory(kind, B, torch.float64)
        return cache[(kind, B)]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", SIZES)
def test_scheduled_trajectory_matches_float64(gpu, traj64, B, kind):
    """12 steps of sgd (0.3), momentum (0.05, mu 0.9) and Adam (1e-3, epsilon 1e-3) under the
    exponential schedule with warm-up, through step(), run() and run_launched(flush=True),
    against the float64 trajectory.  Tolerance: 4 x CPU_GAP, the distance between that float64
    trajectory and the f32 CPU one (the table above, measured on the CPU; never taken from the
    GPU result)."""
    ref = traj64(kind, B)
    tol = traj_tol(kind, B)
    errs = []
    for mode in MODES:
        tr = _trainer(gpu, B, LR0[kind], optimizer=kind, epsilon=EPS, lr_schedule=EXP_WARM)
        if mode == "launched":
            tr.run_launched(TRAJ_STEPS, flush=True)
        else:
            _advance(tr, mode, TRAJ_STEPS)
            tr.flush()
        torch.cuda.synchronize()
        assert tr.global_step() == TRAJ_STEPS
        err = (tr.params.double().cpu() - ref).abs().max().item()
        print("trajectory", kind, "B", B, mode, "max |p - p64| %.3e" % err, "tol %.3e" % tol)
        errs.append(err)
    for err in errs:
        assert err <= tol


# ---- 6. the all-reduce engine on one GPU ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_allreduce_engine_matches_single_gpu(gpu, kind):
    """world_size = 2 with an ``allreduce`` that doubles the gradient in place (two identical
    replicas): ``mlp_lr_sched`` + ops.optim's kernels reading the device rate give the one-GPU
    scheduled trainer's trajectory within test 5's tolerance (eager and graph replay) and its
    rate ring bit for bit; snapshot(with_slots=True) / evaluate() with a gradient pending move
    neither parameters, slots, counter nor ring."""
    B = 100
    kw = dict(optimizer=kind, epsilon=EPS, lr_schedule=EXP_WARM)
    one = _trainer(gpu, B, LR0[kind], **kw)
    one.run(TRAJ_STEPS)
    one.flush()
    want_rates = one.learning_rates(0, TRAJ_STEPS)
    for use_graph in (False, True):
        dp = _trainer(gpu, B, LR0[kind], allreduce=lambda g: g.mul_(2.0), world_size=2, **kw)
        assert not dp.pipelined and dp._inplace
        dp.max_graph_steps = 3
        dp.run(TRAJ_STEPS, use_graph=use_graph)
        assert dp.pending
        p, slots = dp.params.clone(), [s.clone() for s in dp.slots]
        ctr, ring = dp.ws.ctr.clone(), dp.opt.rates.clone()
        snap, ssnap = dp.snapshot(with_slots=True)
        assert torch.equal(dp.snapshot(), snap)
        ev = dp.evaluate(dp.x, dp.labels)  # (on snapshot(): the pending gradient on a copy)
        torch.cuda.synchronize()
        assert dp.pending and torch.equal(dp.params, p)
        for a, b in zip(dp.slots, slots):
            assert torch.equal(a, b)
        assert torch.equal(dp.ws.ctr, ctr) and torch.equal(dp.opt.rates, ring)
        assert not torch.equal(snap, p)
        dp.flush()
        torch.cuda.synchronize()
        assert dp.global_step() == TRAJ_STEPS
        assert torch.equal(dp.params, snap)
        for a, b in zip(dp.slots, ssnap):
            assert torch.equal(a, b)
        ev2 = dp.evaluate(dp.x, dp.labels)
        assert (float(ev.accuracy), float(ev.loss)) == (float(ev2.accuracy), float(ev2.loss))
        assert torch.equal(dp.learning_rates(0, TRAJ_STEPS), want_rates)
        err = (dp.params - one.params).abs().max().item()
        print("all-reduce engine", kind, "graph" if use_graph else "eager", "%.3e" % err)
        assert err <= traj_tol(kind, B)


# ---- 7. graph replay across reshuffled epochs -----------------------------------------------------
@pytest.mark.gpu
def test_adam_schedule_graph_replay_across_shuffled_epochs_is_eager(gpu):
    B = 100
    data = _data(B, nb=4, extra=7)  # 4 batches + a dropped tail; 12 steps = 3 epochs
    out = []
    for use_graph in (True, False):
        tr = _trainer(gpu, B, 1e-3, data, optimizer="adam", shuffle=True, shuffle_seed=5,
                      lr_schedule=EXP_WARM)
        tr.max_graph_steps = 3
        tr.run(12, use_graph=use_graph)
        tr.flush()
        torch.cuda.synchronize()
        assert tr.global_step() == 12
        out.append((tr.params.clone(), [s.clone() for s in tr.slots], tr.stats_range(0, 12),
                    tr.learning_rates(0, 12)))
    assert torch.equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a, b)
    assert torch.equal(out[0][2], out[1][2]) and torch.equal(out[0][3], out[1][3])
    assert len(set(out[0][3].tolist())) == 12


# ---- 8. refusals --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_unsupported_combinations_raise_before_any_launch(gpu):
    from distributedtensorflowexample_amd.ops._ext import hip
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = (t.to(gpu) for t in _data(100))
    comm = object()  # never touched: the constructor refuses first
    with pytest.raises(ValueError, match="lr_schedule: the exchange engines"):
        FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, fused_comm=comm, lr_schedule=EXP_WARM)
    with pytest.raises(ValueError, match="lr_schedule: the exchange engines"):
        FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, factor_comm=comm,
                        x_all=torch.stack([x, x]), lr_schedule=EXP_WARM)
    with pytest.raises(ValueError, match="pipeline=False"):
        FusedMLPTrainer(p, x, y, 100, 0.1, pipeline=False, lr_schedule=EXP_WARM)
    tr = FusedMLPTrainer(p, x, y, 100, 0.1, lr_schedule=EXP_WARM)
    assert not tr.persistent_ok
    with pytest.raises(ValueError, match="run_persistent"):
        tr.run_persistent(4)
    old = hip().mlp_set_flush_fused(1)  # DTFX_MLP_FLUSH_FUSED, selected in-process
    try:
        with pytest.raises(RuntimeError, match="fused flush.*no learning-rate schedule"):
            tr.run_launched(4, flush=True)
    finally:
        hip().mlp_set_flush_fused(old)
    torch.cuda.synchronize()
    assert tr.global_step() == 0 and not tr.pending and torch.equal(tr.params, p)
    with pytest.raises(RuntimeError, match="no lr_schedule"):
        FusedMLPTrainer(p, x, y, 100, 0.1).learning_rate()
    assert FusedMLPTrainer(p, x, y, 100, 0.1, lr_schedule=LRSchedule()).persistent_ok


# ---- 9. the mirrored loop on the GPU: summaries and resume ------------------------------------------
@pytest.mark.gpu
def test_mirrored_loop_resumes_on_the_curve(gpu, tmp_path, monkeypatch):
    """``train_mirrored`` on one GPU with a schedule: 5 steps, the chief's checkpoint, a restart
    to 10 -- the bits of an uninterrupted 10-step run (``seek`` puts the step pair back, so the
    restored run continues with lr(5)), and not the constant-rate run's."""
    import types

    from distributedtensorflowexample_amd.data.mnist import DataSet, DataSets
    from distributedtensorflowexample_amd.train.mirrored_mlp import train_mirrored

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    B = 100
    _, x, y = _data(B, extra=7)
    x, y = x.numpy(), y.numpy().astype(np.uint8)
    test = DataSet(x[:64], y[:64], one_hot=False)
    ds = DataSets(train=DataSet(x, y, one_hot=False), validation=test, test=test,
                  synthetic_train=True)
    sched = dict(lr_schedule="exponential", lr_decay_steps=3, lr_decay_rate=0.5,
                 lr_staircase=True, lr_warmup_steps=2)

    def run(tag, steps, **kw):
        fl = types.SimpleNamespace(batch_size=B, learning_rate=0.3, training_steps=steps,
                                   logdir=str(tmp_path / tag), log_every=5, eval_every=10 ** 9,
                                   save_model_secs=1000.0, save_summaries_secs=1000.0,
                                   use_locking=False, seed=0, device="cuda", **kw)
        return train_mirrored(fl, ds, log=lambda *_: None)

    _, full = run("full", 10, **sched)
    run("part", 5, **sched)
    hist, cont = run("part", 10, **sched)
    assert [h[0] for h in hist] == [10]
    assert torch.equal(full, cont)
    _, const = run("const", 10)
    assert (full - const).abs().max().item() > 1e-3


KS14_SCRIPT = """
import torch
from distributedtensorflowexample_amd.ops.lr_schedule import LRSchedule
from distributedtensorflowexample_amd.ops import mlp_step
from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer
p = torch.zeros(mlp_step.NPARAM, device="cuda")
x = torch.zeros(300, 784, device="cuda")
y = torch.zeros(300, dtype=torch.int32, device="cuda")
try:
    FusedMLPTrainer(p, x, y, 100, 0.1, lr_schedule=LRSchedule("exponential", 7, 0.96))
except ValueError as e:
    print("REFUSED", e)
"""


@pytest.mark.gpu
def test_ks14_refuses_a_schedule(gpu):
    """DTFX_MLP_KS is read once per process, so this refusal is shown in a child process."""
    env = dict(os.environ, DTFX_MLP_KS="14")
    r = subprocess.run([sys.executable, "-c", KS14_SCRIPT], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "REFUSED lr_schedule: DTFX_MLP_KS=14" in r.stdout, r.stdout + r.stderr
