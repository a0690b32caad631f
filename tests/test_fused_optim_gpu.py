"""Momentum and Adam inside the fused two-launch MLP step (``FusedMLPTrainer(optimizer=...)``,
``mlp_lean_fwdapply_opt``): bit-identity with SGD at mu = 0, the float64 ``torch.optim``
references fed the kernel's own gradient, the explicit apply bit, float64 trajectories, graph
replay across reshuffled epochs, the all-reduce engine, the refusals and checkpoints.

Every dataset has 3 batches (so ``x_prev`` wraps) unless a test says otherwise; batch sizes 1
(single row), 17 (generic NGT = 0 tail), 100 (the NGT = 7 instantiation), 113 (the first size
past it) and 256 (B > 128: phase B's late row tiles)."""
import types

import numpy as np
import pytest
import torch

import optim_reference as oref
from distributedtensorflowexample_amd.ops import mlp_step
from distributedtensorflowexample_amd.parallel import gpu_ps_optim

SIZES = [1, 17, 100, 113, 256]
NB = 3
W1 = mlp_step.OFF_B1
REGIONS = [("W1", torch.arange(0, W1)), ("small", torch.arange(W1, mlp_step.NPARAM))]


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


# ---- 1. mu = 0 is SGD, bit for bit -------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["step", "graph", "launched"])
@pytest.mark.parametrize("B", SIZES)
def test_momentum_mu0_is_sgd_bit_for_bit(gpu, B, mode):
    """7 steps + flush, then 8 more + flush (both buffer parities, a re-primed pipeline): the
    parameters and the recorded stats of a mu = 0 momentum trainer are the sgd trainer's bits,
    and the slot plane is the last applied gradient (float64 reference of the state it was
    formed at, at the 1e-4 the suite allows the gradient kernels)."""
    lr = 0.3
    ts = _trainer(gpu, B, lr)
    tm = _trainer(gpu, B, lr, optimizer="momentum", momentum=0.0)
    p, x, y = _data(B)
    done = 0
    for n in (7, 8):
        _advance(ts, mode, n)
        _advance(tm, mode, n)
        done += n
        assert tm.pending and ts.pending
        before = tm.params.double().cpu()  # the state the pending gradient belongs to
        if mode == "launched" and n == 8:  # the flush issued by the same C++ call
            ts.run_launched(1, flush=True)
            tm.run_launched(1, flush=True)
            before, done = None, done + 1
        else:
            _finish(ts, mode)
            _finish(tm, mode)
        torch.cuda.synchronize()
        assert ts.global_step() == tm.global_step() == done
        assert torch.equal(ts.params, tm.params)
        assert torch.equal(ts.stats_range(0, done), tm.stats_range(0, done))
        if before is not None:
            b = (done - 1) % NB
            g, _, _ = mlp_step.reference_step(before, x[b * B:(b + 1) * B].double(),
                                              y[b * B:(b + 1) * B])
            err = (tm.slots[0].double().cpu() - g).abs().max().item()
            print("B", B, mode, "slot vs float64 gradient", err)
            assert err < 1e-4
            # ... and exactly the gradient that was applied: p' = p - lr * slot
            want = before - float(np.float32(lr)) * tm.slots[0].double().cpu()
            assert (tm.params.double().cpu() - want).abs().max().item() <= 2.0 ** -24 * max(
                1.0, want.abs().max().item())


# ---- 2. the kernel's own gradient as the oracle ---------------------------------------------------
def _kernel_gradient(oracle, p, step):
    """The exact f32 gradient the kernel forms at (p, batch ``step`` % nb): a mu = 0 momentum
    apply leaves it in the slot plane (test 1)."""
    oracle.load_params(p)
    oracle.seek(step)
    oracle.step()
    oracle.flush()
    return oracle.slots[0].clone()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["momentum", "adam_t1", "adam_t1001"])
@pytest.mark.parametrize("B", SIZES)
def test_apply_matches_float64_reference_on_kernel_gradient(gpu, B, case):
    """Three consecutive applies from non-zero slots at lr = 1e-3 -- two inside following steps'
    first launches, the third by flush() -- against torch.optim in float64 fed the kernel's own
    gradient: p and every slot within optim_reference.bound(k, ref) after k applies, W1 and the
    small parameters separately.  Adam (defaults, eps = 1e-8) from global_step 0 and 1000:
    t = 1, 2, 3 and 1001, 1002, 1003."""
    lr, gs = 1e-3, (1000 if case == "adam_t1001" else 0)
    kind = "momentum" if case == "momentum" else "adam"
    data = _data(B)
    oracle = _trainer(gpu, B, lr, data, optimizer="momentum", momentum=0.0)
    tr = _trainer(gpu, B, lr, data, optimizer=kind)
    gen = torch.Generator().manual_seed(7 + B)
    m0 = 0.1 * torch.randn(mlp_step.NPARAM, generator=gen)
    v0 = 0.01 + 0.1 * torch.rand(mlp_step.NPARAM, generator=gen)
    slots0 = [m0] if kind == "momentum" else [m0, v0]
    tr.load_slots([s.to(gpu) for s in slots0])
    tr.seek(gs)
    ref_p = data[0].double()
    ref_s = [s.double() for s in slots0]
    tr.step()
    for k in range(1, 4):
        assert tr.pending
        g = _kernel_gradient(oracle, tr.params.clone(), gs + k - 1).cpu()
        if k < 3:
            tr.step()   # applies update k (t = gs + k) in its first launch
        else:
            tr.flush()  # ... and the apply-only launch
        torch.cuda.synchronize()
        if kind == "momentum":
            ref_p, buf = oref.sgd_step(ref_p, g, lr, mu=0.9, buf=ref_s[0])
            ref_s = [buf]
        else:
            ref_p, m, v = oref.adam_step(ref_p, g, ref_s[0], ref_s[1], lr, gs + k, eps=1e-8,
                                         wd=0.0, adamw=False)
            ref_s = [m, v]
        oref.assert_close("p after %d" % k, tr.params, ref_p, k, REGIONS)
        for i, (s, r) in enumerate(zip(tr.slots, ref_s)):
            oref.assert_close("slot %d after %d" % (i, k), s, r, k, REGIONS)
    assert tr.global_step() == gs + 3


# ---- 3. apply=False touches no slot byte ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["step", "launched"])
@pytest.mark.parametrize("B", SIZES)
def test_first_step_after_flush_copies_and_leaves_slots(gpu, B, mode):
    tr = _trainer(gpu, B, 0.3, optimizer="adam")
    _advance(tr, mode, 2)
    tr.flush()
    gen = torch.Generator().manual_seed(B)
    tr.load_slots([(0.5 + torch.rand(mlp_step.NPARAM, generator=gen)).to(gpu) for _ in range(2)])
    for f in tr.ws.rowmajor_factors():  # the factors a wrongly taken apply would read
        f.fill_(0.25)
    slots = [s.clone() for s in tr.slots]
    p, step = tr.params.clone(), tr.global_step()
    _advance(tr, mode, 1)
    torch.cuda.synchronize()
    assert tr.pending and tr.global_step() == step + 1 and tr.ws.global_step() == step
    assert torch.equal(tr.params, p)  # the other buffer now: a pure copy
    for a, b in zip(tr.slots, slots):
        assert torch.equal(a, b)


# ---- 4. trajectories ---------------------------------------------------------------------------------
TRAJ_STEPS = 12
TRAJ_LR = {"momentum": 0.05, "adam": 1e-3}
TRAJ_EPS = 1e-3


def trajectory(kind, B, dtype):
    """12 steps on the CPU in ``dtype``: float64 -> reference_step + optim_reference (the
    oracle); float32 -> reference_step + gpu_ps_optim.apply_reference (the f32 yardstick)."""
    p, x, y = _data(B)
    lr = TRAJ_LR[kind]
    hyper = gpu_ps_optim.hyper_args(kind, epsilon=TRAJ_EPS)
    p, x = p.to(dtype), x.to(dtype)
    slots = [torch.zeros_like(p) for _ in range(gpu_ps_optim.num_slots(kind))]
    for s in range(TRAJ_STEPS):
        sl = slice((s % NB) * B, (s % NB + 1) * B)
        g, _, _ = mlp_step.reference_step(p, x[sl], y[sl])
        if dtype == torch.float64 and kind == "momentum":
            p, buf = oref.sgd_step(p, g, lr, mu=0.9, buf=slots[0])
            slots = [buf]
        elif dtype == torch.float64:
            p, m, v = oref.adam_step(p, g, slots[0], slots[1], lr, s + 1, eps=TRAJ_EPS, wd=0.0,
                                     adamw=False)
            slots = [m, v]
        else:
            pn, sn = gpu_ps_optim.apply_reference(kind, p.numpy(), g.numpy(),
                                                  [t.numpy() for t in slots], lr, s + 1, hyper)
            p, slots = torch.from_numpy(pn), [torch.from_numpy(t) for t in sn]
    return p


# max |p_f32 - p_f64| of the two CPU trajectories above after 12 steps (measured once on the CPU)
CPU_GAP = {
    ("momentum", 1): 9.832e-08, ("momentum", 17): 1.073e-07, ("momentum", 100): 8.817e-08,
    ("momentum", 113): 9.010e-08, ("momentum", 256): 8.949e-08,
    ("adam", 1): 8.185e-08, ("adam", 17): 8.670e-08, ("adam", 100): 1.008e-07,
    ("adam", 113): 9.356e-08, ("adam", 256): 1.050e-07,
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
@pytest.mark.parametrize("kind", ["momentum", "adam"])
@pytest.mark.parametrize("B", SIZES)
def test_trajectory_matches_float64(gpu, traj64, B, kind):
    """12 steps of momentum (lr 0.05, mu 0.9) and Adam (lr 1e-3, epsilon 1e-3: at 1e-8 an
    element whose gradient is below its own f32 rounding error moves by +-lr either way) through
    step(), run() and run_launched(flush=True) against the float64 trajectory.

    Tolerance: 4 x CPU_GAP, the distance between that float64 trajectory and the f32 CPU one
    (reference_step in f32 + gpu_ps_optim.apply_reference) -- the MFMA's summation order is not
    the CPU's.  Measured gaps: 0.82e-7 .. 1.07e-7 over the ten (kind, B) cases (the table
    above), so the tolerances are 3.3e-7 .. 4.3e-7 on parameters of magnitude <= 0.5.  The three ways of running agree with each other as the sgd test asks
    (test_kernels_gpu.py: parameters 1e-5, loss 1e-4, accuracy equal)."""
    ref = traj64(kind, B)
    tol = traj_tol(kind, B)
    runs = []
    for mode in ("step", "graph", "launched"):
        tr = _trainer(gpu, B, TRAJ_LR[kind], optimizer=kind, epsilon=TRAJ_EPS)
        if mode == "launched":
            tr.run_launched(TRAJ_STEPS, flush=True)
        else:
            _advance(tr, mode, TRAJ_STEPS)
            tr.flush()
        torch.cuda.synchronize()
        assert tr.global_step() == TRAJ_STEPS
        err = (tr.params.double().cpu() - ref).abs().max().item()
        print("trajectory", kind, "B", B, mode, "max |p - p64| %.3e" % err, "tol %.3e" % tol)
        runs.append((tr.params.clone(), tr.stats(), tr.stats_range(0, TRAJ_STEPS), err))
    for p, st, sr, err in runs:
        assert err <= tol
        assert (p - runs[0][0]).abs().max().item() < 1e-5
        assert abs(st[0] - runs[0][1][0]) < 1e-4 and st[1] == runs[0][1][1]
        assert torch.allclose(sr, runs[0][2], atol=1e-4)


# ---- 5. graph replay across reshuffled epochs -----------------------------------------------------
@pytest.mark.gpu
def test_adam_graph_replay_across_shuffled_epochs_is_eager(gpu):
    B = 100
    data = _data(B, nb=4, extra=7)  # 4 batches + a dropped tail; 10 steps = 2.5 epochs
    out = []
    for use_graph in (True, False):
        tr = _trainer(gpu, B, 1e-3, data, optimizer="adam", shuffle=True, shuffle_seed=5)
        tr.max_graph_steps = 3
        tr.run(10, use_graph=use_graph)
        tr.flush()
        torch.cuda.synchronize()
        assert tr.global_step() == 10
        out.append((tr.params.clone(), [s.clone() for s in tr.slots], tr.stats_range(0, 10)))
    assert torch.equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a, b)
    assert torch.equal(out[0][2], out[1][2])
    assert out[0][1][1].abs().max().item() > 0


# ---- 6. the all-reduce engine on one GPU ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_allreduce_engine_matches_single_gpu(gpu, kind):
    """world_size = 2 with an ``allreduce`` that doubles the gradient in place (two identical
    replicas): scale_(1/2) + ops.optim's kernels give the single-GPU trainer's trajectory within
    test 4's tolerance (eager and graph replay), and snapshot() / evaluate() move neither the
    parameters nor the slots."""
    B = 100
    kw = dict(optimizer=kind, epsilon=TRAJ_EPS)
    one = _trainer(gpu, B, TRAJ_LR[kind], **kw)
    one.run(TRAJ_STEPS)
    one.flush()
    for use_graph in (False, True):
        dp = _trainer(gpu, B, TRAJ_LR[kind], allreduce=lambda g: g.mul_(2.0), world_size=2, **kw)
        assert not dp.pipelined
        dp.max_graph_steps = 3
        dp.run(TRAJ_STEPS, use_graph=use_graph)
        assert dp.pending
        p, slots = dp.params.clone(), [s.clone() for s in dp.slots]
        snap, ssnap = dp.snapshot(with_slots=True)
        assert torch.equal(dp.snapshot(), snap)
        ev = dp.evaluate(dp.x, dp.labels)  # (on snapshot(): the pending gradient on a copy)
        assert dp.pending and torch.equal(dp.params, p)
        for a, b in zip(dp.slots, slots):
            assert torch.equal(a, b)
        dp.flush()
        torch.cuda.synchronize()
        assert dp.global_step() == TRAJ_STEPS
        assert torch.equal(dp.params, snap)
        for a, b in zip(dp.slots, ssnap):
            assert torch.equal(a, b)
        ev2 = dp.evaluate(dp.x, dp.labels)
        assert (float(ev.accuracy), float(ev.loss)) == (float(ev2.accuracy), float(ev2.loss))
        err = (dp.params - one.params).abs().max().item()
        print("all-reduce engine", kind, "graph" if use_graph else "eager", "%.3e" % err)
        assert err <= traj_tol(kind, B)


# ---- 7. refusals --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_unsupported_combinations_raise_before_any_launch(gpu):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = (t.to(gpu) for t in _data(100))
    comm = object()  # never touched: the constructor refuses first
    with pytest.raises(ValueError, match="optimizer adam"):
        FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, fused_comm=comm, optimizer="adam")
    with pytest.raises(ValueError, match="optimizer momentum"):
        FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, factor_comm=comm,
                        x_all=torch.stack([x, x]), optimizer="momentum")
    with pytest.raises(ValueError, match="pipeline=False"):
        FusedMLPTrainer(p, x, y, 100, 0.1, pipeline=False, optimizer="adam")
    with pytest.raises(ValueError, match="--optimizer must be one of"):
        FusedMLPTrainer(p, x, y, 100, 0.1, optimizer="adagrad")
    tr = FusedMLPTrainer(p, x, y, 100, 0.1, optimizer="momentum")
    assert not tr.persistent_ok
    with pytest.raises(RuntimeError, match="run_persistent"):
        tr.run_persistent(4)
    torch.cuda.synchronize()
    assert tr.global_step() == 0 and torch.equal(tr.params, p)
    assert FusedMLPTrainer(p, x, y, 100, 0.1).persistent_ok  # (sgd: unchanged)


# ---- 8. checkpoints --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_adam_checkpoint_round_trip_through_the_mirrored_loop(gpu, tmp_path, monkeypatch):
    """5 Adam steps, the chief's checkpoint, a fresh process-like restart to 10: the bits of an
    uninterrupted 10-step run.  The checkpoint holds the slot variables in TF layout; an sgd
    run restores it (ignoring them) and the eval job reads it."""
    from distributedtensorflowexample_amd.data.mnist import DataSet, DataSets
    from distributedtensorflowexample_amd.train.eval_job import eval_job
    from distributedtensorflowexample_amd.train.mirrored_mlp import train_mirrored
    from distributedtensorflowexample_amd.train.saver import latest_checkpoint, load_checkpoint

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    B = 100
    _, x, y = _data(B, extra=7)
    x, y = x.numpy(), y.numpy().astype(np.uint8)
    test = DataSet(x[:64], y[:64], one_hot=False)
    ds = DataSets(train=DataSet(x, y, one_hot=False), validation=test, test=test,
                  synthetic_train=True)

    def run(tag, steps, **kw):
        fl = types.SimpleNamespace(batch_size=B, learning_rate=1e-3, training_steps=steps,
                                   logdir=str(tmp_path / tag), log_every=5, eval_every=10 ** 9,
                                   save_model_secs=1000.0, save_summaries_secs=1000.0,
                                   use_locking=False, seed=0, device="cuda", **kw)
        return train_mirrored(fl, ds, log=lambda *_: None)

    _, full = run("full", 10, optimizer="adam")
    run("part", 5, optimizer="adam")
    v = load_checkpoint(latest_checkpoint(str(tmp_path / "part")))
    assert int(v["global/global_step"]) == 5
    for name in ("Adam", "Adam_1"):
        assert tuple(v["global/dense/kernel/" + name].shape) == (784, 100)
        assert tuple(v["global/dense_1/kernel/" + name].shape) == (100, 10)
        assert tuple(v["global/dense/bias/" + name].shape) == (100,)
        assert float(np.abs(np.asarray(v["global/dense_1/bias/" + name])).max()) > 0
    hist, cont = run("part", 10, optimizer="adam")
    assert [h[0] for h in hist] == [10]
    assert torch.equal(full, cont)
    hist, _ = run("part", 15)  # an sgd run restores the Adam checkpoint
    assert [h[0] for h in hist] == [15]
    lines = []
    fl = types.SimpleNamespace(logdir=str(tmp_path / "full"), device="auto", data_dir="",
                               eval_output="")
    assert eval_job(fl, log=lines.append) == 0
    assert lines[0] == "global_step: 10" and lines[1].startswith("test accuracy:")
