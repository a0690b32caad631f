"""Weight decay (L2, AdamW) and Nesterov momentum inside the fused two-launch MLP step
(``FusedMLPTrainer(weight_decay=, adamw=, nesterov=)``, ``mlp_lean_fwdapply_wd``): single applies
against float64 ``torch.optim`` fed the kernel's own gradient, coupled against decoupled decay
in the slots, the apply bit, float64 trajectories, composition with shuffle and dropout, the
all-reduce engine, the refusals, and ``weight_decay=0`` as the trainer there was.

Shapes as ``test_fused_optim_gpu.py``: 3 batches per dataset (``x_prev`` wraps), batch sizes 1, 17
(generic NGT = 0 tail), 100 (the NGT = 7 instantiation), 113 (the first size past it) and 256
(B > 128).  Inputs: ``weight_decay_reference`` (non-zero biases, wd 0.05, lr 0.3 / 0.01)."""
import os
import subprocess
import sys

import pytest
import torch

import optim_reference as oref
import weight_decay_reference as wr
from distributedtensorflowexample_amd.ops import lr_schedule, mlp_step
from distributedtensorflowexample_amd.ops._ext import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, NB, WD, LR, REGIONS = wr.SIZES, wr.NB, wr.WD, wr.LR, wr.REGIONS


def _trainer(gpu, B, lr, data=None, **kw):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = data if data is not None else wr.data(B)
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


def _kernel_gradient(oracle, p, step):
    """The exact f32 gradient the kernel forms at (p, batch ``step`` % nb): a mu = 0,
    weight_decay = 0 momentum apply leaves it in the slot plane (test_fused_optim_gpu.py, 1)."""
    oracle.load_params(p)
    oracle.seek(step)
    oracle.step()
    oracle.flush()
    return oracle.slots[0].clone()


def _bound1(ref):
    return oref.bound(1, ref)


# ---- 1. one apply against float64 on the kernel's own gradient ----------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sgd_l2", "momentum_l2", "nesterov", "nesterov_l2", "adam_l2",
                                  "adamw_t1", "adamw_t1001"])
@pytest.mark.parametrize("B", SIZES)
def test_apply_matches_float64_reference_on_kernel_gradient(gpu, B, case):
    """Three consecutive applies from non-zero slots -- two inside following steps' first launches
    (both buffer parities), the third by flush() (the apply-only instantiation) -- against
    torch.optim in float64 fed the kernel's own gradient: p and every slot within
    optim_reference.bound(k, ref) after k applies, W1, b1, W2 and b2 separately (wgrad_small is
    separate code; the region edges 78400, 78500, 79500 are where an index slip lands).  AdamW from
    global_step 0 and 1000: t = 1, 2, 3 and 1001, 1002, 1003.

    Condition, on the float64 references of the FIRST apply alone: the one with the term and the
    one without it (no decay; for Nesterov without decay, plain momentum) differ by >= 100 x the
    tolerance in each region.  It is asserted on p, except for adam with adamw=False, where it is
    asserted on m: there the decay enters p only through m / sqrt(v) -- d m = (1 - b1) wd p = 5e-4
    at |p| = 0.1, against sqrt(v) of ~0.25 and lr = 0.01 that is ~2e-6 on p, under 100 x 2.4e-7 --
    while m itself moves by 5e-4 against its own 2.4e-7."""
    name = case.split("_t")[0]
    kind, term = wr.CASES[name]
    gs = 1000 if case.endswith("t1001") else 0
    lr = LR[kind]
    data = wr.data(B)
    oracle = _trainer(gpu, B, lr, data, optimizer="momentum", momentum=0.0)
    tr = _trainer(gpu, B, lr, data, optimizer=kind, **term)
    s0 = wr.slots0(kind, B)
    tr.load_slots([s.to(gpu) for s in s0])
    tr.seek(gs)
    ref_p, ref_s = data[0].double(), [s.double() for s in s0]
    tr.step()
    for k in range(1, 4):
        assert tr.pending
        g = _kernel_gradient(oracle, tr.params.clone(), gs + k - 1).cpu()
        if k == 1:  # the reference alone
            without_p, without_s = wr.ref_apply(kind, ref_p, g, ref_s, lr, gs + 1,
                                                **wr.plain_terms(term))
            with_p, with_s = wr.ref_apply(kind, ref_p, g, ref_s, lr, gs + 1, **term)
            if name == "adam_l2":
                wr.assert_term_visible(case + " m", with_s[0], without_s[0], _bound1)
            else:
                wr.assert_term_visible(case + " p", with_p, without_p, _bound1)
        if k < 3:
            tr.step()   # applies update k (t = gs + k) in its first launch
        else:
            tr.flush()  # ... and the apply-only launch
        torch.cuda.synchronize()
        ref_p, ref_s = wr.ref_apply(kind, ref_p, g, ref_s, lr, gs + k, **term)
        oref.assert_close("p after %d" % k, tr.params, ref_p, k, REGIONS)
        assert len(tr.slots) == len(ref_s)
        for i, (s, r) in enumerate(zip(tr.slots, ref_s)):
            oref.assert_close("slot %d after %d" % (i, k), s, r, k, REGIONS)
    assert tr.global_step() == gs + 3


# ---- 2. coupled decay reaches the slots; decoupled decay does not -------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", SIZES)
def test_coupled_decay_is_in_the_slot_and_decoupled_is_not(gpu, B):
    data = wr.data(B)
    p0 = data[0].double()
    # momentum, mu = 0, wd > 0: the slot holds g + wd * p
    oracle = _trainer(gpu, B, LR["momentum"], data, optimizer="momentum", momentum=0.0)
    tm = _trainer(gpu, B, LR["momentum"], data, optimizer="momentum", momentum=0.0,
                  weight_decay=WD)
    g = _kernel_gradient(oracle, data[0].to(gpu), 0).double().cpu()
    tm.step()
    tm.flush()
    want = g + oref.f32(WD) * p0
    wr.assert_term_visible("slot", want, g, _bound1)
    oref.assert_close("slot = g + wd p", tm.slots[0], want, 1, REGIONS)
    # AdamW: m and v are the wd = 0 run's, bit for bit; the parameters are not
    s0 = wr.slots0("adam", B)
    out = []
    for wd in (0.0, WD):
        ta = _trainer(gpu, B, LR["adam"], data, optimizer="adam", weight_decay=wd, adamw=True)
        ta.load_slots([s.to(gpu) for s in s0])
        ta.step()
        ta.flush()
        torch.cuda.synchronize()
        out.append((ta.params.clone(), [s.clone() for s in ta.slots]))
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a, b)
    assert not torch.equal(out[0][0], out[1][0])


# ---- 3. the apply bit ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["step", "launched"])
@pytest.mark.parametrize("name", ["sgd_l2", "nesterov_l2", "adamw"])
@pytest.mark.parametrize("B", SIZES)
def test_nothing_pending_is_a_pure_copy(gpu, B, name, mode):
    """With wd = 0.05 the first step after construction, after load_params and after flush
    leaves the parameters bit-identical (in the other buffer) and no slot written: nothing
    decays while nothing is pending."""
    kind, term = wr.CASES[name]
    data = wr.data(B)
    tr = _trainer(gpu, B, LR[kind], data, optimizer=kind, **term)
    gen = torch.Generator().manual_seed(B)

    def check(p_want):
        for f in tr.ws.rowmajor_factors():  # the factors a wrongly taken apply would read
            f.fill_(0.25)
        tr.load_slots([(0.5 + torch.rand(mlp_step.NPARAM, generator=gen)).to(gpu)
                       for _ in tr.slots])
        slots = [s.clone() for s in tr.slots]
        step = tr.global_step()
        assert not tr.pending
        _advance(tr, mode, 1)
        torch.cuda.synchronize()
        assert tr.pending and tr.global_step() == step + 1 and tr.ws.global_step() == step
        assert torch.equal(tr.params, p_want)
        for a, b in zip(tr.slots, slots):
            assert torch.equal(a, b)

    check(data[0].to(gpu))            # after construction
    q = (data[0] + 0.01).to(gpu)
    tr.load_params(q)                 # drops the pending update
    check(q)
    _advance(tr, mode, 1)
    tr.flush()
    check(tr.params.clone())          # after flush


# ---- 4. trajectories ----------------------------------------------------------------------------
def _traj_trainer(gpu, B, case, **kw):
    kind, term, sched = wr.TRAJ[case]
    return _trainer(gpu, B, LR[kind], optimizer=kind, epsilon=wr.TRAJ_EPS, lr_schedule=sched,
                    **term, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(wr.TRAJ))
@pytest.mark.parametrize("B", SIZES)
def test_trajectory_matches_float64(gpu, B, case):
    """12 steps of sgd + L2 (lr 0.3), Nesterov + L2 (lr 0.3, mu 0.9) and AdamW (lr 0.01, epsilon
    1e-3, exponential decay 0.5 per 4 steps with a 3-step warm-up) through step(), run() with
    max_graph_steps = 3 and run_launched(flush=True) against the float64 trajectory.

    Tolerance: 4 x the distance between that float64 trajectory and the f32 CPU one
    (reference_step in f32 + ops.optim's CPU branches), computed here by weight_decay_reference.traj
    -- the margin test_fused_optim_gpu.py takes, for the same reason (the MFMA's summation order is
    not the CPU's).  Measured CPU gaps over the five batch sizes (they move by a few 1e-8 with the
    host's BLAS; the test prints its own): 1.0e-7 .. 6.3e-7 (sgd + L2), 0.8e-7 .. 2.1e-7 (Nesterov
    + L2; 2.1e-5 .. 2.3e-5 at batch 1, where a single row at lr 0.3 with mu 0.9 amplifies every
    rounding) and 1.2e-7 .. 1.4e-7 (AdamW); the GPU's own distance was 0.7e-7 .. 1.8e-7, at
    batch 1 5.4e-7 (sgd + L2) and 2.9e-5 (Nesterov + L2).  The condition: the float64
    trajectory without the term differs by >= 100 x the tolerance in every region.  The three
    ways of running agree with each other as that file's test 4 asks."""
    ref, tol, gap = wr.traj(case, B)
    kind, term, sched = wr.TRAJ[case]
    plain = "_plain_" + case
    wr.TRAJ[plain] = (kind, wr.plain_terms(term), sched)
    try:
        without, _ = wr.trajectory(plain, B, torch.float64)
    finally:
        del wr.TRAJ[plain]
    wr.assert_term_visible(case, ref, without, lambda r: tol)
    runs = []
    for mode in ("step", "graph", "launched"):
        tr = _traj_trainer(gpu, B, case)
        if mode == "launched":
            tr.run_launched(wr.TRAJ_STEPS, flush=True)
        else:
            _advance(tr, mode, wr.TRAJ_STEPS)
            tr.flush()
        torch.cuda.synchronize()
        assert tr.global_step() == wr.TRAJ_STEPS
        err = (tr.params.double().cpu() - ref).abs().max().item()
        print("trajectory", case, "B", B, mode, "max |p - p64| %.3e" % err, "tol %.3e" % tol,
              "cpu gap %.3e" % gap)
        runs.append((tr.params.clone(), tr.stats(), tr.stats_range(0, wr.TRAJ_STEPS), err))
    for p, st, sr, err in runs:
        assert err <= tol
        assert (p - runs[0][0]).abs().max().item() < 1e-5
        assert abs(st[0] - runs[0][1][0]) < 1e-4 and st[1] == runs[0][1][1]
        assert torch.allclose(sr, runs[0][2], atol=1e-4)


# ---- 5. composition ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_adamw_shuffle_dropout_graph_replay_is_eager(gpu):
    B = 100
    data = wr.data(B, nb=4, extra=7)  # 4 batches + a dropped tail; 10 steps = 2.5 epochs
    out = []
    for use_graph in (True, False):
        tr = _trainer(gpu, B, LR["adam"], data, optimizer="adam", weight_decay=WD, adamw=True,
                      shuffle=True, shuffle_seed=5, dropout=0.5, dropout_seed=3)
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


# ---- 6. the all-reduce engine --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(wr.TRAJ))
def test_allreduce_engine_matches_single_gpu(gpu, case):
    """world_size = 1 with an identity ``allreduce``: ops.optim's kernels with the same terms give
    the single-GPU trainer's trajectory within test 4's tolerance (eager and graph replay), and
    snapshot() / evaluate() move neither the parameters nor the slots."""
    B = 100
    _, tol, _ = wr.traj(case, B)
    one = _traj_trainer(gpu, B, case)
    one.run(wr.TRAJ_STEPS)
    one.flush()
    for use_graph in (False, True):
        dp = _traj_trainer(gpu, B, case, allreduce=lambda g: g, world_size=1)
        assert not dp.pipelined
        dp.max_graph_steps = 3
        dp.run(wr.TRAJ_STEPS, use_graph=use_graph)
        assert dp.pending
        p, slots = dp.params.clone(), [s.clone() for s in dp.slots]
        snap, ssnap = dp.snapshot(with_slots=True)
        assert torch.equal(dp.snapshot(), snap) and not torch.equal(snap, p)
        ev = dp.evaluate(dp.x, dp.labels)  # (on snapshot(): the pending gradient on a copy)
        assert dp.pending and torch.equal(dp.params, p)
        for a, b in zip(dp.slots, slots):
            assert torch.equal(a, b)
        dp.flush()
        torch.cuda.synchronize()
        assert dp.global_step() == wr.TRAJ_STEPS
        assert torch.equal(dp.params, snap)
        for a, b in zip(dp.slots, ssnap):
            assert torch.equal(a, b)
        ev2 = dp.evaluate(dp.x, dp.labels)
        assert (float(ev.accuracy), float(ev.loss)) == (float(ev2.accuracy), float(ev2.loss))
        err = (dp.params - one.params).abs().max().item()
        print("all-reduce engine", case, "graph" if use_graph else "eager", "%.3e" % err,
              "tol %.3e" % tol)
        assert err <= tol


# ---- 7. refusals ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_unsupported_combinations_raise_before_any_launch(gpu):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = (t.to(gpu) for t in wr.data(100))
    comm = object()  # never touched: the constructor refuses first
    for kw in (dict(weight_decay=WD), dict(optimizer="momentum", nesterov=True)):
        with pytest.raises(ValueError, match="exchange engines.*all-reduce engine"):
            FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, fused_comm=comm, **kw)
        with pytest.raises(ValueError, match="exchange engines.*all-reduce engine"):
            FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, factor_comm=comm,
                            x_all=torch.stack([x, x]), **kw)
        with pytest.raises(ValueError, match=r"pipeline=False.*two-launch step"):
            FusedMLPTrainer(p, x, y, 100, 0.1, pipeline=False, **kw)
    for bad in (-0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight_decay must be finite and >= 0"):
            FusedMLPTrainer(p, x, y, 100, 0.1, weight_decay=bad)
    for kind in ("sgd", "adam"):
        with pytest.raises(ValueError, match="nesterov needs optimizer momentum"):
            FusedMLPTrainer(p, x, y, 100, 0.1, optimizer=kind, nesterov=True)
    for kw in (dict(weight_decay=WD), dict(optimizer="momentum", nesterov=True),
               dict(optimizer="adam", weight_decay=WD)):
        tr = FusedMLPTrainer(p, x, y, 100, 0.1, **kw)
        assert not tr.persistent_ok
        with pytest.raises(ValueError, match="run_persistent.*no weight-decay"):
            tr.run_persistent(4)
        old = hip().mlp_set_flush_fused(1)  # DTFX_MLP_FLUSH_FUSED, selected in-process
        try:
            with pytest.raises(ValueError, match="fused flush.*no weight-decay"):
                tr.run_launched(4, flush=True)
        finally:
            hip().mlp_set_flush_fused(old)
        torch.cuda.synchronize()
        assert tr.global_step() == 0 and not tr.pending and torch.equal(tr.params, p)
    assert FusedMLPTrainer(p, x, y, 100, 0.1).persistent_ok  # (no terms: unchanged)


KS14_SCRIPT = """
import torch
from distributedtensorflowexample_amd.ops import mlp_step
from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer
p = torch.zeros(mlp_step.NPARAM, device="cuda")
x = torch.zeros(300, 784, device="cuda")
y = torch.zeros(300, dtype=torch.int32, device="cuda")
try:
    FusedMLPTrainer(p, x, y, 100, 0.1, weight_decay=0.05)
except ValueError as e:
    print("REFUSED", e)
"""


@pytest.mark.gpu
def test_ks14_refuses_weight_decay(gpu):
    """DTFX_MLP_KS is read once per process, so this refusal is shown in a child process."""
    env = dict(os.environ, DTFX_MLP_KS="14")
    r = subprocess.run([sys.executable, "-c", KS14_SCRIPT], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "REFUSED weight_decay / nesterov: DTFX_MLP_KS=14" in r.stdout, r.stdout + r.stderr


# ---- 8. weight_decay = 0, nesterov = False is the trainer there was -----------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam"])
@pytest.mark.parametrize("B", [17, 100])
def test_zero_decay_is_bit_identical_to_no_arguments(gpu, B, kind):
    data = wr.data(B)
    sched = lr_schedule.LRSchedule("exponential", 4, 0.5, False, 3)
    for extra in ({}, dict(lr_schedule=sched)):
        a = _trainer(gpu, B, LR[kind], data, optimizer=kind, **extra)
        b = _trainer(gpu, B, LR[kind], data, optimizer=kind, weight_decay=0.0, adamw=False,
                     nesterov=False, **extra)
        assert b.decay is None and (b.opt is None) == (a.opt is None)
        for tr in (a, b):
            tr.max_graph_steps = 3
            tr.step()
            tr.run(4)
            tr.run_launched(3, flush=True)
        torch.cuda.synchronize()
        assert a.global_step() == b.global_step() == 8
        assert torch.equal(a.params, b.params)
        assert len(a.slots) == len(b.slots)
        for s, t in zip(a.slots, b.slots):
            assert torch.equal(s, t)
        assert torch.equal(a.stats_range(0, 8), b.stats_range(0, 8))
