"""Moving average of the parameters inside the fused two-launch MLP step
(``FusedMLPTrainer(ema_decay=, ema_num_updates=)``, ``mlp_lean_fwdapply_ema``, ``ops.optim.ema_``):
single shadow updates against float64 fed the kernel's own inputs, no feedback into training, the
apply bit and the plane's edges, the run modes, ``seek``, the all-reduce engine, ``evaluate`` and
the refusals.

Shapes as ``test_fused_weight_decay_gpu.py``: 3 batches per dataset (``x_prev`` wraps), batch sizes
1, 17 (generic NGT = 0 tail), 100 (the NGT = 7 instantiation), 113 (the first size past it) and 256
(B > 128).  Inputs: ``ema_reference`` (decay 0.99, a starting shadow ~0.1 from the parameters)."""
import os
import subprocess
import sys

import pytest
import torch

import ema_reference as er
import optim_reference as oref
from distributedtensorflowexample_amd.ops import mlp_step, optim
from distributedtensorflowexample_amd.ops._ext import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, LR, REGIONS, DECAY = er.SIZES, er.LR, er.REGIONS, er.DECAY


def _trainer(gpu, B, lr, data=None, **kw):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = data if data is not None else er.data(B)
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


# ---- 1. one update at a time ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nu", [False, True])
@pytest.mark.parametrize("case", list(er.CASES))
@pytest.mark.parametrize("B", SIZES)
def test_shadow_update_matches_float64_on_kernel_inputs(gpu, B, case, nu):
    """From ``global_step`` 0 and 1000: three applies -- two inside following steps' first
    launches (both buffer parities), the third by flush() (the apply-only instantiation).  After
    each, the reference is ``ref_update`` fed the kernel's own previous shadow and the kernel's own
    new ``params`` (exact f32 inputs: only the shadow arithmetic is under test), W1, b1, W2 and b2
    separately, within ``optim_reference.bound(1, ref)`` = 2 ulp at max(1, |ref|): the expression
    rounds ``e - v``, the product and the difference, at most 1.5 ulp in total.  With
    ``num_updates`` the reference's coefficient is ``one_minus_decay_f32(t)``; the kernel's
    ``9 / (10 + t)`` is a correctly rounded division, not v_rcp_f32, so nothing is added."""
    kind, term = er.CASES[case]
    data = er.data(B)
    for gs in er.STARTS:
        tr = _trainer(gpu, B, LR[kind], data, optimizer=kind, ema_decay=DECAY, ema_num_updates=nu,
                      **term)
        tr.load_ema(er.shadow0(B).to(gpu))
        tr.seek(gs)
        tr.step()
        for k in range(1, 4):
            assert tr.pending
            prev = tr.ema.clone()
            if k < 3:
                tr.step()   # applies update k (t = gs + k) in its first launch
            else:
                tr.flush()  # ... and the apply-only launch
            torch.cuda.synchronize()
            ref = er.ref_update(prev, tr.params, gs + k, DECAY, nu)
            if k == 1:
                er.assert_visible("%s gs %d" % (case, gs), ref, prev)
            err = float((tr.ema.cpu().double() - ref).abs().max())
            print("B", B, case, "nu", nu, "gs", gs, "apply", k, "max error %.3e" % err)
            oref.assert_close("shadow, gs %d apply %d" % (gs, k), tr.ema, ref, 1, REGIONS)
        assert tr.global_step() == gs + 3


# ---- 2. the shadow does not perturb training ----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(er.NO_FEEDBACK))
@pytest.mark.parametrize("B", [17, 100])
def test_parameters_and_slots_are_those_of_ema_decay_zero(gpu, B, case):
    """7 steps + flush: ``params``, every slot and the recorded stats are bit-identical to the
    same trainer with ``ema_decay=0`` (which launches the kernels there were: no shadow, and for
    plain sgd no optimizer object at all).  Without decay the moving-average family runs the
    weight-decay block with the coefficients (0, 0, 0, 1); this is the test that they reproduce
    the non-decay kernels."""
    kind, term = er.NO_FEEDBACK[case]
    data = er.data(B)
    out = []
    for decay in (0.0, DECAY):
        tr = _trainer(gpu, B, LR[kind], data, optimizer=kind, ema_decay=decay,
                      ema_num_updates=decay > 0, **term)
        if decay == 0.0:
            assert tr.avg is None and (tr.opt is None) == (case == "sgd")
        tr.max_graph_steps = 3
        tr.step()
        tr.run(3)
        tr.run_launched(3, flush=True)
        torch.cuda.synchronize()
        assert tr.global_step() == 7
        out.append((tr.params.clone(), [s.clone() for s in tr.slots], tr.stats_range(0, 7)))
    assert torch.equal(out[0][0], out[1][0])
    assert len(out[0][1]) == len(out[1][1])
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a, b)
    assert torch.equal(out[0][2], out[1][2])


# ---- 3. apply == 0 and the padding ---------------------------------------------------------------
GUARD = 64
EDGES = [0, 78399, 78400, 78499, 78500, 79499, 79500, 79509]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("B", SIZES)
def test_nothing_pending_and_the_plane_edges(gpu, B, kind):
    """The first step of a fresh trainer (nothing to apply) leaves the shadow bit-identical; a
    shadow allocation with 64 guard floats of a NaN pattern on both sides keeps them through
    three applies, and the plane has moved up to both sides of every region edge (78400 / 78500 /
    79500 / 79510: ``test_ema_cpu.py`` shows the starting shadow at least 1e-4 from the parameters
    there, a motion of >= 1e-6 per update) and all but a handful of elements whose distance from the parameters rounds away."""
    n = mlp_step.NPARAM
    tr = _trainer(gpu, B, LR[kind], optimizer=kind, ema_decay=DECAY)
    assert torch.equal(tr.ema, tr.params)  # shadow_0: the initial parameters
    big = torch.full((n + 2 * GUARD,), float("nan"), device=gpu)
    big.view(torch.int32).fill_(0x7FC0BEEF)
    pattern = big.view(torch.int32).clone()
    tr.opt.shadow = big[GUARD:GUARD + n]
    assert tr.opt.shadow.data_ptr() % 16 == 0
    s0 = er.shadow0(B).to(gpu)
    tr.load_ema(s0)
    tr.step()
    torch.cuda.synchronize()
    assert torch.equal(tr.ema, s0)
    tr.step()
    tr.step()
    tr.flush()
    torch.cuda.synchronize()
    got = big.view(torch.int32)
    assert torch.equal(got[:GUARD], pattern[:GUARD]) and torch.equal(got[-GUARD:], pattern[-GUARD:])
    assert bool(torch.isfinite(tr.ema).all())
    moved = tr.ema != s0
    assert bool(moved[torch.tensor(EDGES, device=gpu)].all())
    assert int(moved.sum()) >= n - 16


# ---- 4. modes agree ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("case", ["sgd", "adam", "adam_sched"])
def test_step_graph_and_host_loop_give_the_same_shadow(gpu, case, shuffle):
    """7 steps through ``step()``, graph replay and the C++ host loop give ``torch.equal`` shadows,
    parameters and (``adam_sched``) rate rings.  ``snapshot(with_ema=True)`` in the ``step`` run
    equals ``ema`` after ``flush()`` and does not move ``global_step()``.  On one GPU the snapshot
    IS the flush (``snapshot``'s rule), so the shadow is the trainer's own afterwards; of the rate
    ring it may write nothing but the pending step's entry, with the value the flush of the other
    two runs writes: the entries of steps 0..5 are bit-identical across it, and the whole ring
    equals the ``graph`` / ``launched`` runs', which never took a snapshot."""
    kind, term = er.CASES[case]
    B = 100
    data = er.data(B, nb=4, extra=7)  # 7 steps cross an epoch boundary
    out = []
    for mode in ("step", "graph", "launched"):
        tr = _trainer(gpu, B, LR[kind], data, optimizer=kind, ema_decay=DECAY,
                      ema_num_updates=True, shuffle=shuffle, shuffle_seed=5, **term)
        tr.load_ema(er.shadow0(B).to(gpu))
        _advance(tr, mode, 7)
        assert tr.pending and tr.global_step() == 7
        if mode == "step":  # snapshot(with_ema=True): the shadow after every step run so far
            rates = tr.opt.rates.clone() if tr.sched is not None else None
            p, sh = tr.snapshot(with_ema=True)
            assert tr.global_step() == 7
            p2, sl, sh2 = tr.snapshot(with_slots=True, with_ema=True)
            assert torch.equal(sh, sh2) and torch.equal(p, p2) and len(sl) == len(tr.slots)
            if rates is not None:  # steps 0..5 were recorded before; step 6 is the pending one
                assert torch.equal(tr.opt.rates[:6], rates[:6])
                assert torch.equal(tr.opt.rates[7:], rates[7:])
                assert bool((rates[:6] > 0).all()) and float(rates[6]) == 0.0
        tr.flush()
        torch.cuda.synchronize()
        if mode == "step":
            assert torch.equal(sh, tr.ema) and torch.equal(p, tr.params)
            assert sh.data_ptr() != tr.ema.data_ptr()
        assert tr.global_step() == 7
        ring = tr.opt.rates.clone() if tr.sched is not None else torch.zeros(0, device=gpu)
        out.append((tr.ema.clone(), tr.params.clone(), ring))
    for sh, p, ring in out[1:]:
        assert torch.equal(sh, out[0][0]) and torch.equal(p, out[0][1])
        assert torch.equal(ring, out[0][2])
    if case == "adam_sched":
        want = torch.tensor([float(er.SCHED.value_f32(LR[kind], s)) for s in range(7)])
        assert torch.equal(out[0][2][:7].cpu(), want)
    assert not torch.equal(out[0][0], er.shadow0(B).to(gpu))


# ---- 5. seek resumes -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_seek_round_trip_resumes_bit_for_bit(gpu, kind):
    """With ``num_updates`` (d_t depends on the step word): 4 steps, the state carried into a new
    trainer by load_params / load_slots / load_ema / seek, 3 more steps == 7 uninterrupted steps.
    ``seek`` itself leaves the shadow alone."""
    B = 100
    data = er.data(B)
    kw = dict(optimizer=kind, ema_decay=DECAY, ema_num_updates=True)
    whole = _trainer(gpu, B, LR[kind], data, **kw)
    for _ in range(7):
        whole.step()
    whole.flush()
    a = _trainer(gpu, B, LR[kind], data, **kw)
    for _ in range(4):
        a.step()
    p, slots, sh = a.snapshot(with_slots=True, with_ema=True)
    b = _trainer(gpu, B, LR[kind], data, **kw)
    b.load_params(p)
    b.load_slots(slots)
    b.load_ema(sh)
    b.seek(a.global_step())
    assert torch.equal(b.ema, sh)
    for _ in range(3):
        b.step()
    b.flush()
    torch.cuda.synchronize()
    assert b.global_step() == whole.global_step() == 7
    assert torch.equal(b.params, whole.params)
    assert torch.equal(b.ema, whole.ema)


# ---- 6. the all-reduce engine --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nu", [False, True])
@pytest.mark.parametrize("case", ["sgd", "adam", "adam_sched"])
def test_allreduce_engine_shadow(gpu, case, nu):
    """world_size = 1 with an identity ``allreduce``: ``ops.optim.ema_`` after the optimizer.  The
    shadow after k = 3 applies against the reference iterated in float64 on the engine's own
    parameters, within ``bound(k, ref)``; ``snapshot(with_ema=True)`` with a pending gradient
    equals the shadow after the later flush and moves nothing of the trainer's: parameters,
    shadow, ``global_step()`` and, with a schedule, the rate ring (the pending step's rate is
    computed for the copies without being published; the later flush publishes it)."""
    kind, term = er.CASES[case]
    B = 100
    dp = _trainer(gpu, B, LR[kind], optimizer=kind, ema_decay=DECAY, ema_num_updates=nu,
                  allreduce=lambda g: g, world_size=1, **term)
    assert not dp.pipelined
    s0 = er.shadow0(B)
    dp.load_ema(s0.to(gpu))
    ref = s0.double()
    dp.step()
    for k in range(1, 4):
        assert dp.pending
        if k < 3:
            dp.step()
        else:
            p, sh, gs = dp.params.clone(), dp.ema.clone(), dp.global_step()
            rates = dp.opt.rates.clone() if dp.sched is not None else None
            snap_p, snap_sh = dp.snapshot(with_ema=True)
            assert torch.equal(dp.params, p) and torch.equal(dp.ema, sh) and dp.pending
            assert dp.global_step() == gs
            if rates is not None:
                torch.cuda.synchronize()
                assert torch.equal(dp.opt.rates, rates)
                assert bool((rates[:2] > 0).all()) and float(rates[2]) == 0.0
            dp.flush()
            if rates is not None:  # ... and the flush records the step's rate
                assert float(dp.opt.rates[2]) == float(er.SCHED.value_f32(LR[kind], 2))
        torch.cuda.synchronize()
        new = er.ref_update(ref, dp.params, k, DECAY, nu)
        if k == 1:
            er.assert_visible("all-reduce %s" % case, new, ref)
        ref = new
    assert torch.equal(dp.params, snap_p) and torch.equal(dp.ema, snap_sh)
    oref.assert_close("shadow after 3", dp.ema, ref, 3, REGIONS)
    assert dp.global_step() == 3


# ---- 7. evaluate(ema=True) -----------------------------------------------------------------------
@pytest.mark.gpu
def test_evaluate_ema_evaluates_the_shadow(gpu):
    """``evaluate(ema=True)`` is ``ops.mlp_eval.evaluate`` of the shadow, and the float64 CPU
    reference says it must differ from ``evaluate()``: the shadow starts 0.5 per element from the
    parameters, and after two steps the float64 losses of the trainer's own shadow and parameters
    are >= 100 x the eval kernel's loss tolerance apart (``test_mlp_eval_gpu.py``: 1e-4 relative)."""
    from distributedtensorflowexample_amd.ops import mlp_eval

    B = 100
    p, x, y = er.data(B)
    far = p + 5.0 * (er.shadow0(B) - p)

    def loss64(q):
        _, logits = mlp_step.reference_forward(q.cpu().double(), x.double())
        return float((torch.logsumexp(logits, 1)
                      - logits.gather(1, y.long()[:, None])[:, 0]).mean())

    def loss_tol(ref):
        return 1e-4 * max(1.0, abs(ref))

    tr = _trainer(gpu, B, LR["sgd"], (p, x, y), ema_decay=DECAY)
    tr.load_ema(far.to(gpu))
    tr.step()
    tr.step()
    gs = tr.global_step()
    ev = tr.evaluate(tr.x, tr.labels, ema=True)
    assert tr.global_step() == gs
    want = mlp_eval.evaluate(tr.ema, tr.x, tr.labels)
    raw = tr.evaluate(tr.x, tr.labels)
    ref_ema, ref_raw = loss64(tr.ema), loss64(tr.params)
    print("loss: shadow", float(ev.loss), "ref", ref_ema, "parameters", float(raw.loss), "ref",
          ref_raw)
    assert abs(ref_ema - ref_raw) >= 100 * loss_tol(ref_ema)
    assert (float(ev.loss), float(ev.accuracy)) == (float(want.loss), float(want.accuracy))
    assert abs(float(ev.loss) - ref_ema) <= loss_tol(ref_ema)
    assert abs(float(raw.loss) - ref_raw) <= loss_tol(ref_raw)
    plain = _trainer(gpu, B, LR["sgd"], (p, x, y))
    with pytest.raises(RuntimeError, match="keeps no moving average"):
        plain.evaluate(plain.x, plain.labels, ema=True)
    with pytest.raises(RuntimeError, match="keeps no moving average"):
        plain.ema


# ---- 8. refusals ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_unsupported_combinations_raise_before_any_launch(gpu):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = (t.to(gpu) for t in er.data(100))
    comm = object()  # never touched: the constructor refuses first
    kw = dict(ema_decay=DECAY)
    with pytest.raises(ValueError, match="exchange engines.*all-reduce engine"):
        FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, fused_comm=comm, **kw)
    with pytest.raises(ValueError, match="exchange engines.*all-reduce engine"):
        FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, factor_comm=comm,
                        x_all=torch.stack([x, x]), **kw)
    with pytest.raises(ValueError, match=r"pipeline=False.*two-launch step"):
        FusedMLPTrainer(p, x, y, 100, 0.1, pipeline=False, **kw)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"ema_decay must lie in \(0, 1\)"):
            FusedMLPTrainer(p, x, y, 100, 0.1, ema_decay=bad)
    for kind in ("sgd", "adam"):
        tr = FusedMLPTrainer(p, x, y, 100, 0.1, optimizer=kind, **kw)
        assert not tr.persistent_ok
        with pytest.raises(ValueError, match="run_persistent.*no moving average"):
            tr.run_persistent(4)
        old = hip().mlp_set_flush_fused(1)  # DTFX_MLP_FLUSH_FUSED, selected in-process
        try:
            with pytest.raises(ValueError, match="fused flush.*no moving-average"):
                tr.run_launched(4, flush=True)
        finally:
            hip().mlp_set_flush_fused(old)
        torch.cuda.synchronize()
        assert tr.global_step() == 0 and not tr.pending and torch.equal(tr.params, p)
        assert torch.equal(tr.ema, p)
    assert FusedMLPTrainer(p, x, y, 100, 0.1).persistent_ok  # (no moving average: unchanged)


@pytest.mark.gpu
def test_launcher_rejects_a_bad_shadow_plane_or_decay(gpu):
    """``check_opt``: a null or misaligned shadow plane and a decay outside (0, 1) throw before
    any launch."""
    B = 100
    tr = _trainer(gpu, B, 0.1, ema_decay=DECAY)
    good = tr.opt.shadow
    buf = torch.zeros(mlp_step.NPARAM + 4, device=gpu)
    tr.opt.shadow = buf[1:1 + mlp_step.NPARAM]
    with pytest.raises(RuntimeError, match="shadow plane must be 16-byte aligned"):
        tr.step()
    tr.opt.shadow = good
    args = list(tr.opt.ema_args())
    h, x = hip(), tr.x[:B]

    def launch(a):
        from distributedtensorflowexample_amd.ops._ext import ptr, stream_handle

        h.mlp_lean_fwdapply_ema(ptr(tr.bufs[0]), ptr(tr.bufs[1]), 0.1, ptr(x), ptr(x),
                                ptr(tr.ws.buf), ptr(tr.ws.ctr), ptr(tr.ws.stats),
                                tr.ws.stats_ring, B, 0, 0, *a, stream_handle())
    null = list(args)
    null[-3] = 0
    with pytest.raises(RuntimeError, match="null shadow plane"):
        launch(null)
    for omd in (0.0, 1.0, -0.5, float("nan")):
        bad = list(args)
        bad[-2] = omd
        with pytest.raises(RuntimeError, match=r"decay must lie in \(0, 1\)"):
            launch(bad)
    torch.cuda.synchronize()
    assert tr.global_step() == 0


CHILD_SCRIPT = """
import torch
from distributedtensorflowexample_amd.ops import mlp_step
from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer
p = torch.zeros(mlp_step.NPARAM, device="cuda")
x = torch.zeros(300, 784, device="cuda")
y = torch.zeros(300, dtype=torch.int32, device="cuda")
try:
    tr = FusedMLPTrainer(p, x, y, 100, 0.1, ema_decay=0.99)
    tr.run_launched(4, flush=True)
except ValueError as e:
    print("REFUSED", e)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("env,msg", [
    ({"DTFX_MLP_KS": "14"}, "REFUSED ema_decay: DTFX_MLP_KS=14"),
    ({"DTFX_MLP_FLUSH_FUSED": "1"}, "REFUSED ema_decay: the fused flush"),
])
def test_ks14_and_fused_flush_refuse_in_a_fresh_process(gpu, env, msg):
    """Both knobs are read once per process, so the refusals are shown in a child process."""
    r = subprocess.run([sys.executable, "-c", CHILD_SCRIPT], env=dict(os.environ, **env), cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert msg in r.stdout, r.stdout + r.stderr


# ---- 9. ops.optim.ema_ on the GPU ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nu", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 4097, 79510])
def test_optim_ema_kernel_matches_float64(gpu, n, nu):
    """The in-place dwordx4 kernel against float64: vector body, scalar tail, and a view one float
    off 16-byte alignment (the scalar loop alone); ``t`` as a constant and from the int32 device
    counter.  t = 3 takes the ``(1 + t) / (10 + t)`` side of the min(), t = 2000 the decay's."""
    gen = torch.Generator().manual_seed(n)
    e0, p = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    regions = [("all", torch.arange(n))]
    for t in (3, 2000):
        ref = er.ref_update(e0, p, t, DECAY, nu)
        assert float((ref - e0.double()).abs().max()) >= 100 * oref.bound(1, ref)
        for off in (0, 1):
            for counter in (False, True):
                base = torch.full((n + 8,), 7.0, device=gpu)
                pb = torch.zeros(n + 8, device=gpu)
                sh, pv = base[off:off + n], pb[off:off + n]
                sh.copy_(e0)
                pv.copy_(p)
                if counter:
                    ctr = torch.tensor([t], dtype=torch.int32, device=gpu)
                    optim.ema_(sh, pv, DECAY, nu, step_tensor=ctr)
                else:
                    optim.ema_(sh, pv, DECAY, nu, step=t)
                torch.cuda.synchronize()
                oref.assert_close("ema_ n %d t %d off %d" % (n, t, off), sh, ref, 1, regions)
                assert bool((base[:off] == 7.0).all()) and bool((base[off + n:] == 7.0).all())
                assert torch.equal(pv.cpu(), p)
