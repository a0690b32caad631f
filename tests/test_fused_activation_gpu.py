"""ReLU and tanh hidden activations inside the fused MLP step and the fused evaluation kernel
(``FusedMLPTrainer(activation=...)``, ``ops.mlp_eval.evaluate(.., activation=...)``,
``ops/hidden_act.py``): the head against float64, hbuf's padding and ReLU's exact zeros, the applied
gradient, one model through every way of running it, the default as today's trainer, the
evaluation kernel, the all-reduce engine, the refusals and the mirrored loop.

Data: ``dropout_reference.data`` (p = 0.1 randn with zero biases, x = rand, 3 batches so ``x_prev``
wraps); batch sizes 1, 17, 100 (the NGT = 7 kernels), 113 and 256; learning rate 0.01.

ReLU's kink.  The derivative is discontinuous at z1 = 0 and an f32 z1 a few ulps from the float64
one can sit on the other side, so the float64 reference takes the pattern of active units from
the GPU's own ``hbuf > 0`` (with dropout: active and kept) -- after the pattern has been asserted
equal to the reference's ``z1 > 0`` on every element with ``|z1| > 1e-4``.  The elements left out
may be at most 0.1 % of a case's B x 100; that cap is asserted on the float64 side first.  At the
initial parameters 0 / 1 / 0 / 0 / 3 of 300 / 5,100 / 30,000 / 33,900 / 76,800 are left out for
B = 1 / 17 / 100 / 113 / 256 (tests/test_activation_cpu.py).

Bounds.  For relu and tanh every bound is 4 x the gap between the float32 and the float64 CPU
evaluation of ``activation_reference.step`` on the same case (``activation_reference.gaps``: from
the reference alone), floored at the suite's sigmoid bound: per-row loss 1e-4, dl 1e-6, dz1 and
hbuf 1e-6 x the dropout scale, applied gradient 1e-4.  Every test prints gap, bound and error.
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import activation_reference as ar
import dropout_reference as dr
from distributedtensorflowexample_amd.ops import mlp_eval, mlp_step
from distributedtensorflowexample_amd.ops._ext import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, SEED, NB = dr.SIZES, dr.SEED, dr.NB
LR, STEPS, KS, HP = 0.01, 7, 28, mlp_step.HP
NEW = ("relu", "tanh")
FLOOR = dict(rowloss=1e-4, dl=1e-6, dz=1e-6, hd=1e-6, grad=1e-4, prob=1e-4)
KINK_SHARE = 0.001  # of B x 100: what a ReLU pattern comparison may leave out
_CASES = {}


def _bounds(gap, scale=1.0):
    """4 x the reference's f32 / f64 gap, floored at the sigmoid bound (dz1, hbuf: x the scale)."""
    return {k: max(4.0 * gap[k], FLOOR[k] * (scale if k in ("dz", "hd") else 1.0)) for k in FLOOR}


def _case(act, B, rate):
    """(inputs, float64 step, f32 / f64 gaps) of the first batch at the initial parameters, once,
    with the preconditions asserted before any GPU value is looked at."""
    key = (act, B, rate)
    if key not in _CASES:
        p, x, y = dr.data(B)
        xb, yb = x[:B], y[:B]
        keep = dr.keep_mask(SEED, 0, 0, B, rate) if rate else None
        scale = dr.threshold(rate)[1] if rate else 1.0
        ref = ar.step(p, xb, yb, act, keep, scale)
        near = int(ar.near_kink(ref["z1"]).sum())
        amb = int((ref["gap"] <= 1e-3).sum())
        gap = ar.gaps(p, xb, yb, act, keep, scale, ref=ref)
        print("float64 %s B=%d dropout %g: %d of %d units within 1e-4 of the kink, %d rows with a "
              "top-2 gap <= 1e-3, max h %.3f, f32/f64 gaps %s"
              % (act, B, rate, near, B * 100, amb, float(ref["h"].max()),
                 {k: "%.2e" % v for k, v in gap.items()}))
        assert near <= KINK_SHARE * B * 100
        assert amb <= 0.01 * B
        _CASES[key] = (p, xb, yb, keep, scale, ref, gap)
    return _CASES[key]


def _trainer(gpu, B, data=None, lr=LR, **kw):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = data if data is not None else dr.data(B)
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


def _views(ws, B):
    """(hbuf [BP, 112], dz1R, dlR, rowstat [BP, 2], dz1T [112, BP]) of a workspace."""
    BP = (B + 15) // 16 * 16
    dz, dl = ws.rowmajor_factors()
    hb = ws.buf[KS * BP * HP:(KS + 1) * BP * HP].view(BP, HP)
    dzt = ws.buf[(KS + 1) * BP * HP:(KS + 2) * BP * HP].view(HP, BP)
    rs = ws.buf[-4 - 2 * BP:-4].view(BP, 2)
    return hb, dz, dl, rs, dzt


def _gpu_pattern(hb, B, z1_ref, keep, tag):
    """The GPU's pattern of active (and kept) units, asserted equal to the reference's ``z1 > 0``
    (and kept) outside ``|z1| <= 1e-4``."""
    got = hb[:B, :100].cpu() > 0
    want = z1_ref > 0
    if keep is not None:
        want = want & keep
    sure = ~ar.near_kink(z1_ref)
    assert int((~sure).sum()) <= KINK_SHARE * B * 100, tag
    flips = int((got != want).sum())
    print(tag, "pattern: %d of %d units differ from the float64 one (%d within 1e-4 of the kink)"
          % (flips, B * 100, int((~sure).sum())))
    assert torch.equal(got[sure], want[sure]), tag
    return got


# ---- 1. the head against float64 ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lean", [True, False], ids=["lean", "three_launch"])
@pytest.mark.parametrize("rate", [0.0, 0.5])
@pytest.mark.parametrize("B", [17, 100])
@pytest.mark.parametrize("act", NEW)
def test_head_matches_float64(gpu, act, B, rate, lean):
    """hbuf, per-row loss, dl and dz1 of one step's head, lean and three-launch, plain and with
    dropout 0.5, within 4 x the reference's f32 / f64 gap (floored at the sigmoid bounds); accuracy
    on the rows whose float64 top-2 gap exceeds 1e-3 (at most 1 % are left out).

    Observed on the MI355X, largest over the 8 cases of an activation (gap / bound / error):
    hbuf relu 4.97e-6 / 6.9e-6 .. 2.0e-5 / 1.94e-6, tanh 3.68e-6 / 5.0e-6 .. 1.5e-5 / 1.57e-6;
    per-row loss relu 1.69e-6 / 1e-4 / 1.22e-6, tanh 9.1e-7 / 1e-4 / 6.6e-7; dl relu 1.5e-8 / 1e-6 /
    9.8e-9, tanh 9.4e-9 / 1e-6 / 9.0e-9; dz1 relu 8.3e-9 / 1e-6 x scale / 8.7e-9, tanh 1.3e-8 /
    1e-6 x scale / 9.9e-9: only hbuf's bound comes from the gap, the others are the sigmoid floors.
    ReLU's pattern equals the float64 one on every element (profiles/activation/README.md)."""
    p, xb, yb, keep, scale, ref, gap = _case(act, B, rate)
    kw = dict(activation=act, dropout=rate, dropout_seed=SEED)
    tr = _trainer(gpu, B, **kw, **({} if lean else {"pipeline": False}))
    tr.step()
    torch.cuda.synchronize()
    hb, dz, dl, rs, dzt = _views(tr.ws, B)
    tag = "%s B=%d dropout %g %s" % (act, B, rate, "lean" if lean else "three-launch")
    if act == "relu":
        active = _gpu_pattern(hb, B, ref["z1"], keep, tag)
        ref = ar.step(p, xb, yb, act, keep, scale, active=active)
    if lean:
        dz_g, dl_g = dz[:B, :100], dl[:B, :10]
    else:  # transposed factors: dz1T [112][BP], dlT [16][BP] behind it
        BP = dzt.shape[1]
        dlt = tr.ws.buf[(KS + 2) * BP * HP:(KS + 2) * BP * HP + 16 * BP].view(16, BP)
        dz_g, dl_g = dzt[:100, :B].t(), dlt[:10, :B].t()
    err = dict(hd=float((hb[:B, :100].double().cpu() - ref["hd"]).abs().max()),
               rowloss=float((rs[:B, 0].double().cpu() - ref["rowloss"]).abs().max()),
               dl=float((dl_g.double().cpu() - ref["dl"]).abs().max()),
               dz=float((dz_g.double().cpu() - ref["dz"]).abs().max()))
    bound = _bounds(gap, scale)
    for k in err:
        print("%s %s: gap %.3e bound %.3e error %.3e" % (tag, k, gap[k], bound[k], err[k]))
    for k in err:
        assert err[k] <= bound[k], (tag, k)
    clear = ref["gap"] > 1e-3
    assert torch.equal(rs[:B, 1].cpu()[clear] == 1.0, ref["correct"][clear])
    # (and it is this activation's head: the sigmoid h of the same z1 is far away)
    assert float((hb[:B, :100].double().cpu() - torch.sigmoid(ref["z1"])).abs().max()) > 0.1


# ---- 2. padding and ReLU's exact zeros ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lean", [True, False], ids=["lean", "three_launch"])
@pytest.mark.parametrize("B", [1, 17, 113])
@pytest.mark.parametrize("act", NEW)
def test_hbuf_padding_and_relu_zeros_are_exact(gpu, act, B, lean):
    """hbuf rows >= B and columns >= 100 hold 0 bits; for ReLU so does every unit whose reference
    z1 < -1e-4 (+0: not -0, not a denormal, not NaN)."""
    p, x, y = dr.data(B)
    z1 = ar.forward(p, x[:B], act)[0]
    tr = _trainer(gpu, B, activation=act, **({} if lean else {"pipeline": False}))
    hb = _views(tr.ws, B)[0]
    hb.fill_(float("nan"))  # (whatever the head does not write stays visible)
    hb[B:].zero_()
    hb[:, 100:].zero_()
    tr.step()
    torch.cuda.synchronize()
    bits = hb.cpu().view(torch.int32)
    assert int((bits[B:] != 0).sum()) == 0 and int((bits[:, 100:] != 0).sum()) == 0
    live = hb[:B, :100].cpu()
    assert bool(torch.isfinite(live).all())
    if act == "relu":
        off = z1 < -ar.ZTOL
        assert int(off.sum()) > 0.3 * B * 100
        assert int((bits[:B, :100][off] != 0).sum()) == 0
        assert bool((live[z1 > ar.ZTOL] > 0).all())
    else:
        sure = ~ar.near_kink(z1)
        assert bool((live.abs() <= 1.0).all())
        assert torch.equal(torch.signbit(live)[sure], (z1 < 0)[sure])


# ---- 3. the applied gradient --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["step", "graph", "launched"])
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("act", NEW)
def test_applied_gradient_matches_float64(gpu, act, B, mode):
    """A momentum = 0 trainer leaves the applied gradient in its slot plane: after 7 steps + flush
    it is the float64 gradient of step 6 at the GPU's pre-flush parameters (ReLU: with the GPU's
    pattern of active units) within 4 x the reference's f32 / f64 gap on that case, floored at
    1e-4.

    Observed on the MI355X, largest over the 15 cases (gap / bound / error): relu 1.11e-6 / 1e-4 /
    8.9e-7 at max |grad| 2.75, tanh 5.5e-7 / 1e-4 / 3.2e-7 at max |grad| 0.65."""
    p, x, y = dr.data(B)
    tr = _trainer(gpu, B, optimizer="momentum", momentum=0.0, activation=act)
    _advance(tr, mode, STEPS)
    assert tr.pending
    before = tr.params.double().cpu()
    b = (STEPS - 1) % NB
    xb, yb = x[b * B:(b + 1) * B], y[b * B:(b + 1) * B]
    ref = ar.step(before, xb, yb, act)
    tag = "%s B=%d %s" % (act, B, mode)
    assert int(ar.near_kink(ref["z1"]).sum()) <= KINK_SHARE * B * 100, tag
    gap = ar.gaps(before, xb, yb, act, ref=ref)
    if mode == "launched":
        tr.run_launched(0, flush=True)
    else:
        tr.flush()
    torch.cuda.synchronize()
    assert tr.global_step() == STEPS
    if act == "relu":
        active = _gpu_pattern(_views(tr.ws, B)[0], B, ref["z1"], None, tag)
        ref = ar.step(before, xb, yb, act, active=active)
    bound = _bounds(gap)["grad"]
    err = float((tr.slots[0].double().cpu() - ref["grad"]).abs().max())
    sig = mlp_step.reference_step(before, xb.double(), yb)[0]
    print("%s: slot vs float64 gradient: gap %.3e bound %.3e error %.3e (max |grad| %.3f; vs the "
          "sigmoid model's gradient %.3e)" % (tag, gap["grad"], bound, err,
                                              float(ref["grad"].abs().max()),
                                              float((tr.slots[0].double().cpu() - sig).abs().max())))
    assert err <= bound


# ---- 4. one model through every way of running it -----------------------------------------------
def _full_kw():
    from distributedtensorflowexample_amd.ops.lr_schedule import LRSchedule

    return dict(optimizer="adam", lr_schedule=LRSchedule("exponential", 2, 0.5, warmup_steps=2),
                weight_decay=0.01, dropout=0.5, dropout_seed=SEED)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sgd", "adam_sched_decay_dropout"])
@pytest.mark.parametrize("B", [17, 100])
@pytest.mark.parametrize("act", NEW)
def test_every_way_of_running_gives_the_same_bits(gpu, act, B, case):
    """step(), run() (max_graph_steps = 3) and run_launched(): 7 + 6 steps over 3 batches, so
    graphs are replayed in later epochs and both plan kinds of the C++ host loop carry the
    activation; and the model is not the sigmoid one."""
    kw = dict(lr=1e-3, **_full_kw()) if case != "sgd" else {}
    outs = []
    for mode in ("step", "graph", "launched"):
        tr = _trainer(gpu, B, activation=act, **kw)
        for n in (7, 6):
            _advance(tr, mode, n)
        tr.flush()
        torch.cuda.synchronize()
        assert tr.global_step() == 13
        outs.append((tr.params.clone(), tr.stats_range(0, 13)))
    for p, st in outs[1:]:
        assert torch.equal(p, outs[0][0])
        assert torch.equal(st, outs[0][1])
    sig = _trainer(gpu, B, **kw)
    _advance(sig, "step", 13)
    sig.flush()
    assert not torch.equal(sig.stats_range(0, 13), outs[0][1])
    assert float((sig.params - outs[0][0]).abs().max()) > 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("act", NEW)
def test_shuffle_mode_host_loop_carries_the_activation(gpu, act):
    """The per-epoch form of run_launched (shuffle mode) against step(), across two boundaries."""
    B = 100
    outs = []
    for mode in ("step", "launched"):
        tr = _trainer(gpu, B, data=dr.data(B, extra=7), activation=act, shuffle=True,
                      shuffle_seed=3)
        _advance(tr, mode, 8)
        tr.flush()
        torch.cuda.synchronize()
        outs.append((tr.params.clone(), tr.stats_range(0, 8)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- 5. the default is today's trainer ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["step", "graph", "launched"])
@pytest.mark.parametrize("B", [17, 100])
def test_sigmoid_is_todays_trainer(gpu, B, mode):
    a = _trainer(gpu, B, lr=0.3)
    b = _trainer(gpu, B, lr=0.3, activation="sigmoid")
    assert a.activation == b.activation == "sigmoid" and b.persistent_ok == a.persistent_ok
    done = 0
    for n in (7, 8):
        for tr in (a, b):
            _advance(tr, mode, n)
            tr.flush()
        done += n
        torch.cuda.synchronize()
        assert a.global_step() == b.global_step() == done
        assert torch.equal(a.params, b.params)
        assert torch.equal(a.stats_range(0, done), b.stats_range(0, done))
    xe, ye = a.x[:50].contiguous(), a.labels[:50].contiguous()
    ea, eb = a.evaluate(xe, ye, probs=True), mlp_eval.evaluate(b.params, xe, ye, probs=True)
    assert torch.equal(ea.acc, eb.acc) and torch.equal(ea.probs, eb.probs)


# ---- 6. the evaluation kernel -------------------------------------------------------------------
def _eval_sizes():
    try:
        T = int(hip().mlp_eval_row_tile())
    except RuntimeError:  # (collection without the built module: the tests then fail loudly)
        T = 64
    return [1, T - 1, T + 1, 3 * T + 5]


@pytest.mark.gpu
@pytest.mark.parametrize("n", _eval_sizes())
@pytest.mark.parametrize("act", NEW)
def test_eval_kernel_matches_float64(gpu, act, n):
    """Loss, accuracy, confusion, predictions and probabilities of ``evaluate(.., activation=)`` on
    n rows: mean loss and probabilities within 4 x the reference's f32 / f64 gap, floored at the
    evaluation tests' sigmoid bounds (1e-4 max(1, |ref|) and 1e-4); predictions equal on every row
    whose float64 top-2 gap exceeds 1e-3 (at most 1 % of the rows, at least one allowed, are
    left out; counts may differ by the rows left out).

    Observed on the MI355X: mean loss within 1e-6 (bounds 2.4e-4 .. 3.2e-4, the floor);
    probabilities relu 4.7e-7 against a gap of 2.8e-7, tanh 1.8e-7 against 1.5e-7 (bound 1e-4, the
    floor); 0 (relu) and 1 (tanh, n >= 63) ambiguous rows."""
    p, x, y = dr.data(100)
    x, y = x[:n].contiguous(), y[:n].contiguous()
    ref = ar.step(p, x, y, act)
    clear = ref["gap"] > 1e-3
    amb = int((~clear).sum())
    assert amb <= max(1, 0.01 * n)
    gap = ar.gaps(p, x, y, act, ref=ref)
    loss64 = float(ref["loss"])
    b_loss = max(4.0 * gap["rowloss"], 1e-4 * max(1.0, abs(loss64)))
    b_prob = max(4.0 * gap["prob"], 1e-4)
    res = mlp_eval.evaluate(p.to(gpu), x.to(gpu), y.to(gpu), predictions=True, probs=True,
                            activation=act)
    pred, probs = res.pred.cpu().long(), res.probs.cpu().double()
    e_prob = float((probs - ref["prob"]).abs().max())
    print("%s n=%d: loss %.6f ref %.6f (gap %.2e bound %.2e) prob error %.2e (gap %.2e bound "
          "%.2e), %d ambiguous rows" % (act, n, res.loss, loss64, gap["rowloss"], b_loss, e_prob,
                                        gap["prob"], b_prob, amb))
    assert res.count == n and pred.shape == (n,) and probs.shape == (n, 10)
    assert abs(res.loss - loss64) <= b_loss
    assert e_prob <= b_prob
    want = ref["logits"].argmax(1)
    assert torch.equal(pred[clear], want[clear])
    assert abs(res.correct - int(ref["correct"].sum())) <= amb
    conf = torch.zeros(10, 10, dtype=torch.int64)
    conf.index_put_((y.long(), pred), torch.ones(n, dtype=torch.int64), accumulate=True)
    assert torch.equal(res.confusion, conf) and res.correct == int((pred == y.long()).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("act", NEW)
def test_trainer_evaluates_with_its_activation(gpu, act):
    B = 100
    tr = _trainer(gpu, B, activation=act)
    for _ in range(3):
        tr.step()
    ev = tr.evaluate(tr.x, tr.labels, probs=True)
    snap = tr.snapshot()
    want = mlp_eval.evaluate(snap, tr.x, tr.labels, probs=True, activation=act)
    sig = mlp_eval.evaluate(snap, tr.x, tr.labels, probs=True)
    torch.cuda.synchronize()
    assert tr.global_step() == 3
    assert torch.equal(ev.acc, want.acc) and torch.equal(ev.probs, want.probs)
    assert not torch.equal(ev.probs, sig.probs) and abs(ev.loss - sig.loss) > 1e-3


# ---- 7. the all-reduce engine -------------------------------------------------------------------
AR_STEPS, AR_LR = 12, 0.01


def _cpu_gap(act, B, data):
    """max |p_f32 - p_f64| of two CPU sgd trajectories of ``activation_reference.step`` (as
    test_fused_optim_gpu's CPU_GAP, computed here).  ReLU: the f32 run takes each step's pattern of
    active units from the float64 run, so a unit at the kink is not an f32 error."""
    p, x, y = data
    p64, p32, lr = p.double(), p.float(), float(np.float32(AR_LR))
    for s in range(AR_STEPS):
        sl = slice((s % NB) * B, (s % NB + 1) * B)
        r64 = ar.step(p64, x[sl], y[sl], act)
        active = (r64["z1"] > 0) if act == "relu" else None
        r32 = ar.step(p32, x[sl], y[sl], act, active=active, dtype=torch.float32)
        p64 = p64 - lr * r64["grad"]
        p32 = p32 - lr * r32["grad"]
    return float((p32.double() - p64).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("act", NEW)
def test_allreduce_engine_matches_single_gpu(gpu, act):
    """world_size = 2 with an ``allreduce`` that doubles the gradient in place (two identical
    replicas): the single-GPU trainer's parameters after 12 sgd steps within 4 x the CPU f32 / f64
    gap of that trajectory, eager and graph replay.  The two engines sum the K slabs in different
    orders, so with ReLU a unit within an ulp of 0 could flip; on this data (seed 0) none does.

    Observed on the MI355X: 2.98e-8 for both activations, eager and graph; CPU gaps 1.09e-7 (relu)
    and 9.52e-8 (tanh), bounds 4.37e-7 and 3.81e-7."""
    B = 100
    data = dr.data(B)
    gap = _cpu_gap(act, B, data)
    tol = 4.0 * gap
    one = _trainer(gpu, B, data=data, lr=AR_LR, activation=act)
    one.run(AR_STEPS)
    one.flush()
    sig = _trainer(gpu, B, data=data, lr=AR_LR)
    sig.run(AR_STEPS)
    sig.flush()
    for use_graph in (False, True):
        dp = _trainer(gpu, B, data=data, lr=AR_LR, allreduce=lambda g: g.mul_(2.0), world_size=2,
                      activation=act)
        assert not dp.pipelined
        dp.max_graph_steps = 3
        dp.run(AR_STEPS, use_graph=use_graph)
        dp.flush()
        torch.cuda.synchronize()
        assert dp.global_step() == AR_STEPS
        err = float((dp.params - one.params).abs().max())
        print("all-reduce engine %s %s: CPU f32/f64 gap %.3e bound %.3e error %.3e"
              % (act, "graph" if use_graph else "eager", gap, tol, err))
        assert err <= tol
        assert float((dp.params - sig.params).abs().max()) > 100 * tol  # (not the sigmoid model)


# ---- 8. refusals --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("act", NEW)
def test_unsupported_combinations_raise(gpu, act):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = (t.to(gpu) for t in dr.data(100))
    comm = object()  # never touched: the constructor refuses first
    with pytest.raises(ValueError, match="activation %s: the exchange engines" % act):
        FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, fused_comm=comm, activation=act)
    with pytest.raises(ValueError, match="activation %s: the exchange engines" % act):
        FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, factor_comm=comm,
                        x_all=torch.stack([x, x]), activation=act)
    with pytest.raises(ValueError, match="unknown hidden activation 'gelu'"):
        FusedMLPTrainer(p, x, y, 100, 0.1, activation="gelu")
    tr = FusedMLPTrainer(p, x, y, 100, 0.1, activation=act)
    assert not tr.persistent_ok
    with pytest.raises(ValueError, match="run_persistent.*sigmoid head only"):
        tr.run_persistent(4)
    old = hip().mlp_set_flush_fused(1)  # DTFX_MLP_FLUSH_FUSED, selected in-process
    try:
        with pytest.raises(ValueError, match="fused flush.*sigmoid head only"):
            tr.run_launched(4, flush=True)
        with pytest.raises(RuntimeError, match="fused flush.*no relu / tanh variant"):
            plan = hip().MlpRunPlan(tr.bufs[0].data_ptr(), tr.bufs[1].data_ptr(),
                                    tr.x.data_ptr(), tr.labels.data_ptr(), tr.nbatches,
                                    tr.ws.buf.data_ptr(), tr.ws.ctr.data_ptr(),
                                    tr.ws.stats.data_ptr(), tr.ws.stats_ring, 100)
            plan.set_act(1 if act == "relu" else 2)
            plan.run(0, 0, 0.1, 0, 4, 1, 0)
    finally:
        hip().mlp_set_flush_fused(old)
    for bad in (3, -1):  # the launchers validate the id themselves
        with pytest.raises(RuntimeError, match="unknown hidden activation id"):
            hip().mlp_lean_head(tr.bufs[0].data_ptr(), tr.labels.data_ptr(),
                                tr.ws.buf.data_ptr(), 100, 0, bad)
        with pytest.raises(RuntimeError, match="unknown hidden activation id"):
            hip().mlp_head(tr.bufs[0].data_ptr(), 0, 0.0, 0, tr.labels.data_ptr(),
                           tr.ws.buf.data_ptr(), 100, 0, 0, bad)
        with pytest.raises(ValueError, match="unknown hidden activation id"):
            hip().mlp_eval(tr.bufs[0].data_ptr(), tr.x.data_ptr(), 0, 100, 0,
                           0, 0, 0, bad)
    torch.cuda.synchronize()
    assert tr.global_step() == 0 and not tr.pending and torch.equal(tr.params, p)
    assert FusedMLPTrainer(p, x, y, 100, 0.1).persistent_ok  # (sigmoid: unchanged)


KS14_SCRIPT = """
import torch
from distributedtensorflowexample_amd.ops import mlp_step
from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer
p = torch.zeros(mlp_step.NPARAM, device="cuda")
x = torch.zeros(300, 784, device="cuda")
y = torch.zeros(300, dtype=torch.int32, device="cuda")
for act in ("relu", "tanh"):
    try:
        FusedMLPTrainer(p, x, y, 100, 0.1, activation=act)
    except ValueError as e:
        print("REFUSED", e)
tr = FusedMLPTrainer(p, x, y, 100, 0.1, activation="sigmoid")
print("SIGMOID", tr.activation)
"""


@pytest.mark.gpu
def test_ks14_refuses_relu_and_tanh(gpu):
    """DTFX_MLP_KS is read once per process, so this refusal is shown in a child process."""
    env = dict(os.environ, DTFX_MLP_KS="14")
    r = subprocess.run([sys.executable, "-c", KS14_SCRIPT], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "REFUSED activation relu: DTFX_MLP_KS=14" in r.stdout, r.stdout + r.stderr
    assert "REFUSED activation tanh: DTFX_MLP_KS=14" in r.stdout, r.stdout + r.stderr
    assert "SIGMOID sigmoid" in r.stdout, r.stdout + r.stderr


# ---- 9. the mirrored loop on the GPU: checkpoint and resume -------------------------------------
@pytest.mark.gpu
def test_mirrored_loop_trains_and_resumes_with_relu(gpu, tmp_path, monkeypatch):
    """``train_mirrored`` on one GPU with --activation relu: 5 steps, the chief's checkpoint, a
    restart to 10 -- the bits of an uninterrupted 10-step run, and not the sigmoid run's."""
    from distributedtensorflowexample_amd.data.mnist import DataSet, DataSets
    from distributedtensorflowexample_amd.train.mirrored_mlp import train_mirrored

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    B = 100
    _, x, y = dr.data(B, extra=7)
    x, y = x.numpy(), y.numpy().astype(np.uint8)
    test = DataSet(x[:64], y[:64], one_hot=False)
    ds = DataSets(train=DataSet(x, y, one_hot=False), validation=test, test=test,
                  synthetic_train=True)

    def run(tag, steps, **more):
        fl = types.SimpleNamespace(batch_size=B, learning_rate=1e-2, training_steps=steps,
                                   logdir=str(tmp_path / tag), log_every=5, eval_every=5,
                                   save_model_secs=1000.0, save_summaries_secs=1000.0,
                                   use_locking=False, seed=0, device="cuda", **more)
        return train_mirrored(fl, ds, log=lambda *_: None)

    _, full = run("full", 10, activation="relu")
    run("part", 5, activation="relu")
    hist, cont = run("part", 10, activation="relu")
    assert [h[0] for h in hist] == [10]
    assert torch.equal(full, cont)
    _, sig = run("sig", 10)
    assert float((full - sig).abs().max()) > 1e-4
