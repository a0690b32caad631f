"""Hidden-layer dropout inside the fused MLP step (``FusedMLPTrainer(dropout=..., dropout_seed=...)``,
``ops/dropout.py``): the exact Philox mask in ``hbuf``, the head against float64, the applied
gradient, nothing frozen in a captured graph, resume through ``seek``, ``dropout=0`` as today's
trainer, ``evaluate`` / ``snapshot``, the all-reduce engine and the refusals.

Data: ``dropout_reference.data`` (the recipe of test_fused_optim_gpu._data: p = 0.1 randn with zero
biases, x = rand, 3 batches so ``x_prev`` wraps); batch sizes 1, 17, 100 (NGT = 7), 113 and 256;
rates 0.5 (scale exactly 2) and 0.1; ``dropout_seed`` 5; learning rate 0.01.  The float64
trajectories (steps 0..6) are computed once and their preconditions asserted before any GPU
result is looked at: every h >= 1e-3 (the smallest is 0.0019, at batch 17; a zero in hbuf can
then only be a dropped unit: h times the scale is nowhere near an f32 zero), every softmax
probability in [0.0037, 0.70], and a top-2 logit gap of 1e-3 or less on at most 1 % of a case's
rows (at most 4 of the 1,792 rows at B = 256)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dropout_reference as dr
from distributedtensorflowexample_amd.ops import dropout as dropout_mod
from distributedtensorflowexample_amd.ops import mlp_step
from distributedtensorflowexample_amd.ops._ext import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, RATES, SEED, NB = dr.SIZES, dr.RATES, dr.SEED, dr.NB
LR, STEPS, KS, HP = 0.01, 7, 28, mlp_step.HP
_TRAJ = {}


def _traj(B, rate):
    """The float64 dropout trajectory of (B, rate), once, with its preconditions asserted."""
    if (B, rate) not in _TRAJ:
        tr, _ = dr.trajectory(B, rate, STEPS, LR)
        hmin = min(float(r["h"].min()) for _, r in tr)
        pmin = min(float(r["prob"].min()) for _, r in tr)
        pmax = max(float(r["prob"].max()) for _, r in tr)
        near = sum(int((r["gap"] <= 1e-3).sum()) for _, r in tr)
        gmax = max(float(r["grad"].abs().max()) for _, r in tr)
        print("float64 B=%d rate=%g: min h %.5f, prob [%.4f, %.4f], %d of %d rows with a top-2 gap "
              "<= 1e-3, max |grad| %.3f" % (B, rate, hmin, pmin, pmax, near, STEPS * B, gmax))
        assert hmin >= 1e-3
        assert 0.0037 <= pmin and pmax <= 0.70
        assert near <= 0.01 * STEPS * B and (B != 256 or near <= 4)
        assert gmax < 2.0
        _TRAJ[(B, rate)] = tr
    return _TRAJ[(B, rate)]


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


def _ulps(a, b):
    """max distance in units of the last place between two positive f32 tensors"""
    ia = a.contiguous().view(torch.int32).long()
    ib = b.contiguous().view(torch.int32).long()
    return int((ia - ib).abs().max())


def _assert_mask(hb, hb_plain, keep, scale, B, tag):
    live = hb[:B, :100].cpu()
    assert int((hb[B:] != 0).sum()) == 0 and int((hb[:, 100:] != 0).sum()) == 0  # padding
    assert torch.equal(live == 0, ~keep), tag  # zero exactly where the reference mask drops
    want = (hb_plain[:B, :100].cpu() * np.float32(scale))[keep]
    got = live[keep]
    print(tag, "kept entries bit-equal to f32(hbuf_plain * scale):", bool(torch.equal(got, want)))
    assert _ulps(got, want) <= 1


# ---- 1. the exact mask --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("step", [0, 3, 2 ** 31 - 2])
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("B", SIZES)
def test_hbuf_carries_the_exact_mask(gpu, B, rate, step):
    """One copy + forward + lean head at global_step ``step`` (seek), and the three-launch head
    of replica 1: hbuf is 0 exactly where the reference mask drops, its padding is 0, and kept
    entries are f32(hbuf_plain * scale) of the plain head run on the same inputs (1 ulp)."""
    _traj(B, rate)
    _, scale = dr.threshold(rate)
    keep0 = dr.keep_mask(SEED, step, 0, B, rate)
    keep1 = dr.keep_mask(SEED, step, 1, B, rate)
    assert B == 1 or not torch.equal(keep0, keep1)
    for kw, keep in ((dict(), keep0), (dict(pipeline=False, rank=1), keep1)):
        plain = _trainer(gpu, B, **kw)
        drop = _trainer(gpu, B, dropout=rate, dropout_seed=SEED, **kw)
        for tr in (plain, drop):
            tr.seek(step)
            tr.step()
        torch.cuda.synchronize()
        assert drop.global_step() == step + 1
        _assert_mask(_views(drop.ws, B)[0], _views(plain.ws, B)[0], keep, scale, B,
                     "B=%d rate=%g step=%d %s" % (B, rate, step, "direct" if kw else "lean"))


# ---- 2. the head against float64 ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lean", [True, False], ids=["lean", "three_launch"])
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("B", [17, 100])
def test_head_matches_float64(gpu, B, rate, lean):
    """Per-row loss 1e-4, dl 1e-6, dz1 1e-6 x scale (test_mlp_head_labels_gpu's bounds; dz1 grows
    by at most the scale); accuracy on rows whose float64 top-2 gap exceeds 1e-3, which leave out
    at most 1 %."""
    _, ref = _traj(B, rate)[0]
    _, scale = dr.threshold(rate)
    tr = _trainer(gpu, B, dropout=rate, dropout_seed=SEED, **({} if lean else {"pipeline": False}))
    tr.step()
    torch.cuda.synchronize()
    hb, dz, dl, rs, dzt = _views(tr.ws, B)
    if lean:
        dz_g, dl_g = dz[:B, :100], dl[:B, :10]
    else:  # transposed factors: dz1T [112][BP], dlT [16][BP] behind it
        BP = dzt.shape[1]
        dlt = tr.ws.buf[(KS + 2) * BP * HP:(KS + 2) * BP * HP + 16 * BP].view(16, BP)
        dz_g, dl_g = dzt[:100, :B].t(), dlt[:10, :B].t()
    e_loss = float((rs[:B, 0].double().cpu() - ref["rowloss"]).abs().max())
    e_dl = float((dl_g.double().cpu() - ref["dl"]).abs().max())
    e_dz = float((dz_g.double().cpu() - ref["dz"]).abs().max())
    e_h = float((hb[:B, :100].double().cpu() - ref["hd"]).abs().max())
    print("B=%d rate=%g: loss %.3e dl %.3e dz1 %.3e (bound %.3e) hbuf %.3e"
          % (B, rate, e_loss, e_dl, e_dz, 1e-6 * scale, e_h))
    assert e_loss <= 1e-4 and e_dl <= 1e-6 and e_dz <= 1e-6 * scale
    clear = ref["gap"] > 1e-3
    assert int((~clear).sum()) <= 0.01 * B
    assert torch.equal(rs[:B, 1].cpu()[clear] == 1.0, ref["correct"][clear])


# ---- 3. the applied gradient --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["step", "graph", "launched"])
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("B", SIZES)
def test_applied_gradient_matches_float64(gpu, B, rate, mode):
    """A momentum = 0 trainer leaves the applied gradient in its slot plane: after 7 steps + flush
    it is within 1e-4 (the suite's bound for the gradient kernels; |grad| < 2 here) of the float64
    dropout gradient of step 6 at the pre-flush parameters."""
    _traj(B, rate)
    p, x, y = dr.data(B)
    _, scale = dr.threshold(rate)
    tr = _trainer(gpu, B, optimizer="momentum", momentum=0.0, dropout=rate, dropout_seed=SEED)
    _advance(tr, mode, STEPS)
    assert tr.pending
    before = tr.params.double().cpu()
    if mode == "launched":
        tr.run_launched(0, flush=True)
    else:
        tr.flush()
    torch.cuda.synchronize()
    assert tr.global_step() == STEPS
    b = (STEPS - 1) % NB
    ref = dr.step(before, x[b * B:(b + 1) * B], y[b * B:(b + 1) * B],
                  dr.keep_mask(SEED, STEPS - 1, 0, B, rate), scale)
    err = float((tr.slots[0].double().cpu() - ref["grad"]).abs().max())
    plain = mlp_step.reference_step(before, x[b * B:(b + 1) * B].double(), y[b * B:(b + 1) * B])[0]
    print("B=%d rate=%g %s: slot vs float64 dropout gradient %.3e (vs the undropped one %.3e)"
          % (B, rate, mode, err, float((tr.slots[0].double().cpu() - plain).abs().max())))
    assert err < 1e-4


# ---- 4. nothing frozen in a graph ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("B", [17, 100])
def test_graph_replay_takes_each_steps_own_mask(gpu, B, optimizer):
    """max_graph_steps = 3, 7 steps over 3 batches and then 6 more, so captured graphs are replayed
    in later epochs: step(), run() and run_launched() give the same bits, and the hbuf the last
    step leaves carries the mask of its own global_step (6, then 12)."""
    rate = 0.5
    outs = []
    for mode in ("step", "graph", "launched"):
        tr = _trainer(gpu, B, optimizer=optimizer, dropout=rate, dropout_seed=SEED)
        done = 0
        for n in (7, 6):
            _advance(tr, mode, n)
            done += n
            torch.cuda.synchronize()
            hb = _views(tr.ws, B)[0][:B, :100].cpu()
            assert torch.equal(hb != 0, dr.keep_mask(SEED, done - 1, 0, B, rate)), (mode, done)
            assert not torch.equal(hb != 0, dr.keep_mask(SEED, 0, 0, B, rate))
        tr.flush()
        torch.cuda.synchronize()
        assert tr.global_step() == 13
        outs.append((tr.params.clone(), tr.stats_range(0, 13)))
    for p, st in outs[1:]:
        assert torch.equal(p, outs[0][0])
        assert torch.equal(st, outs[0][1])


# ---- 5. resume ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sgd", "adam_sched"])
def test_seek_resumes_the_mask_sequence(gpu, case):
    from distributedtensorflowexample_amd.ops.lr_schedule import LRSchedule

    B = 100
    kw = dict(dropout=0.5, dropout_seed=SEED)
    if case == "adam_sched":
        kw.update(optimizer="adam", lr_schedule=LRSchedule("exponential", 2, 0.5, warmup_steps=2))
    full = _trainer(gpu, B, **kw)
    for _ in range(5):
        full.step()
    full.flush()
    part = _trainer(gpu, B, **kw)
    for _ in range(3):
        part.step()
    snap, slots = part.snapshot(with_slots=True)
    cont = _trainer(gpu, B, **kw)
    cont.load_params(snap)
    cont.load_slots(slots)
    cont.seek(3)
    cont.step()
    cont.step()
    cont.flush()
    torch.cuda.synchronize()
    assert cont.global_step() == full.global_step() == 5
    assert torch.equal(cont.params, full.params)
    for a, b in zip(cont.slots, full.slots):
        assert torch.equal(a, b)
    assert torch.equal(cont.stats_range(3, 5), full.stats_range(3, 5))
    # ... and it is the mask that matters: a run resumed at the wrong step differs
    wrong = _trainer(gpu, B, **kw)
    wrong.load_params(snap)
    wrong.load_slots(slots)
    wrong.seek(3 + NB)  # (the same batches, other masks)
    wrong.step()
    wrong.flush()
    cont2 = _trainer(gpu, B, **kw)
    cont2.load_params(snap)
    cont2.load_slots(slots)
    cont2.seek(3)
    cont2.step()
    cont2.flush()
    assert cont2.stats(3) != wrong.stats(3 + NB)


# ---- 6. dropout = 0 is today's trainer ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["step", "graph", "launched"])
@pytest.mark.parametrize("B", [17, 100])
def test_dropout_zero_is_todays_trainer(gpu, B, mode):
    a = _trainer(gpu, B, lr=0.3)
    b = _trainer(gpu, B, lr=0.3, dropout=0.0, dropout_seed=SEED)
    assert b.drop is None and b.persistent_ok == a.persistent_ok
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


# ---- 7. evaluate() and snapshot() never drop ----------------------------------------------------
@pytest.mark.gpu
def test_evaluate_and_snapshot_do_not_drop_or_move_the_mask(gpu):
    from distributedtensorflowexample_amd.ops import mlp_eval

    B = 100
    kw = dict(dropout=0.5, dropout_seed=SEED)
    a, b = _trainer(gpu, B, **kw), _trainer(gpu, B, **kw)
    for tr in (a, b):
        for _ in range(3):
            tr.step()
    ev = a.evaluate(a.x, a.labels)
    snap = a.snapshot()
    assert a.global_step() == 3
    want = mlp_eval.evaluate(a.flush().clone(), a.x, a.labels)
    torch.cuda.synchronize()
    assert torch.equal(snap, a.params)
    assert (float(ev.accuracy), float(ev.loss)) == (float(want.accuracy), float(want.loss))
    for tr in (a, b):  # (b was never evaluated: the next step's mask and result are the same)
        tr.step()
        tr.flush()
    torch.cuda.synchronize()
    assert a.global_step() == b.global_step() == 4
    hb = _views(a.ws, B)[0][:B, :100].cpu()
    assert torch.equal(hb != 0, dr.keep_mask(SEED, 3, 0, B, 0.5))
    assert torch.equal(a.params, b.params) and a.stats(3) == b.stats(3)


# ---- 8. the all-reduce engine -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam"])
def test_allreduce_engine_matches_single_gpu(gpu, kind):
    """world_size = 2 with an ``allreduce`` that doubles the gradient in place (two identical
    replicas, rank 0's stream): the single-GPU trajectory within test_fused_optim_gpu's
    ``traj_tol`` (4 x the f32 / f64 CPU gap of 12 steps, <= 1.05e-7 over its cases), eager and
    graph replay."""
    B, steps = 100, 12
    lr = {"sgd": 0.05, "momentum": 0.05, "adam": 1e-3}[kind]
    tol = 4.0 * {"sgd": 8.817e-08, "momentum": 8.817e-08, "adam": 1.008e-07}[kind]
    kw = dict(optimizer=kind, epsilon=1e-3, dropout=0.5, dropout_seed=SEED)
    one = _trainer(gpu, B, lr=lr, **kw)
    one.run(steps)
    one.flush()
    nodrop = _trainer(gpu, B, lr=lr, optimizer=kind, epsilon=1e-3)
    nodrop.run(steps)
    nodrop.flush()
    for use_graph in (False, True):
        dp = _trainer(gpu, B, lr=lr, allreduce=lambda g: g.mul_(2.0), world_size=2, **kw)
        assert not dp.pipelined
        dp.max_graph_steps = 3
        dp.run(steps, use_graph=use_graph)
        dp.flush()
        torch.cuda.synchronize()
        assert dp.global_step() == steps
        err = float((dp.params - one.params).abs().max())
        print("all-reduce engine", kind, "graph" if use_graph else "eager", "%.3e" % err,
              "tol %.3e" % tol)
        assert err <= tol
        assert float((dp.params - nodrop.params).abs().max()) > 100 * tol  # (it did drop)


# ---- 9. refusals --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_unsupported_combinations_raise(gpu):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = (t.to(gpu) for t in dr.data(100))
    comm = object()  # never touched: the constructor refuses first
    with pytest.raises(ValueError, match="dropout: the exchange engines"):
        FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, fused_comm=comm, dropout=0.5)
    with pytest.raises(ValueError, match="dropout: the exchange engines"):
        FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, factor_comm=comm,
                        x_all=torch.stack([x, x]), dropout=0.5)
    for bad in (1.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="dropout rate must be in"):
            FusedMLPTrainer(p, x, y, 100, 0.1, dropout=bad)
    with pytest.raises(ValueError, match="keeps nothing"):
        dropout_mod.threshold(1.0 - 2.0 ** -26)
    tr = FusedMLPTrainer(p, x, y, 100, 0.1, dropout=0.5)
    assert not tr.persistent_ok
    with pytest.raises(ValueError, match="run_persistent.*no dropout"):
        tr.run_persistent(4)
    old = hip().mlp_set_flush_fused(1)  # DTFX_MLP_FLUSH_FUSED, selected in-process
    try:
        with pytest.raises(ValueError, match="fused flush.*no dropout"):
            tr.run_launched(4, flush=True)
    finally:
        hip().mlp_set_flush_fused(old)
    torch.cuda.synchronize()
    assert tr.global_step() == 0 and not tr.pending and torch.equal(tr.params, p)
    assert FusedMLPTrainer(p, x, y, 100, 0.1).persistent_ok  # (no dropout: unchanged)


KS14_SCRIPT = """
import torch
from distributedtensorflowexample_amd.ops import mlp_step
from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer
p = torch.zeros(mlp_step.NPARAM, device="cuda")
x = torch.zeros(300, 784, device="cuda")
y = torch.zeros(300, dtype=torch.int32, device="cuda")
try:
    FusedMLPTrainer(p, x, y, 100, 0.1, dropout=0.5)
except ValueError as e:
    print("REFUSED", e)
"""


@pytest.mark.gpu
def test_ks14_refuses_dropout(gpu):
    """DTFX_MLP_KS is read once per process, so this refusal is shown in a child process."""
    env = dict(os.environ, DTFX_MLP_KS="14")
    r = subprocess.run([sys.executable, "-c", KS14_SCRIPT], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "REFUSED dropout: DTFX_MLP_KS=14" in r.stdout, r.stdout + r.stderr


# ---- 10. the mirrored loop on the GPU: checkpoint and resume ------------------------------------
@pytest.mark.gpu
def test_mirrored_loop_resumes_in_the_mask_sequence(gpu, tmp_path, monkeypatch):
    """``train_mirrored`` on one GPU with --dropout 0.5, adam, an exponential schedule and
    --shuffle: 5 steps, the chief's checkpoint, a restart to 10 -- the bits of an uninterrupted
    10-step run (the checkpoint holds nothing of the mask: ``seek`` restores the counter the head
    reads), and not the bits of the run without dropout."""
    import types

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
    kw = dict(optimizer="adam", lr_schedule="exponential", lr_decay_steps=3, lr_decay_rate=0.5,
              lr_staircase=True, lr_warmup_steps=2, shuffle=True, shuffle_seed=3)

    def run(tag, steps, **more):
        fl = types.SimpleNamespace(batch_size=B, learning_rate=1e-3, training_steps=steps,
                                   logdir=str(tmp_path / tag), log_every=5, eval_every=10 ** 9,
                                   save_model_secs=1000.0, save_summaries_secs=1000.0,
                                   use_locking=False, seed=0, device="cuda", **kw, **more)
        return train_mirrored(fl, ds, log=lambda *_: None)

    drop = dict(dropout=0.5, dropout_seed=SEED)
    _, full = run("full", 10, **drop)
    run("part", 5, **drop)
    hist, cont = run("part", 10, **drop)
    assert [h[0] for h in hist] == [10]
    assert torch.equal(full, cont)
    _, plain = run("plain", 10)
    assert float((full - plain).abs().max()) > 1e-4
