"""The large-batch gradient kernels (``csrc/kernels/mlp_large_batch.hip``, ``ops/mlp_large_batch.py``)
and ``FusedMLPTrainer(batch_size > 256)`` against float64.

Data: seeded uniform x in [0, 1) with about 80 % zeros (MNIST-like), N(0, 0.1) parameters, uniform
labels.  References: ``mlp_step.reference_step`` on float64 copies, on the CPU.  Bounds: 4 x the gap
between that reference in float32 and in float64 on the same inputs, floored at the floors of
``test_fused_activation_gpu._bounds`` (gradient 1e-4, loss 1e-4); trajectories 4 x the gap between
the float32 and the float64 CPU trajectory, as ``test_fused_optim_gpu`` does (Adam at epsilon 1e-3
for the reason given there).  Every test prints gap, bound and error.
"""
import numpy as np
import pytest
import torch

from distributedtensorflowexample_amd.ops import mlp_step
from distributedtensorflowexample_amd.parallel import gpu_ps_optim

FLOOR = dict(grad=1e-4, loss=1e-4)
SEGS = dict(W1=(mlp_step.OFF_W1, mlp_step.OFF_B1), b1=(mlp_step.OFF_B1, mlp_step.OFF_W2),
            W2=(mlp_step.OFF_W2, mlp_step.OFF_B2), b2=(mlp_step.OFF_B2, mlp_step.NPARAM))
TB, STEPS, EPS = 257, 4, 1e-3
LR = {"sgd": 0.05, "momentum": 0.05, "adam": 1e-3}
_CACHE = {}


def _data(B, nb=1):
    g = torch.Generator().manual_seed(1000 * nb + B)
    x = torch.rand(nb * B, 784, generator=g) * (torch.rand(nb * B, 784, generator=g) < 0.2)
    p = 0.1 * torch.randn(mlp_step.NPARAM, generator=g)
    y = torch.randint(0, 10, (nb * B,), generator=g).to(torch.int32)
    return p, x, y


def _grad_case(B, act):
    """(inputs, float64 (grad, loss, acc), f32 / f64 gaps, share of rows with a near-tie), once."""
    if (B, act) not in _CACHE:
        p, x, y = _data(B)
        g64, l64, a64 = mlp_step.reference_step(p.double(), x.double(), y, act)
        g32, l32, _ = mlp_step.reference_step(p, x, y, act)
        gap = {k: float((g32[a:b].double() - g64[a:b]).abs().max()) for k, (a, b) in SEGS.items()}
        gap["loss"] = abs(float(l32) - float(l64))
        top = mlp_step.reference_forward(p.double(), x.double(), act)[1].topk(2, 1).values
        amb = float(((top[:, 0] - top[:, 1]) <= 1e-3).sum()) / B
        _CACHE[(B, act)] = (p, x, y, g64, float(l64), float(a64), gap, amb)
    return _CACHE[(B, act)]


# ---- 1. the gradient --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,act", [(257, "sigmoid"), (271, "sigmoid"), (400, "sigmoid"),
                                   (1031, "sigmoid"), (257, "relu"), (257, "tanh")])
def test_gradient_matches_float64(gpu, B, act):
    """All four gradient segments, the recorded loss and accuracy and global_step + 1 of one
    ``step_grad``; a second call on the same inputs returns the same bits.  257 = 16 x 16 + 1: one
    live row in the last row tile and slice; 271 = 16 x 17 - 1; 400: whole tiles; 1031: at least
    five slices, the last ragged."""
    from distributedtensorflowexample_amd.ops import mlp_large_batch as lb

    p, x, y, g64, l64, a64, gap, amb = _grad_case(B, act)
    S, R = lb.slices(B)
    print("B=%d %s: %d slices of %d rows" % (B, act, S, R))
    assert S >= 2 and 64 <= R <= 256 and R % 16 == 0 and S * R >= B
    ws = lb.LargeBatchWorkspace(B, gpu, stats_ring=8)
    ws.set_global_step(5)
    pg, xg, yg = p.to(gpu), x.to(gpu), y.to(gpu)
    grads = []
    for k in range(2):
        grad = torch.full((mlp_step.NPARAM,), float("nan"), device=gpu)
        lb.step_grad(pg, xg, yg, ws, grad, activation=act)
        torch.cuda.synchronize()
        assert ws.global_step() == 6 + k
        grads.append(grad)
    assert torch.equal(grads[0], grads[1])
    assert torch.equal(ws.stats[5], ws.stats[6])
    assert int((ws.buf[-4:].view(torch.int32) != 0).sum()) == 0
    got = grads[0].double().cpu()
    for k, (a, b) in SEGS.items():
        bound = max(4.0 * gap[k], FLOOR["grad"])
        err = float((got[a:b] - g64[a:b]).abs().max())
        print("B=%d %s %s: gap %.3e bound %.3e error %.3e (max |grad| %.3e)"
              % (B, act, k, gap[k], bound, err, float(g64[a:b].abs().max())))
        assert err <= bound, k
        assert err <= 0.01 * float(g64[a:b].abs().max()), k  # (the floor alone would pass zeros)
    loss, acc = (float(v) for v in ws.stats[5].cpu())
    bound = max(4.0 * gap["loss"], FLOOR["loss"])
    print("B=%d %s loss: gap %.3e bound %.3e error %.3e; accuracy %.4f ref %.4f (near-ties %.4f)"
          % (B, act, gap["loss"], bound, abs(loss - l64), acc, a64, amb))
    assert abs(loss - l64) <= bound
    assert abs(acc - a64) <= amb + 1e-6


# ---- 2. the trainer ---------------------------------------------------------------------------------
def _trajectory(kind, dtype):
    """``STEPS`` steps over 3 batches of 257 rows on the CPU in ``dtype`` with the update rules of
    ``parallel/gpu_ps_optim.py`` (float32: its ``apply_reference``) -> (parameters, losses)."""
    if (kind, dtype) in _CACHE:
        return _CACHE[(kind, dtype)]
    p, x, y = _data(TB, 3)
    p, x = p.to(dtype), x.to(dtype)
    lr = float(np.float32(LR[kind]))
    hyper = gpu_ps_optim.hyper_args(kind, epsilon=EPS)
    slots = [torch.zeros_like(p) for _ in range(gpu_ps_optim.num_slots(kind))]
    losses = []
    for s in range(STEPS):
        sl = slice((s % 3) * TB, (s % 3 + 1) * TB)
        g, loss, _ = mlp_step.reference_step(p, x[sl], y[sl])
        losses.append(float(loss))
        if dtype == torch.float32:
            pn, sn = gpu_ps_optim.apply_reference(kind, p.numpy(), g.numpy(),
                                                  [t.numpy() for t in slots], lr, s + 1, hyper)
            p, slots = torch.from_numpy(pn), [torch.from_numpy(t) for t in sn]
        elif kind == "sgd":
            p = p - lr * g
        elif kind == "momentum":
            slots = [float(np.float32(hyper[0])) * slots[0] + g]
            p = p - lr * slots[0]
        else:
            b1, b2, eps = (float(np.float32(h)) for h in hyper)
            m = b1 * slots[0] + (1 - b1) * g
            v = b2 * slots[1] + (1 - b2) * g * g
            slots = [m, v]
            p = p - (lr / (1 - b1 ** (s + 1))) * m / (v.sqrt() / (1 - b2 ** (s + 1)) ** 0.5 + eps)
    _CACHE[(kind, dtype)] = (p, losses)
    return _CACHE[(kind, dtype)]


def _trainer(gpu, B=TB, **kw):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = _data(TB, 3)
    return FusedMLPTrainer(p.to(gpu), x.to(gpu), y.to(gpu), B, **kw)


def _run(tr, graph):
    if graph:
        tr.run(STEPS)
    else:
        for _ in range(STEPS):
            tr.step()
    tr.flush()
    torch.cuda.synchronize()
    assert tr.global_step() == STEPS and not tr.pending and tr.cur == 0
    tr.check()
    return tr.params.clone(), tr.stats_range(0, STEPS)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam"])
def test_trainer_matches_float64_and_graph_replay(gpu, kind):
    """Four ``step()``s + ``flush()`` at batch 257 against the float64 loop, the step-for-step
    losses too; a second trainer driven by ``run(4)`` (graph replay) ends bit-identical."""
    p64, l64 = _trajectory(kind, torch.float64)
    p32, l32 = _trajectory(kind, torch.float32)
    kw = dict(learning_rate=LR[kind], optimizer=kind, epsilon=EPS)
    tr = _trainer(gpu, **kw)
    assert not tr.pipelined and not tr.direct and not tr.host_loop_ok and not tr.persistent_ok
    p, st = _run(tr, False)
    gap = float((p32.double() - p64).abs().max())
    err = float((p.double().cpu() - p64).abs().max())
    print("%s parameters: gap %.3e bound %.3e error %.3e (moved %.3e)"
          % (kind, gap, 4.0 * gap, err, float((p64 - _data(TB, 3)[0].double()).abs().max())))
    assert err <= 4.0 * gap
    lgap = max(abs(a - b) for a, b in zip(l32, l64))
    lerr = float((st[:, 0].double() - torch.tensor(l64)).abs().max())
    print("%s losses: gap %.3e bound %.3e error %.3e" % (kind, lgap, max(4 * lgap, 1e-4), lerr))
    assert lerr <= max(4.0 * lgap, FLOOR["loss"])
    pg, sg = _run(_trainer(gpu, **kw), True)
    assert torch.equal(pg, p) and torch.equal(sg, st)


@pytest.mark.gpu
def test_trainer_options_replay_like_eager(gpu):
    """Weight decay, the moving average and a schedule on the large-batch engine: graph == eager
    bitwise and a finite loss (their numerics are tested on the engine that applies them)."""
    from distributedtensorflowexample_amd.ops.lr_schedule import LRSchedule

    outs = []
    for graph in (False, True):
        tr = _trainer(gpu, learning_rate=1e-3, optimizer="adam", weight_decay=0.05, ema_decay=0.9,
                      lr_schedule=LRSchedule("exponential", 2, 0.5))
        p, st = _run(tr, graph)
        outs.append((p, st, tr.ema.clone()))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    assert bool(torch.isfinite(outs[0][1]).all()) and not torch.equal(outs[0][0], outs[0][2])


# ---- 3. the allreduce hook --------------------------------------------------------------------------
@pytest.mark.gpu
def test_allreduce_hook_sees_the_gradient(gpu):
    """Two identical replicas (the hook doubles the gradient, world_size = 2): the plain run's bits."""
    plain = _run(_trainer(gpu, learning_rate=0.05), False)[0]
    calls = []

    def hook(g):
        calls.append(g.numel())
        g.mul_(2)

    dp = _run(_trainer(gpu, learning_rate=0.05, allreduce=hook, world_size=2), False)[0]
    assert calls == [mlp_step.NPARAM] * STEPS and torch.equal(dp, plain)


# ---- 4. refusals ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_and_batch_256_is_todays_trainer(gpu):
    with pytest.raises(ValueError, match="dropout"):
        _trainer(gpu, dropout=0.5)
    with pytest.raises(ValueError, match="fused_comm"):
        _trainer(gpu, fused_comm=object(), world_size=2)
    with pytest.raises(ValueError, match="batch_size 65537.*65536"):
        _trainer(gpu, B=65537)
    tr = _trainer(gpu, B=256)
    assert tr.pipelined and isinstance(tr.ws, mlp_step.StepWorkspace)
