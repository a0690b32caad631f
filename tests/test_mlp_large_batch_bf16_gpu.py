"""The bf16 large-batch kernels (``csrc/kernels/mlp_large_batch_bf16.hip``, ``ops.mlp_large_batch.
step_grad_bf16``) and ``FusedMLPTrainer(compute_dtype="bf16")``.

Data as ``test_mlp_large_batch_gpu``: seeded, about 80 % zeros, N(0, 0.1) parameters.  bf16 rounding
on the CPU is ``t.bfloat16()``: round-to-nearest-even, the kernels' conversion.  The float64
references multiply exactly the operands the kernels multiply (bf(x), bf(W1); for dW1 the kernel's
own bf16 dz1 plane), so the only error left is f32 accumulation and the f32 rule applies: 4 x the
gap between that reference in float32 and in float64, floored at that file's FLOOR (gradient 1e-4,
loss 1e-4).  Every test prints gap, bound and error.
"""
import pytest
import torch

from distributedtensorflowexample_amd.ops import hidden_act, mlp_step
from distributedtensorflowexample_amd.parallel import gpu_ps_optim

FLOOR = dict(grad=1e-4, loss=1e-4)
SEGS = dict(b1=(mlp_step.OFF_B1, mlp_step.OFF_W2), W2=(mlp_step.OFF_W2, mlp_step.OFF_B2),
            b2=(mlp_step.OFF_B2, mlp_step.NPARAM))
TB, EPS = 257, 1e-3
LR = {"sgd": 0.05, "momentum": 0.05, "adam": 1e-3}


def _data(B, nb=1):
    g = torch.Generator().manual_seed(1000 * nb + B)
    x = torch.rand(nb * B, 784, generator=g) * (torch.rand(nb * B, 784, generator=g) < 0.2)
    p = 0.1 * torch.randn(mlp_step.NPARAM, generator=g)
    y = torch.randint(0, 10, (nb * B,), generator=g).to(torch.int32)
    return p, x, y


def _reference(p, x, y, act):
    """h, dz1, dl, the gradient and the loss of ``reference_forward`` / ``reference_step`` in the
    dtype of ``p``."""
    h, logits = mlp_step.reference_forward(p, x, act)
    dl = (torch.softmax(logits, 1) - torch.nn.functional.one_hot(y.long(), 10).to(p.dtype)) / len(y)
    d = h * (1 - h) if act == "sigmoid" else hidden_act.derivative(h, act)
    g, loss, acc = mlp_step.reference_step(p, x, y, act)
    return dict(h=h, dz1=(dl @ mlp_step.unflatten(p)[2]) * d, dl=dl, g=g, loss=float(loss),
                acc=float(acc), logits=logits)


def _check(name, got, r32, r64, floor=FLOOR["grad"], rel=False):
    gap = float((r32.double() - r64).abs().max())
    bound, err = max(4.0 * gap, floor), float((got.double() - r64).abs().max())
    print("%s: gap %.3e bound %.3e error %.3e (max |ref| %.3e)"
          % (name, gap, bound, err, float(r64.abs().max())))
    assert err <= bound, name
    assert not rel or err <= 0.01 * float(r64.abs().max()), name  # (the floor alone passes zeros)


# ---- 1, 2. factors and gradient ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,act", [(257, "sigmoid"), (271, "sigmoid"), (400, "sigmoid"),
                                   (1031, "sigmoid"), (257, "relu"), (257, "tanh")])
def test_factors_and_gradient_match_float64(gpu, B, act):
    """One ``step_grad_bf16`` (twice: the same bits): h, dz1, dl, loss and accuracy against float64
    at bf(x) and bf(W1); the bf16 dz1 plane against the f32 one, bit for bit, zero past row B; dW1
    against float64 ``dz1h^T . bf(x)``; the small segments against the reference's gradient.  257:
    one live row in the last 16-row tile, 31 dead rows in the last 32-row chunk; 271 = 16 x 17 - 1;
    400: whole tiles, half a chunk; 1031: at least five slices, the last ragged."""
    from distributedtensorflowexample_amd.ops import mlp_large_batch as lb

    p, x, y = _data(B)
    xh = x.bfloat16()
    pr = p.clone()
    pr[:mlp_step.OFF_B1] = pr[:mlp_step.OFF_B1].bfloat16().float()
    r32, r64 = _reference(pr, xh.float(), y, act), _reference(pr.double(), xh.double(), y, act)
    S, R = lb.slices_bf16(B)
    print("B=%d %s: %d slices of %d rows" % (B, act, S, R))
    assert S >= 2 and 64 <= R <= 256 and R % 32 == 0 and S * R >= B
    ws = lb.LargeBatchWorkspace(B, gpu, stats_ring=8, bf16=True)
    ws.set_global_step(5)
    pg, xg, yg = p.to(gpu), xh.to(gpu), y.to(gpu)
    grads = []
    for k in range(2):
        grad = torch.full((mlp_step.NPARAM,), float("nan"), device=gpu)
        lb.step_grad_bf16(pg, xg, yg, ws, grad, activation=act)
        torch.cuda.synchronize()
        assert ws.global_step() == 6 + k
        grads.append(grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(ws.stats[5], ws.stats[6])
    assert int((ws.buf[-4:].view(torch.int32) != 0).sum()) == 0
    f = {k: v.cpu() for k, v in ws.factors_bf16().items()}
    for k in ("h", "dz1", "dl"):
        n = r64[k].shape[1]
        _check("B=%d %s %s" % (B, act, k), f[k][:B, :n], r32[k], r64[k])
    assert torch.equal(f["dz1h"][:B], f["dz1"][:B].bfloat16())
    assert int((f["dz1h"][B:] != 0).sum()) == 0 and f["dz1h"].shape[0] == (B + 31) // 32 * 32
    loss, acc = (float(v) for v in ws.stats[5].cpu())
    gap = abs(r32["loss"] - r64["loss"])
    top = r64["logits"].topk(2, 1).values
    amb = float(((top[:, 0] - top[:, 1]) <= 1e-3).sum()) / B
    print("loss: gap %.3e bound %.3e error %.3e; accuracy %.4f ref %.4f (near-ties %.4f)"
          % (gap, max(4 * gap, FLOOR["loss"]), abs(loss - r64["loss"]), acc, r64["acc"], amb))
    assert abs(loss - r64["loss"]) <= max(4.0 * gap, FLOOR["loss"])
    assert abs(acc - r64["acc"]) <= amb + 1e-6
    got = grads[0].cpu()
    dzh = f["dz1h"][:B, :100]
    _check("B=%d %s dW1" % (B, act), got[:mlp_step.OFF_B1].view(100, 784),
           dzh.float().t() @ xh.float(), dzh.double().t() @ xh.double(), rel=True)
    for k, (a, b) in SEGS.items():
        _check("B=%d %s %s" % (B, act, k), got[a:b], r32["g"][a:b], r64["g"][a:b], rel=True)


# ---- 3. the trainer ---------------------------------------------------------------------------------
def _trainer(gpu, B=TB, **kw):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = _data(TB, 3)
    return FusedMLPTrainer(p.to(gpu), x.to(gpu), y.to(gpu), B, **kw)


def _final(tr):
    tr.flush()
    torch.cuda.synchronize()
    tr.check()
    return tr.params.clone(), tr.stats_range(0, tr.global_step())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam"])
def test_trainer_is_the_kernels_plus_the_optimizer(gpu, kind):
    """One ``step()`` + ``flush()`` == ``step_grad_bf16`` + the same ``ops.optim`` apply, bitwise;
    ``run(4)`` (graph replay) == four ``step()``s, bitwise; ``check()`` and ``evaluate()``."""
    from distributedtensorflowexample_amd.ops import mlp_large_batch as lb
    from distributedtensorflowexample_amd.ops import optim

    kw = dict(learning_rate=LR[kind], optimizer=kind, epsilon=EPS, compute_dtype="bf16")
    tr = _trainer(gpu, **kw)
    assert tr.large and tr.ws.bf16 and tr.batch(0)[0].dtype == torch.bfloat16
    tr.step()
    one = _final(tr)[0]
    p, x, y = (t.to(gpu) for t in _data(TB, 3))
    ws = lb.LargeBatchWorkspace(TB, gpu, bf16=True)
    grad = torch.zeros_like(p)
    lb.step_grad_bf16(p, x[:TB].bfloat16(), y[:TB], ws, grad)
    h = gpu_ps_optim.hyper_args(kind, epsilon=EPS)
    slots = [torch.zeros_like(p) for _ in range(gpu_ps_optim.num_slots(kind))]
    if kind == "sgd":
        optim.sgd_(p, grad, LR[kind])
    elif kind == "momentum":
        optim.momentum_(p, grad, slots[0], LR[kind], momentum=h[0])
    else:
        optim.adam_(p, grad, slots[0], slots[1], LR[kind], 0, beta1=h[0], beta2=h[1], eps=h[2],
                    step_tensor=ws.ctr, weight_decay=0.0, adamw=False)
    assert torch.equal(one, p) and not torch.equal(one, _data(TB, 3)[0].to(gpu))
    for _ in range(3):
        tr.step()
    eager = _final(tr)
    tg = _trainer(gpu, **kw)
    tg.run(4)
    graph = _final(tg)
    assert tg.global_step() == 4 and all(torch.equal(a, b) for a, b in zip(eager, graph))
    ev = tg.evaluate(*(t.to(gpu) for t in _data(TB, 3)[1:]))
    assert bool(torch.isfinite(torch.tensor([ev.loss, ev.accuracy])).all())


@pytest.mark.gpu
def test_shuffle_across_an_epoch_graph_equals_eager(gpu):
    """``shuffle=True`` over 3 batches, 5 steps: the bf16 copy is remade at the epoch boundary."""
    outs = []
    for graph in (False, True):
        tr = _trainer(gpu, learning_rate=0.05, shuffle=True, shuffle_seed=3, compute_dtype="bf16")
        if graph:
            tr.run(5)
        else:
            for _ in range(5):
                tr.step()
        outs.append(_final(tr))
        assert tr.epoch == 1 and torch.equal(tr.xh, tr.x.bfloat16())
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert bool(torch.isfinite(outs[0][1]).all())


# ---- 4. refusals and non-interference ---------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_and_fp32_is_todays_trainer(gpu):
    from distributedtensorflowexample_amd.ops import mlp_large_batch as lb

    with pytest.raises(ValueError, match="compute_dtype.*256"):
        _trainer(gpu, B=256, compute_dtype="bf16")
    p, x, y = (t.to(gpu) for t in _data(TB))
    ws = lb.LargeBatchWorkspace(TB, gpu, bf16=True)
    grad = torch.zeros_like(p)
    wide = torch.zeros(TB + 1, 2 * 784, device=gpu, dtype=torch.bfloat16)
    for bad in (x, wide.view(-1)[4:4 + TB * 784].view(TB, 784), wide[:TB, :784]):
        with pytest.raises(ValueError, match="xh must be"):
            lb.step_grad_bf16(p, bad, y, ws, grad)
    outs = []
    for kw in ({}, {"compute_dtype": "fp32"}):
        tr = _trainer(gpu, learning_rate=0.05, **kw)
        tr.step()
        tr.step()
        outs.append(_final(tr))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
