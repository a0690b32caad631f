"""LARS / LAMB (``csrc/kernels/optim.hip``'s two-launch kernels, ``ops.optim.lars_`` / ``lamb_``) and
``FusedMLPTrainer(optimizer="lars" | "lamb")`` against the float64 definition (``ops/layerwise.py``).

Each segment's ``p`` is scaled by a different power of ten (1e-2 .. 1e1) and its ``g`` by the reverse:
a ratio or partial sum taken from the wrong place is off by far more than any bound.  Bounds, per
segment: 4 x the gap between the float32 CPU implementation and float64 on the same inputs, floored
at ``optim_reference.bound(1, ref)`` (``test_optim_kernels_gpu``'s for ``adam_``); trajectories 4 x
the f32-versus-f64 CPU trajectory gap (LAMB at epsilon 1e-3).  Every comparison prints its figures.
"""
import numpy as np
import pytest
import torch

import optim_reference as R
from distributedtensorflowexample_amd.ops import layerwise, mlp_step, optim

pytestmark = pytest.mark.gpu

KINDS = ["lars", "lamb"]
MLP = (0, 78400, 78500, 79500, 79510)
TABLES = [(0, 8), (0, 1024, 2052), (0, 4, 1032, 1038), MLP]
LR, WD, ETA = 0.1, 0.01, 0.02


def _lw(kind, wd=WD, **kw):
    return layerwise.Layerwise(kind, wd, ETA, **kw)


def _case(kind, seg):
    gen = torch.Generator().manual_seed(seg[-1] + len(kind))
    n = seg[-1]
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    for k, (a, b) in enumerate(zip(seg, seg[1:])):
        p[a:b] *= 10.0 ** (k % 4 - 2)
        g[a:b] *= 10.0 ** (1 - k % 4)
    slots = [0.1 * torch.randn(n, generator=gen)]
    if kind == "lamb":
        slots.append(0.01 * torch.rand(n, generator=gen))
    return p, g, slots


def _call(lw, p, g, slots, lr, t, seg, tensors=False):
    kw = dict(lw.kw)
    if tensors:
        kw["lr_tensor"] = torch.tensor([lr], dtype=torch.float32, device=p.device)
        lr = 999.0
    if lw.kind == "lars":
        return optim.lars_(p, g, slots[0], lr, seg, **kw)
    if tensors:
        kw["step_tensor"] = torch.tensor([t], dtype=torch.int32, device=p.device)
        t = 77
    return optim.lamb_(p, g, slots[0], slots[1], lr, t, seg, **kw)


def _check(gpu, lw, seg, case, tensors=False, t=3):
    p, g, slots = case
    ref_p, ref_s = lw.update(p, g, slots, float(np.float32(LR)), t, seg)
    cp, cs = p.clone(), [s.clone() for s in slots]
    _call(lw, cp, g, cs, LR, t, seg, tensors)
    gp, gs = p.to(gpu), [s.to(gpu) for s in slots]
    _call(lw, gp, g.to(gpu), gs, LR, t, seg, tensors)
    torch.cuda.synchronize()
    for name, got, cpu, ref in zip("p s0 s1".split(), [gp] + gs, [cp] + cs, [ref_p] + ref_s):
        assert bool(torch.isfinite(got).all())
        for k, (a, b) in enumerate(zip(seg, seg[1:])):
            gap = float((cpu[a:b].double() - ref[a:b]).abs().max())
            bound = max(4.0 * gap, R.bound(1, ref[a:b]))
            err = float((got[a:b].double().cpu() - ref[a:b]).abs().max())
            print("%s %s seg %d [%d, %d): gap %.3e bound %.3e error %.3e"
                  % (lw.kind, name, k, a, b, gap, bound, err))
            assert err <= bound, (name, k)
    return gp, gs


@pytest.mark.parametrize("tensors", [False, True])
@pytest.mark.parametrize("seg", TABLES, ids=lambda s: "n%d" % s[-1])
@pytest.mark.parametrize("kind", KINDS)
def test_one_call_matches_float64(gpu, kind, seg, tensors):
    gp, _ = _check(gpu, _lw(kind), seg, _case(kind, seg), tensors)
    assert not torch.equal(gp.cpu(), _case(kind, seg)[0])


@pytest.mark.parametrize("case", ["p0", "g0"])
@pytest.mark.parametrize("kind", KINDS)
def test_fallbacks(gpu, kind, case):
    """Segment 1 with p = 0 takes r = 1; with g = 0 (lamb: m = v = 0) and no decay the ratio's
    denominator is 0: lamb leaves p bit-identical, lars ends finite with accum = mu accum."""
    seg, (a, b) = TABLES[1], (1024, 2052)
    p, g, slots = _case(kind, seg)
    if case == "p0":
        p[a:b] = 0.0
        _check(gpu, _lw(kind), seg, (p, g, slots))
        return
    g[a:b] = 0.0
    if kind == "lamb":
        slots[0][a:b], slots[1][a:b] = 0.0, 0.0
    gp, gs = _check(gpu, _lw(kind, 0.0), seg, (p, g, slots))
    if kind == "lamb":
        assert torch.equal(gp[a:b].cpu(), p[a:b])
    else:
        assert torch.equal(gs[0][a:b].cpu(), slots[0][a:b] * 0.9)
    assert not torch.equal(gp[:a].cpu(), p[:a])


@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_give_the_same_bits(gpu, kind):
    outs = []
    for _ in range(2):
        p, g, slots = (t.to(gpu) if torch.is_tensor(t) else [s.to(gpu) for s in t]
                       for t in _case(kind, MLP))
        _call(_lw(kind), p, g, slots, LR, 2, MLP)
        outs.append([p] + slots)
    assert all(torch.equal(a, b) for a, b in zip(*outs))


STEPS, EPS, _CACHE = 4, 1e-3, {}
TLR = {"lars": 0.5, "lamb": 0.01}


def _data(B):
    gen = torch.Generator().manual_seed(3000 + B)
    x = torch.rand(3 * B, 784, generator=gen) * (torch.rand(3 * B, 784, generator=gen) < 0.2)
    p = 0.1 * torch.randn(mlp_step.NPARAM, generator=gen)
    return p, x, torch.randint(0, 10, (3 * B,), generator=gen).to(torch.int32)


def _trajectory(kind, B, dtype):
    if (kind, B, dtype) not in _CACHE:
        p, x, y = _data(B)
        p, x = p.to(dtype), x.to(dtype)
        lw = _lw(kind, epsilon=EPS)
        slots = [torch.zeros_like(p) for _ in range(1 if kind == "lars" else 2)]
        for s in range(STEPS):
            sl = slice((s % 3) * B, (s % 3 + 1) * B)
            g = mlp_step.reference_step(p, x[sl], y[sl])[0]
            if dtype == torch.float64:
                p, slots = lw.update(p, g, slots, float(np.float32(TLR[kind])), s + 1, MLP)
            else:
                _call(lw, p, g, slots, TLR[kind], s + 1, MLP)
        _CACHE[(kind, B, dtype)] = p
    return _CACHE[(kind, B, dtype)]


def _run(gpu, kind, B, graph, **kw):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = _data(B)
    tr = FusedMLPTrainer(p.to(gpu), x.to(gpu), y.to(gpu), B, TLR[kind], optimizer=kind,
                         weight_decay=WD, lars_eta=ETA, epsilon=EPS, **kw)
    assert not tr.pipelined and not tr.direct and not tr.host_loop_ok and not tr.persistent_ok
    if graph:
        tr.run(STEPS)
    else:
        for _ in range(STEPS):
            tr.step()
    tr.flush()
    assert tr.global_step() == STEPS and not tr.pending
    return [tr.params.clone()] + [s.clone() for s in tr.slots] + [tr.stats_range(0, STEPS)]


@pytest.mark.parametrize("kind,B,dtype", [(k, B, "fp32") for k in KINDS for B in (100, 257)]
                         + [("lamb", 257, "bf16")])
def test_trainer_matches_float64_and_graph_replay(gpu, kind, B, dtype):
    """Eager against the float64 loop; graph replay bit-identical (bf16: that and a finite loss)."""
    eager = _run(gpu, kind, B, False, compute_dtype=dtype)
    graph = _run(gpu, kind, B, True, compute_dtype=dtype)
    assert all(torch.equal(a, b) for a, b in zip(eager, graph))
    assert bool(torch.isfinite(eager[-1]).all())
    if dtype == "bf16":
        return
    p64, p32 = _trajectory(kind, B, torch.float64), _trajectory(kind, B, torch.float32)
    gap = float((p32.double() - p64).abs().max())
    err = float((eager[0].double().cpu() - p64).abs().max())
    print("%s B=%d parameters: gap %.3e bound %.3e error %.3e (moved %.3e)"
          % (kind, B, gap, 4.0 * gap, err, float((p64 - _data(B)[0].double()).abs().max())))
    assert err <= 4.0 * gap


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(gpu, kind):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = (t.to(gpu) for t in _data(100))
    for kw, msg in [(dict(world_size=2, fused_comm=object()), "exchange engines"),
                    (dict(world_size=2, factor_comm=object()), "exchange engines"),
                    (dict(pipeline=False), "pipeline=False"),
                    (dict(nesterov=True), "nesterov needs optimizer momentum")]:
        with pytest.raises(ValueError, match=msg):
            FusedMLPTrainer(p, x, y, 100, 0.1, optimizer=kind, **kw)
    with pytest.raises(ValueError, match="run_persistent"):
        FusedMLPTrainer(p, x, y, 100, 0.1, optimizer=kind).run_persistent(2)
    q, g, slots = (t.to(gpu) if torch.is_tensor(t) else [s.to(gpu) for s in t]
                   for t in _case(kind, (0, 40)))
    with pytest.raises(ValueError, match="multiple of 4"):
        _call(_lw(kind), q, g, slots, LR, 1, (0, 6, 40))
    with pytest.raises(ValueError, match="1..8 segments"):
        _call(_lw(kind), q, g, slots, LR, 1, tuple(range(0, 44, 4)))
