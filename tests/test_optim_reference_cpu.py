"""The float64 optimizer reference of tests/optim_reference.py against the project's float32 CPU
formulas (ops/optim.py, ops/transformer.py, ops/cnn.py): two independent transcriptions must
agree to the bound the GPU kernels are held to, so the reference itself cannot drift."""
import pytest
import torch

import optim_reference as R
from distributedtensorflowexample_amd.ops import cnn, optim
from distributedtensorflowexample_amd.ops import transformer as T

N, STEPS = 1027, 10


def _grads(n, steps, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) for _ in range(steps)]


def test_hyperparameters_round_to_float32():
    assert R.f32(0.9) == 0.89999997615814208984375
    assert R.f32(0.5) == 0.5
    assert R.bound(10, torch.tensor([4.5])) == pytest.approx(1.073e-5, rel=1e-3)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_reference_matches_cpu_sgd(wd):
    p, g, _, _, regions = R.make_case(N, 1)
    ref = p.double()
    for _ in range(STEPS):
        optim.sgd_(p, g, R.f32(0.01), weight_decay=R.f32(wd))
        ref, _ = R.sgd_step(ref, g, 0.01, wd=wd)
    R.assert_close("p", p, ref, STEPS, regions)


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_reference_matches_cpu_momentum(nesterov, wd):
    p, g, buf, _, regions = R.make_case(N, 2)
    ref, rbuf = p.double(), buf.double()
    for _ in range(STEPS):
        optim.momentum_(p, g, buf, R.f32(0.01), R.f32(0.9), R.f32(wd), nesterov)
        ref, rbuf = R.sgd_step(ref, g, 0.01, wd=wd, mu=0.9, nesterov=nesterov, buf=rbuf)
    R.assert_close("p", p, ref, STEPS, regions)
    R.assert_close("buf", buf, rbuf, STEPS, regions)


@pytest.mark.parametrize("adamw", [True, False])
@pytest.mark.parametrize("wd,b1,b2,step0", [(0.0, 0.9, 0.999, 1), (0.01, 0.9, 0.999, 1),
                                            (0.01, 0.8, 0.95, 1000)])
def test_reference_matches_cpu_adam(adamw, wd, b1, b2, step0):
    p, g, m, v, regions = R.make_case(N, 3)
    ref, rm, rv = p.double(), m.double(), v.double()
    for s in range(step0, step0 + STEPS):
        optim.adam_(p, g, m, v, R.f32(1e-3), s, R.f32(b1), R.f32(b2), R.f32(1e-8), R.f32(wd),
                    adamw)
        ref, rm, rv = R.adam_step(ref, g, rm, rv, 1e-3, s, b1, b2, 1e-8, wd, adamw)
    R.assert_close("p", p, ref, STEPS, regions)
    R.assert_close("m", m, rm, STEPS, regions)
    R.assert_close("v", v, rv, STEPS, regions)


@pytest.mark.parametrize("step0", [1, 1000])
def test_reference_matches_cpu_adam_mixed(step0):
    p, g, m, v, regions = R.make_case(1028, 4)
    ref, rm, rv = p.double(), m.double(), v.double()
    for s in range(step0, step0 + STEPS):
        T.adam_mixed(p, g, m, v, None, R.f32(1e-3), s, R.f32(0.9), R.f32(0.999), R.f32(1e-6),
                     R.f32(0.01), 0.5)
        ref, rm, rv = R.adam_mixed_step(ref, g, rm, rv, 1e-3, s, gscale=0.5)
    R.assert_close("p", p, ref, STEPS, regions)
    R.assert_close("m", m, rm, STEPS, regions)
    R.assert_close("v", v, rv, STEPS, regions)


def test_reference_matches_cpu_sgd_momentum_mixed():
    p, g, v, _, regions = R.make_case(1028, 5)
    ref, rv = p.double(), v.double()
    for _ in range(STEPS):
        cnn.sgd_momentum_mixed(p, g, v, None, R.f32(0.01), R.f32(0.9), R.f32(1e-4), 0.5)
        ref, rv = R.sgd_momentum_mixed_step(ref, g, rv, 0.01, 0.9, 1e-4, 0.5)
    R.assert_close("p", p, ref, STEPS, regions)
    R.assert_close("v", v, rv, STEPS, regions)


def test_bf16_edge_patterns():
    """The bf16 words expected of the GPU kernels are torch's own conversion of the patterns."""
    import numpy as np

    x = torch.from_numpy(np.array(R.EDGE_BITS, dtype=np.uint32).view(np.float32).copy())
    want = torch.from_numpy(np.array(R.EDGE_BF16, dtype=np.uint16).view(np.int16).copy())
    assert torch.equal(x.to(torch.bfloat16).view(torch.int16), want)


@pytest.mark.parametrize("kernel", ["adam_mixed", "sgd_momentum_mixed"])
def test_segments_with_cpu_tensors_raise(kernel):
    """A segment table is a GPU path: CPU tensors raise instead of silently ignoring it."""
    p, g, m, v, _ = R.make_case(16, 94)
    segs = torch.tensor([[0, 1, 0, 1, 1]], dtype=torch.int64)
    before = p.clone()
    with pytest.raises(ValueError, match="GPU path"):
        if kernel == "adam_mixed":
            T.adam_mixed(p, g, m, v, None, 1e-3, 1, segs=segs)
        else:
            cnn.sgd_momentum_mixed(p, g, v, None, 0.01, 0.9, 1e-4, 1.0, segs=segs)
    assert torch.equal(p, before)


def test_reference_takes_fresh_gradients_and_state():
    """The injected state is what the step uses: two single steps equal one two-step run of a
    persistent torch optimizer."""
    g0, g1 = _grads(64, 2, 6)
    q = torch.randn(64, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    w = q.clone().requires_grad_(True)
    opt = torch.optim.AdamW([w], lr=R.f32(1e-3), betas=(R.f32(0.9), R.f32(0.999)),
                            eps=R.f32(1e-8), weight_decay=R.f32(0.01), foreach=False)
    p, m, v = q, torch.zeros(64).double(), torch.zeros(64).double()
    for s, g in ((1, g0), (2, g1)):
        w.grad = g.double()
        opt.step()
        p, m, v = R.adam_step(p, g, m, v, 1e-3, s, wd=0.01)
    assert torch.equal(p, w.detach())
