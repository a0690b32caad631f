"""Row-major backprop factors (dz1R / dlR) of the single-GPU two-launch MLP step and the
class-per-lane head arithmetic (head_row in csrc/kernels/mlp_step_3launch.h,
wave_reduce_scatter in common.h).

Batches: 1, 15, 16, 17 (one row tile, its edges), 100 (the workload), 112 (the padded batch
itself), 113 (BP = 128 != HP = 112: a swapped pitch shows only here; the generic NGT = 0
kernels) and 128; each with the existing tests' 0.1-scaled weights and with raw N(0, 1) weights
(saturated sigmoids, large logits), 3 batches per dataset.
"""
import math

import pytest
import torch

from distributedtensorflowexample_amd.ops import init, mlp_step

pytestmark = pytest.mark.gpu

BATCHES = [1, 15, 16, 17, 100, 112, 113, 128]
NB, LR = 3, 0.3


def _setup(gpu, B, scaled, seed=4):
    p = torch.empty(mlp_step.NPARAM, device=gpu)
    init.fill_(p, "normal", 0.0, 1.0, seed=seed)
    p[mlp_step.OFF_B1:mlp_step.OFF_W2].zero_()
    p[mlp_step.OFF_B2:].zero_()
    if scaled:
        p.mul_(0.1)
    g = torch.Generator().manual_seed(seed + B)
    x = torch.rand(NB * B, 784, generator=g).to(gpu)
    y = torch.randint(0, 10, (NB * B,), generator=g).to(gpu).int()
    return p, x, y


def _regions(ws):
    """(dz1R [BP][112], dlR [BP][16], rowstat [BP][2]) views of a workspace."""
    from distributedtensorflowexample_amd.ops._ext import hip

    o_dz, o_dl, BP = hip().mlp_rowmajor_layout(ws.B)
    assert BP == (ws.B + 15) // 16 * 16 and o_dl == o_dz + BP * 112
    # regions of their own, after the workspace proper (whose last 4 words are the sync words)
    assert o_dz == ws.buf.numel() and o_dl + BP * 16 == ws.store.numel()
    assert ws.store.numel() == hip().mlp_workspace_floats(ws.B)
    dz = ws.store[o_dz:o_dz + BP * 112].view(BP, 112)
    dl = ws.store[o_dl:o_dl + BP * 16].view(BP, 16)
    rs = ws.buf[-4 - 2 * BP:-4].view(BP, 2)
    return dz, dl, rs


def _assert_padding_zero(ws, dz_live=True):
    B = ws.B
    dz, dl, _ = _regions(ws)
    # (the regions are in use: the live part was written)
    assert float(dl[:B, :10].abs().sum()) > 0
    assert not dz_live or float(dz[:B, :100].abs().sum()) > 0
    assert int((dz[B:] != 0).sum()) == 0 and int((dz[:, 100:] != 0).sum()) == 0
    assert int((dl[B:] != 0).sum()) == 0 and int((dl[:, 10:] != 0).sum()) == 0


@pytest.mark.parametrize("scaled", [True, False], ids=["w0.1", "raw"])
@pytest.mark.parametrize("B", BATCHES)
def test_rowmajor_trajectory(gpu, B, scaled):
    """5 pipelined steps, flush, 4 more through a graph replay, flush: the float64 reference
    trajectory (< 1e-4) and the three-launch trainer, which keeps the transposed factors
    (< 1e-5, stats atol 1e-4, equal accuracy and global_step) -- the bounds of
    test_pipelined_trainer_matches_reference_and_three_launch; then the padding of the
    row-major regions is exactly zero."""
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = _setup(gpu, B, scaled)
    tp = FusedMLPTrainer(p, x, y, B, LR)
    t3 = FusedMLPTrainer(p, x, y, B, LR, pipeline=False)
    assert tp.pipelined and not t3.pipelined
    ref = p.double().cpu()
    xr, yr = x.double().cpu(), y.cpu()
    refs = []
    for s in range(9):
        sl = slice((s % NB) * B, (s % NB + 1) * B)
        g, _, _ = mlp_step.reference_step(ref, xr[sl], yr[sl])
        ref = ref - LR * g
        refs.append(ref)
    tp.run(5, use_graph=False)
    t3.run(5, use_graph=False)
    tp.flush()
    torch.cuda.synchronize()
    e5 = (tp.params.double().cpu() - refs[4]).abs().max().item()
    tp.run(4, use_graph=True)
    t3.run(4, use_graph=True)
    tp.flush()
    torch.cuda.synchronize()
    e9 = (tp.params.double().cpu() - refs[8]).abs().max().item()
    e3 = (tp.params - t3.params).abs().max().item()
    lp, ap = tp.stats()
    l3, a3 = t3.stats()
    print("B=%d scaled=%s: vs f64 after 5 / 9 steps %.3e / %.3e, vs three-launch %.3e, "
          "loss diff %.3e" % (B, scaled, e5, e9, e3, abs(lp - l3)))
    assert e5 < 1e-4 and e9 < 1e-4
    assert tp.global_step() == t3.global_step() == 9
    assert e3 < 1e-5
    assert abs(lp - l3) < 1e-4 and ap == a3
    sp, s3 = tp.stats_range(0, 9), t3.stats_range(0, 9)
    assert torch.allclose(sp, s3, atol=1e-4)
    _assert_padding_zero(tp.ws)


def _one_head(gpu, p, x, y, B):
    """fwdapply (copy + forward) and the single-GPU head on (p, x, y): the workspace."""
    ws = mlp_step.StepWorkspace(B, gpu)
    mlp_step.step_pipelined(p, torch.empty_like(p), x, x, y, ws, LR, apply=False)
    torch.cuda.synchronize()
    return ws


@pytest.mark.parametrize("labels", ["random", 0, 9])
@pytest.mark.parametrize("B", [17, 100, 113])
def test_argmax_ties_go_to_the_lowest_class(gpu, B, labels):
    """W2 / b2 zeroed: all ten logits tie at 0, so the prediction is class 0 (first max, like
    tf.argmax) -- per row accuracy = float(label == 0) -- and the loss is log(10); with random
    labels and with batches whose rows all carry one label."""
    p, x, y = _setup(gpu, B, True)
    p[mlp_step.OFF_W2:].zero_()
    x, y = x[:B].contiguous(), y[:B].contiguous()
    if labels != "random":
        y.fill_(labels)
    ws = _one_head(gpu, p, x, y, B)
    _, dl, rs = _regions(ws)
    assert torch.equal(rs[:B, 1].cpu(), (y == 0).float().cpu())
    assert float((rs[:B, 0] - math.log(10.0)).abs().max()) <= 1e-6
    exp = (0.1 - torch.nn.functional.one_hot(y.long(), 10).float()) / B
    assert float((dl[:B, :10] - exp).abs().max()) <= 1e-7
    _assert_padding_zero(ws, dz_live=False)  # (W2 = 0: dz1 = (dl . W2) h (1 - h) is zero)


@pytest.mark.parametrize("scaled", [True, False], ids=["w0.1", "raw"])
@pytest.mark.parametrize("label", [0, 3, 9])
def test_one_label_batch_matches_reference(gpu, label, scaled):
    """A batch whose rows all carry the same label: per-row loss / prediction and the
    row-major factors against the float64 reference."""
    B = 100
    p, x, y = _setup(gpu, B, scaled)
    x, y = x[:B].contiguous(), y[:B].contiguous()
    y.fill_(label)
    ws = _one_head(gpu, p, x, y, B)
    dz, dl, rs = _regions(ws)
    pr, xr = p.double().cpu(), x.double().cpu()
    W1t, b1, W2t, b2 = mlp_step.unflatten(pr)
    h, logits = mlp_step.reference_forward(pr, xr)
    loss = torch.logsumexp(logits, 1) - logits[:, label]
    dl_ref = (torch.softmax(logits, 1) - torch.nn.functional.one_hot(y.long().cpu(), 10)) / B
    dz_ref = (dl_ref @ W2t) * h * (1 - h)
    top2 = logits.topk(2, 1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3  # rows whose argmax f32 rounding cannot move
    acc = (logits.argmax(1) == label).double()
    assert torch.equal(rs[:B, 1].double().cpu()[clear], acc[clear])
    assert float((rs[:B, 0].double().cpu() - loss).abs().max()) <= 1e-4
    assert float((dl[:B, :10].double().cpu() - dl_ref).abs().max()) <= 1e-6
    assert float((dz[:B, :100].double().cpu() - dz_ref).abs().max()) <= 1e-6


@pytest.mark.parametrize("B", [100, 113])
def test_one_workspace_shared_by_direct_and_pipelined_steps(gpu, B):
    """step_direct (transposed factors) and step_pipelined (row-major factors) alternating on
    ONE workspace: bit-identical parameters to the same sequence on two fresh workspaces (the
    two layouts are regions of their own)."""
    p0, x, y = _setup(gpu, B, True)
    xb = [x[i * B:(i + 1) * B] for i in range(NB)]
    yb = [y[i * B:(i + 1) * B] for i in range(NB)]

    def run(ws_d, ws_p):
        bufs, cur, t = [p0.clone(), torch.empty_like(p0)], 0, 0
        for _ in range(2):
            for k in range(2):  # two pipelined steps and their flush
                mlp_step.step_pipelined(bufs[cur], bufs[cur ^ 1], xb[(t - 1) % NB], xb[t % NB],
                                        yb[t % NB], ws_p, LR, apply=k > 0)
                cur ^= 1
                t += 1
            mlp_step.flush_pipelined(bufs[cur], bufs[cur ^ 1], xb[(t - 1) % NB], ws_p, LR)
            cur ^= 1
            for _k in range(2):  # two three-launch steps
                mlp_step.step_direct(bufs[cur], xb[t % NB], yb[t % NB], ws_d, LR)
                t += 1
        torch.cuda.synchronize()
        return bufs[cur].clone()

    shared = mlp_step.StepWorkspace(B, gpu)
    got = run(shared, shared)
    exp = run(mlp_step.StepWorkspace(B, gpu), mlp_step.StepWorkspace(B, gpu))
    assert torch.equal(got, exp)
    assert not torch.equal(got, p0)
    _assert_padding_zero(shared)


@pytest.mark.parametrize("n", [10, 16])
def test_wave_reduce_scatter(gpu, n):
    """Lane l of the wave ends with the sum over all 64 lanes of value l & 15 (integer-valued
    floats: every order of the sum is exact)."""
    from distributedtensorflowexample_amd.ops._ext import hip, ptr, stream_handle

    g = torch.Generator().manual_seed(n)
    v = torch.randint(-64, 65, (64, n), generator=g).float().to(gpu)
    out = torch.full((64,), float("nan"), device=gpu)
    hip().wave_reduce_scatter_test(ptr(v), ptr(out), n, stream_handle())
    torch.cuda.synchronize()
    sums = v.sum(0).cpu()
    for lane in range(64):
        if lane % 16 < n:
            assert float(out[lane]) == float(sums[lane % 16]), (lane, out.cpu(), sums)
