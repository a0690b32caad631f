"""CPU tier of the layer-kernel tests (tests/layer_reference.py).

(a) The float64 references agree with the project's CPU path (ops/nn.py, ops/cnn.py on CPU
    tensors) on every input set the GPU tests use, within the bounds the GPU kernels are held
    to -- two independent transcriptions of each operation, and the reference alone inside its
    bound -- and the backward formulas agree with torch autograd in float64.
(b) The comparison helpers reject deliberately wrong outputs built from the reference.
(c) The launch arithmetic: every shape reaches the branch its GPU test names, computed from the
    constants in the .hip sources.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_reference as R
from distributedtensorflowexample_amd.ops import cnn, nn

BF = torch.bfloat16


# =========================================================================== (a) softmax
def _xent_check(got, ref, want_grad=True):
    loss, d, correct = got
    assert (d is not None) == want_grad
    R.check_xent(loss, d, correct, ref)


@pytest.mark.parametrize("N,C", R.XENT_SHAPES)
def test_xent_reference_matches_cpu_path(N, C):
    logits, ties = R.xent_logits(N, C)
    R.assert_gaps(logits, ties)
    lab, special = R.xent_int_labels(N, C, ties)
    ref = R.softmax_xent(logits, lab, scale=1.0 / N)
    for r in special.values():  # the rule for an ignored / out-of-range row, on the reference
        assert float(ref.loss[r]) == 0 and float(ref.correct[r]) == 0
        assert not bool(ref.dlogits[r].any())
    for r in ties:  # labelled with the higher tied index: not the arg-max
        assert float(ref.correct[r]) == 0
    _xent_check(nn.softmax_xent_stats(logits, lab), ref)
    lab0, zero_rows = R.xent_int_labels_ignore0(N, C, ties)
    ref0 = R.softmax_xent(logits, lab0, ignore_index=0, scale=1.0 / N)
    for r in zero_rows:
        assert float(ref0.loss[r]) == 0 and not bool(ref0.dlogits[r].any())
    _xent_check(nn.softmax_xent_stats(logits, lab0, ignore_index=0), ref0)
    y, kinds = R.xent_dense_labels(N, C, ties)
    laimed, want = R.aim_logits_at_label_ties(logits, y, kinds, ties)
    R.assert_gaps(laimed, ties)
    refd = R.softmax_xent(laimed, y, scale=1.0 / N)
    assert all(float(refd.correct[r]) == v for r, v in want.items())
    if N >= 12:
        assert set(want.values()) == {0.0, 1.0}
    _xent_check(nn.softmax_xent_stats(laimed, y), refd)
    _xent_check(nn.softmax_xent_stats(laimed, y, want_grad=False), refd, want_grad=False)
    refs = R.softmax_xent(logits, lab, scale=0.37)
    _xent_check(nn.softmax_xent_stats(logits, lab, scale=0.37), refs)


def test_xent_dense_kinds_cover_every_row_kind():
    seen = set()
    for N, C in R.XENT_SHAPES:
        logits, ties = R.xent_logits(N, C)
        y, kinds = R.xent_dense_labels(N, C, ties)
        seen |= set(kinds)
        for r, k in enumerate(kinds):
            want = {"onehot": 1.0, "soft": 1.0, "tie2": 1.0, "sum07": 0.7, "sum13": 1.3, "zero": 0.0}[k]
            assert abs(float(y[r].double().sum()) - want) < 1e-5
    assert seen == set(R.DENSE_KINDS)
    kinds_of = {}
    for N, C in R.XENT_SHAPES:
        _, ties = R.xent_logits(N, C)
        kinds_of[(N, C)] = set(R.xent_int_labels(N, C, ties)[1])
    assert all(kinds_of[s] == set(R.SPECIAL_LABELS) for s in [(5, 10), (301, 10), (7, 64), (6, 65)])


def test_xent_wide_range_cpu_path():
    """Logits in +-40: the f32 CPU path stays far inside the hard limit of the GPU case."""
    N, C = 301, 10
    logits, ties = R.xent_logits(N, C, scale=40.0, seed=1)
    lab, _ = R.xent_int_labels(N, C, ties)
    ref = R.softmax_xent(logits, lab, scale=1.0)
    loss, d, correct = nn.softmax_xent_stats(logits, lab, scale=1.0)
    R.check_close("loss", loss, ref.loss, atol=1e-4)
    R.check_exact("correct", correct, ref.correct)


def test_xent_reference_matches_autograd():
    N, C = 7, 13
    logits, ties = R.xent_logits(N, C)
    lab, _ = R.xent_int_labels(N, C, ties)
    l = logits.double().requires_grad_(True)
    # (torch rejects out-of-range targets: compare the rows it accepts)
    ok = (lab >= 0) & (lab < C) | (lab == -100)
    lab_t = torch.where(ok, lab, torch.full_like(lab, -100)).long()
    loss = F.cross_entropy(l, lab_t, reduction="none", ignore_index=-100)
    (g,) = torch.autograd.grad(loss.sum() * 0.25, l)
    ref = R.softmax_xent(logits, lab, scale=0.25)
    assert torch.allclose(ref.loss, loss.detach(), atol=1e-12)
    assert torch.allclose(ref.dlogits, g, atol=1e-12)
    y, _ = R.xent_dense_labels(N, C, ties)
    l = logits.double().requires_grad_(True)
    lossd = -(y.double() * torch.log_softmax(l, 1)).sum(1)
    (g,) = torch.autograd.grad(lossd.sum() * 0.25, l)
    refd = R.softmax_xent(logits, y, scale=0.25)
    assert torch.allclose(refd.loss, lossd.detach(), atol=1e-12)
    assert torch.allclose(refd.dlogits, g, atol=1e-12)
    assert torch.allclose(refd.probs, torch.softmax(logits.double(), 1), atol=1e-15)


# =========================================================================== (a) activations, dense
@pytest.mark.parametrize("n", R.ACT_SIZES + list(R.ew_wrap_sizes()))
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_activation_reference_matches_cpu_path(n, act):
    x, dy = R.act_inputs(n)
    R.check_close("y", nn.activation(x, act), R.activation(x, act), atol=R.TOL_ACT)
    s = R.activation(x, 1).float() if act == 1 else x
    R.check_close("dz", nn.act_backward(dy, s, act), R.activation_grad(dy, s, act), atol=R.TOL_ACT)


def test_act_inputs_hold_the_special_values():
    for n in R.ACT_SIZES[4:] + list(R.ew_wrap_sizes()):
        x, _ = R.act_inputs(n)
        tail = x[n - (n & 3):]
        for v in R.ACT_SPECIALS:
            hit = (x == v) & (torch.signbit(x) == bool(np.signbit(v)))
            assert bool(hit.any()), (n, v)
        assert n & 3 == 3 and set(tail.tolist()) <= {float(np.float32(v)) for v in R.ACT_SPECIALS}
    assert torch.signbit(R.act_inputs(1)[0])[0] and float(R.act_inputs(1)[0][0]) == 0.0


@pytest.mark.parametrize("act", [1, 2, 3])
def test_activation_grad_matches_autograd(act):
    x, dy = R.act_inputs(1027)
    x = x[x != 0]  # (the ReLU boundary is the reference's stated rule, not autograd's)
    dy = dy[:x.numel()]
    z = x.double().requires_grad_(True)
    y = {1: torch.sigmoid, 2: torch.relu, 3: lambda t: F.gelu(t, approximate="tanh")}[act](z)
    (g,) = torch.autograd.grad((y * dy.double()).sum(), z)
    s = y.detach() if act in (1, 2) else x
    assert torch.allclose(R.activation(x, act), y.detach(), atol=1e-12)
    assert torch.allclose(R.activation_grad(dy, s, act), g, atol=1e-12)
    zero = torch.tensor([0.0, -0.0])
    assert not bool(R.activation_grad(torch.ones(2), zero, 2).any())  # derivative 0 at s == 0


@pytest.mark.parametrize("M,N", R.COLSUM_SHAPES)
@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_colsum_reference_matches_cpu_path(M, N, beta):
    g, out0 = R.colsum_case(M, N)
    ref, mag = R.colsum(g, out0, beta)
    R.check_sum("colsum", nn.colsum(g, out=out0.clone(), beta=beta), ref, mag)


@pytest.mark.parametrize("xshape,act,with_bias", R.DENSE_CASES)
def test_dense_reference_matches_cpu_path(xshape, act, with_bias):
    x, w, b, dy = R.dense_case(xshape, with_bias)
    y64, dx64, dw64, db64 = R.dense(x, w, b, act, dy)
    xs = [t.clone().requires_grad_() if t is not None else None for t in (x, w, b)]
    y = nn.dense(xs[0], xs[1], xs[2], act)
    (y * dy).sum().backward()
    R.check_close("y", y, y64, atol=R.TOL_DENSE_Y)
    for name, t, r in (("dx", xs[0], dx64), ("dw", xs[1], dw64), ("db", xs[2], db64)):
        if t is not None:
            R.check_close(name, t.grad, r, atol=R.TOL_DENSE_GRAD)


# =========================================================================== (a) BatchNorm
ALL_BN = R.BN_SETS + [R.BN_LARGE]


@pytest.mark.parametrize("M,C", ALL_BN)
def test_bn_reference_matches_cpu_path(M, C):
    c = R.bn_case(M, C)
    modes = [(True, True)] if (M, C) == R.BN_LARGE else [(r, a) for r in (True, False)
                                                         for a in (True, False)]
    for with_res, relu in modes:
        ref, mag = R.bn_apply_ref(M, C, with_res, relu)
        y = cnn.bn_apply(c.x, c.mean, c.rstd, c.gamma, c.beta, c.res if with_res else None, relu)
        R.check_bf16("bn_apply res=%s relu=%s" % (with_res, relu), y, ref, mag)
    for relu in ((True,) if (M, C) == R.BN_LARGE else (True, False)):
        ref = R.bn_bwd_ref(M, C, relu)
        dg, db = torch.zeros(C), torch.zeros(C)
        dx, dres = cnn.bn_bwd(c.dy, c.y, c.x, c.mean, c.rstd, c.gamma, dg, db, relu, True)
        R.check_bf16("dx relu=%s" % relu, dx, ref.dx, ref.mag_dx)
        R.check_exact("dres", dres, ref.dres)
        R.check_sum("dgamma", dg, ref.sum_dyxh, ref.mag_dyxh)
        R.check_sum("dbeta", db, ref.sum_dy, ref.mag_dy)


@pytest.mark.parametrize("M,C", [(100, 96), (60, 96), (197, 8)])
def test_bn_apply_stats_reference_matches_cpu_path(M, C):
    c = R.bn_case(M, C)
    rm0, rv0 = R.randn(C, seed=1) * 0.5, torch.rand(C, generator=torch.Generator().manual_seed(2)) + 0.5
    fin = R.bn_finalize(c.s, c.q, M, 1e-5, rm0, rv0, 0.9)
    ref, mag = R.bn_apply(c.x, fin.mean, fin.rstd, c.gamma, c.beta, c.res, True)
    rm, rv = rm0.clone(), rv0.clone()
    y, mean, rstd = cnn.bn_apply_stats(c.x, c.s, c.q, M, c.gamma, c.beta, c.res, True, 1e-5, rm, rv)
    R.check_bf16("y", y, ref, mag)
    R.check_close("mean", mean, fin.mean, atol=R.TOL_MEAN)
    R.check_close("rstd", rstd, fin.rstd, atol=1e-8, rtol=R.TOL_RSTD)
    R.check_close("run_mean", rm, fin.run_mean, atol=R.TOL_MEAN)
    R.check_close("run_var", rv, fin.run_var, atol=1e-8, rtol=R.TOL_RSTD)


@pytest.mark.parametrize("C,M,clamp", R.BN_FINALIZE_CASES)
def test_bn_finalize_reference_matches_cpu_path(C, M, clamp):
    s, q, rm0, rv0 = R.bn_finalize_case(C, M, clamp)
    fin = R.bn_finalize(s, q, M, 1e-5, rm0, rv0, 0.9)
    rm, rv = rm0.clone(), rv0.clone()
    mean, rstd = cnn.bn_finalize(s, q, M, 1e-5, rm, rv, 0.9)
    R.check_close("mean", mean, fin.mean, atol=R.TOL_MEAN)
    R.check_close("rstd", rstd, fin.rstd, atol=1e-8, rtol=R.TOL_RSTD)
    R.check_close("run_mean", rm, fin.run_mean, atol=R.TOL_MEAN)
    R.check_close("run_var", rv, fin.run_var, atol=1e-8, rtol=R.TOL_RSTD)
    if clamp:
        assert float(fin.var[0]) == 0.0 and abs(float(fin.rstd[0]) - R.f32(1e-5) ** -0.5) < 1e-9
    if M == 1:
        assert not bool(fin.var.any())
        assert torch.equal(fin.run_var, R.f32(0.9) * rv0.double())  # unbias = 1, var = 0


def test_clamp_channel_rounds_negative_in_float32():
    """The clamp case's premise: M equal values of CLAMP_VALUE have exact f32 sums, an exact
    variance of 0, and q / M - mean^2 negative in float32 for every contraction of the kernel's
    expression (and not positive on the CPU path), with the mean inside its bound."""
    v, M = R.CLAMP_VALUE, R.CLAMP_M
    s, q = np.float32(v * M), np.float32(v * v * M)
    assert float(s) == v * M and float(q) == v * v * M
    var, mu, mu_div = R.f32_variances(s, q, M)
    assert all(x < 0 for x in var[:3]) and var[3] <= 0, var
    assert abs(mu - v) < R.TOL_MEAN and abs(mu_div - v) < R.TOL_MEAN
    sc, qc, _, _ = R.bn_finalize_case(64, M, True)
    assert float(sc[0]) == v * M and float(qc[0]) == v * v * M


def test_bn_backward_matches_autograd():
    """relu(bn(x) + res) with the batch statistics inside the graph, float64."""
    M, C = 37, 16
    x = (R.randn(M, C, seed=1) * 2 + 1).double().requires_grad_(True)
    res = R.randn(M, C, seed=2).double().requires_grad_(True)
    gamma = (R.randn(C, seed=3) * 0.1 + 1).double().requires_grad_(True)
    beta = (R.randn(C, seed=4) * 0.1).double().requires_grad_(True)
    dy = R.randn(M, C, seed=5).double()
    for relu in (True, False):
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
        rstd = 1.0 / torch.sqrt(var + 1e-5)
        z = (x - mean) * rstd * gamma + beta + res
        y = torch.relu(z) if relu else z
        gx, gr, gg, gb = torch.autograd.grad((y * dy).sum(), [x, res, gamma, beta])
        fin = R.bn_finalize(x.detach().sum(0), (x.detach() ** 2).sum(0), M, 1e-5)
        assert torch.allclose(fin.mean, mean.detach(), atol=1e-12)
        assert torch.allclose(fin.rstd, rstd.detach(), rtol=1e-6)  # (eps rounded to f32)
        ref = R.bn_bwd(dy, y.detach(), x.detach(), mean.detach(), rstd.detach(), gamma.detach(), relu)
        yr, _ = R.bn_apply(x.detach(), mean.detach(), rstd.detach(), gamma.detach(), beta.detach(),
                           res.detach(), relu)
        assert torch.allclose(yr, y.detach(), atol=1e-12)
        assert torch.allclose(ref.dx, gx, atol=1e-10)
        assert torch.allclose(ref.dres, gr, atol=1e-12)
        assert torch.allclose(ref.sum_dyxh, gg, atol=1e-10)
        assert torch.allclose(ref.sum_dy, gb, atol=1e-10)


# =========================================================================== (a) pools
ALL_POOL = [(s, k) for s in R.MAXPOOL_SHAPES for k in R.MAXPOOL_KINDS] + [(R.MAXPOOL_ROWLOOP, "ties")]


@pytest.mark.parametrize("shape,kind", ALL_POOL)
def test_maxpool_reference_matches_cpu_path(shape, kind):
    x, dy = R.maxpool_case(shape, kind)
    yr, idxr, dxr = R.maxpool_ref(shape, kind)
    y, idx = cnn.maxpool_fwd(x)
    R.check_exact("y", y, yr)
    R.check_exact("idx", idx, idxr)  # the first maximal tap, ties included
    R.check_bf16("dx", cnn.maxpool_bwd(dy, idx, shape), dxr)
    if kind == "negative":
        assert float(yr.max()) < 0


def test_maxpool_tie_inputs_tie():
    """Most windows of the {0, 0.5, 1} image hold their maximum more than once."""
    shape = (2, 15, 16, 64)
    x, _ = R.maxpool_case(shape, "ties")
    y, idx = R.maxpool_fwd(x)
    xp = F.pad(x.float().permute(0, 3, 1, 2), (1, 1, 1, 1), value=float("-inf"))
    cols = F.unfold(xp, 3, stride=2).view(2, 64, 9, -1)
    multi = (cols == cols.max(2, keepdim=True).values).sum(2) > 1
    assert float(multi.float().mean()) > 0.5


def test_maxpool_reference_matches_autograd_without_ties():
    shape = (2, 15, 16, 64)
    x, dy = R.maxpool_case(shape, "random")
    xs = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    y = F.max_pool2d(xs, 3, 2, 1)
    # tie-free: every window's maximum is unique, so torch's choice is the only one
    xp = F.pad(x.float().permute(0, 3, 1, 2), (1, 1, 1, 1), value=float("-inf"))
    cols = F.unfold(xp, 3, stride=2).view(2, 64, 9, -1)
    keep = ((cols == cols.max(2, keepdim=True).values).sum(2) == 1).view(2, 64, 8, 8)
    g = dy.double().permute(0, 3, 1, 2) * keep
    (gx,) = torch.autograd.grad((y * g).sum(), xs)
    yr, idxr = R.maxpool_fwd(x)
    assert torch.equal(yr, y.detach().permute(0, 2, 3, 1))
    dxr = R.maxpool_bwd(g.permute(0, 2, 3, 1), idxr, shape)
    assert torch.allclose(dxr, gx.permute(0, 2, 3, 1), atol=1e-12)
    assert float(keep.double().mean()) > 0.9


@pytest.mark.parametrize("shape", R.AVGPOOL_SHAPES + [R.AVGPOOL_BWD_WRAP])
def test_avgpool_reference_matches_cpu_path(shape):
    x, dy = R.avgpool_case(shape)
    if shape != R.AVGPOOL_BWD_WRAP:
        ref, mag = R.avgpool_fwd(x)
        R.check_bf16("y", cnn.avgpool_fwd(x), ref, mag)
    dref = R.avgpool_bwd(dy, shape)
    R.check_bf16("dx", cnn.avgpool_bwd(dy, shape), dref, dref.abs())
    xs = x[:1].double().requires_grad_(True)
    (g,) = torch.autograd.grad((xs.mean((1, 2)) * dy[:1].double()).sum(), xs)
    assert torch.allclose(R.avgpool_bwd(dy[:1], (1,) + shape[1:]), g, atol=1e-15)


# =========================================================================== (b) teeth
def _rejects(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


def test_rejects_unwritten_scalar_tail():
    n = 1027
    x, dy = R.act_inputs(n)
    for act in (1, 2, 3):
        ref = R.activation(x, act)
        R.check_close("y", ref.float(), ref, atol=R.TOL_ACT)
        out = ref.float()
        out[n - (n & 3):] = 7.0  # what an output buffer held before
        _rejects(R.check_close, "y", out, ref, atol=R.TOL_ACT)
        out = ref.float()
        out[-1] = 7.0
        _rejects(R.check_close, "y", out, ref, atol=R.TOL_ACT)


def test_rejects_unwritten_last_row_of_partial_block():
    N, C = 301, 10
    assert N % R.launch_constants().xent_rows == 1
    logits, ties = R.xent_logits(N, C)
    lab, _ = R.xent_int_labels(N, C, ties)
    ref = R.softmax_xent(logits, lab, scale=1.0 / N)
    good = (ref.loss.float(), ref.dlogits.float(), ref.correct.float())
    _xent_check(good, ref)
    loss = good[0].clone()
    loss[-1] = -1.0
    _rejects(_xent_check, (loss, good[1], good[2]), ref)
    d = good[1].clone()
    d[-1] = -1.0
    _rejects(_xent_check, (good[0], d, good[2]), ref)
    # a write past row N - 1: the sentinel element after the end
    _rejects(R.check_exact, "sentinel", torch.tensor([0.0]), torch.tensor([-7.0]))


def test_rejects_gradient_on_ignored_row_and_wrong_tie():
    N, C = 301, 10
    logits, ties = R.xent_logits(N, C)
    lab, special = R.xent_int_labels(N, C, ties)
    ref = R.softmax_xent(logits, lab, scale=1.0 / N)
    for r in special.values():
        d = ref.dlogits.float()
        d[r] = (ref.probs[r] * ref.scale).float()  # softmax - 0: the mask forgotten
        _rejects(_xent_check, (ref.loss.float(), d, ref.correct.float()), ref)
        loss = ref.loss.float()
        loss[r] = float(torch.logsumexp(logits[r].double(), 0) - logits[r, 0].double())
        _rejects(_xent_check, (loss, ref.dlogits.float(), ref.correct.float()), ref)
    (r, (a, b)), = ties.items()
    correct = ref.correct.float()
    correct[r] = 1.0  # arg-max taken at the higher tied index, which is the label
    assert int(lab[r]) == b
    _rejects(_xent_check, (ref.loss.float(), ref.dlogits.float(), correct), ref)
    # the same for the dense labels' own tie
    y, kinds = R.xent_dense_labels(N, C, ties)
    refd = R.softmax_xent(logits, y, scale=1.0 / N)
    r = kinds.index("tie2")
    hi = int(torch.where(y[r] == y[r].max())[0][1])
    l2 = logits.clone()
    l2[r, hi] = l2[r].max() + 1.0  # the logits' arg-max is the HIGHER of the two equal labels
    assert float(R.softmax_xent(l2, y).correct[r]) == 0.0
    wrong = R.softmax_xent(l2, y).correct.clone()
    wrong[r] = 1.0
    _rejects(R.check_exact, "correct", wrong, R.softmax_xent(l2, y).correct)


def test_rejects_maxpool_tie_to_later_tap_and_zero_padding():
    shape = (2, 15, 16, 64)
    x, dy = R.maxpool_case(shape, "ties")
    y, idx, dx = R.maxpool_ref(shape, "ties")
    # the LAST maximal tap instead of the first: same y, another idx and another dx
    N, H, W, C = shape
    xp = F.pad(x.double().permute(0, 3, 1, 2), (1, 1, 1, 1), value=float("-inf"))
    cols = F.unfold(xp, 3, stride=2).view(N, C, 9, -1)
    last = torch.where(cols == cols.max(2, keepdim=True).values,
                       torch.arange(9).view(1, 1, 9, 1), torch.full((1,), -1)).max(2).values
    idx_last = last.view(N, C, 8, 8).permute(0, 2, 3, 1).to(torch.uint8)
    assert torch.equal(cols.gather(2, last[:, :, None]).view(N, C, 8, 8).permute(0, 2, 3, 1), y)
    _rejects(R.check_exact, "idx", idx_last, idx)
    _rejects(R.check_bf16, "dx", R.maxpool_bwd(dy, idx_last, shape).to(BF), dx)
    R.check_bf16("dx", dx.to(BF), dx)
    # padding treated as 0 in an all-negative image: border windows return 0
    xn, _ = R.maxpool_case(shape, "negative")
    yn, idxn, _ = R.maxpool_ref(shape, "negative")
    xz = F.pad(xn.double().permute(0, 3, 1, 2), (1, 1, 1, 1), value=0.0)
    yz = F.max_pool2d(xz, 3, 2, 0).permute(0, 2, 3, 1)
    assert float(yz.max()) == 0.0
    _rejects(R.check_exact, "y", yz, yn)
    R.check_exact("y", yn.to(BF), yn)


def test_rejects_wrong_channel_coefficients_and_late_residual():
    M, C = 197, 64
    c = R.bn_case(M, C)
    ref, mag = R.bn_apply_ref(M, C, True, True)
    R.check_bf16("y", ref.to(BF), ref, mag)
    roll = lambda t: torch.roll(t, -8)  # noqa: E731  (channel c with the coefficients of c + 8)
    wrong, _ = R.bn_apply(c.x, roll(c.mean), roll(c.rstd), roll(c.gamma), roll(c.beta), c.res, True)
    _rejects(R.check_bf16, "y", wrong.to(BF), ref, mag)
    only_affine, _ = R.bn_apply(c.x, c.mean, c.rstd, roll(c.gamma), roll(c.beta), c.res, True)
    _rejects(R.check_bf16, "y", only_affine.to(BF), ref, mag)
    late = R.bn_apply(c.x, c.mean, c.rstd, c.gamma, c.beta, None, True)[0] + c.res.double()
    _rejects(R.check_bf16, "y", late.to(BF), ref, mag)
    # half a bf16 ulp more than rounding allows is already out
    off = (ref * (1 + 1.6 * R.BF16_ULP)).to(BF)
    _rejects(R.check_bf16, "y", off, ref, mag)


def test_rejects_dropped_second_channel_pass():
    M, C = 37, 2056
    assert R.bn_bwd_reduce_plan(M, C).passes == 2
    c = R.bn_case(M, C)
    ref = R.bn_bwd_ref(M, C, True)
    R.check_sum("dbeta", ref.sum_dy.float(), ref.sum_dy, ref.mag_dy)
    R.check_sum("dgamma", ref.sum_dyxh.float(), ref.sum_dyxh, ref.mag_dyxh)
    dropped = ref.sum_dy.float()
    dropped[2048:] = 0.0
    _rejects(R.check_sum, "dbeta", dropped, ref.sum_dy, ref.mag_dy)
    # and the dx formed from such sums
    A = (c.gamma * c.rstd).double()
    xh = (c.x.double() - c.mean.double()) * c.rstd.double()
    dx = A * (ref.dres - dropped.double() / M - xh * ref.sum_dyxh / M)
    _rejects(R.check_bf16, "dx", dx.to(BF), ref.dx, ref.mag_dx)
    R.check_bf16("dx", ref.dx.to(BF), ref.dx, ref.mag_dx)
    # a masked copy that is not exact
    bad = ref.dres.clone()
    bad[0, 0] = bad[0, 0] * (1 + R.BF16_ULP) + 1e-3
    _rejects(R.check_exact, "dres", bad, ref.dres)
    # a column sum that lost one row
    g, out0 = R.colsum_case(257, 64)
    full, mag = R.colsum(g, out0, 0.5)
    _rejects(R.check_sum, "colsum", R.colsum(g[:-1], out0, 0.5)[0], full, mag)
    _rejects(R.check_sum, "colsum", R.colsum(g, out0, 0.0)[0], full, mag)


# =========================================================================== (c) reach
def test_reach_softmax_and_elementwise():
    k = R.launch_constants()
    assert k.xent_rows == 4
    partial = [N for N, _ in R.XENT_SHAPES if N % k.xent_rows]
    assert set(partial) == {1, 5, 301, 7, 6, 3, 2}
    assert any(C > 64 for _, C in R.XENT_SHAPES)  # a second trip of the per-lane column loop
    assert [n & 3 for n in R.ACT_SIZES] == [1, 3, 0, 1, 3, 3]
    full, wrap = R.ew_wrap_sizes()
    assert full == 2097155 and wrap == 2097159 and full & 3 == wrap & 3 == 3
    assert R.ew_passes(full) == (k.ew_cap, 1)   # fills the capped grid exactly: one pass
    assert R.ew_passes(wrap) == (k.ew_cap, 2)   # the smallest n with a second grid-stride pass
    assert R.ew_passes(1027) == (1, 1) and 1027 >> 2 == k.ew_block  # one full block + the tail


def test_reach_colsum():
    k = R.launch_constants()
    shapes = dict((s, ((s[1] + k.colsum_cols - 1) // k.colsum_cols, s[1] % k.colsum_cols, s[0]))
                  for s in R.COLSUM_SHAPES)
    assert shapes[(1, 1)] == (1, 1, 1) and shapes[(3, 70)][0] == 2 and shapes[(50, 129)][0] == 3
    assert shapes[(3, 70)][2] < k.colsum_groups  # idle row groups
    assert shapes[(257, 64)][1] == 0 and 257 % k.colsum_groups


def test_reach_batchnorm():
    k = R.launch_constants()
    assert k.ew_u == 2
    paths = {mc: R.bn_stream_path(*mc) for mc in R.BN_SETS + [R.BN_LARGE]}
    assert paths[(100, 96)] == "fast" and 96 // 8 == 12          # non-power-of-two group count
    assert paths[(60, 96)] == "general"
    assert (R.grid_once(100 * 12) * 256) % 12 == 0 and (R.grid_once(60 * 12) * 256) % 12 != 0
    assert paths[(37, 2056)] == "general" and paths[(197, 64)] == "fast" and paths[(197, 8)] == "fast"
    # the existing test_batchnorm_apply_from_sums case C = 96, M = 252 is the FAST path
    assert R.bn_stream_path(252, 96) == "fast"
    p8, p8b = R.bn_bwd_reduce_plan(197, 8), R.bn_bwd_reduce_plan(1500, 8)
    assert p8.rpp == 256 and p8.blocks == 1 and p8b.blocks == 2 and not p8b.from_m
    p96 = R.bn_bwd_reduce_plan(100, 96)
    assert p96.tpr == 12 and p96.rpp == 21 and 256 % 12  # idle threads in the last partial row
    assert R.bn_bwd_reduce_plan(37, 2056).passes == 2 and R.bn_bwd_reduce_plan(197, 64).passes == 1
    big = R.bn_bwd_reduce_plan(*R.BN_LARGE)
    assert big.from_m and big.rpb == 129 and big.blocks == 1017
    assert not R.bn_bwd_reduce_plan(R.BN_LARGE[0] - 77, 64).from_m  # M = 131072: still rpp * 4
    assert R.bn_bwd_reduce_plan(131073, 64).from_m                   # the threshold itself
    for C, M, _ in R.BN_FINALIZE_CASES:
        assert C in (1, 64, 257)
    assert 257 % k.fin_block and 257 > k.fin_block


def test_reach_pools():
    k = R.launch_constants()
    plans = {s: R.maxpool_plan(s) for s in R.MAXPOOL_SHAPES + [R.MAXPOOL_ROWLOOP]}
    assert plans[(1, 16, 16, 264)].xblocks_fwd == 2 and plans[(1, 16, 16, 264)].xblocks_bwd == 3
    assert all(p.xblocks_fwd == 1 for s, p in plans.items() if s != (1, 16, 16, 264))
    assert not any(p.loops_fwd or p.loops_bwd for s, p in plans.items() if s != R.MAXPOOL_ROWLOOP)
    N, H, W, C = R.MAXPOOL_ROWLOOP
    assert plans[R.MAXPOOL_ROWLOOP].loops_fwd and plans[R.MAXPOOL_ROWLOOP].loops_bwd
    assert N * R.pool_out(H) == k.pool_rows_fwd + 1 and C == 8 and W == 2
    for N, H, W, C in R.AVGPOOL_SHAPES:
        assert (N * C) % k.avg_block
    assert any(C % 8 for _, _, _, C in R.AVGPOOL_SHAPES) and any(H * W == 1 for _, H, W, _ in R.AVGPOOL_SHAPES)
    N, H, W, C = R.AVGPOOL_BWD_WRAP
    assert N * H * W * C == 2102784 and R.grid_for_passes(N * H * W * C) == (k.for_cap, 2)
    assert R.grid_for_passes(2 * 15 * 16 * 64)[1] == 1
