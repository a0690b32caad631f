"""softmax_xent.hip, elementwise.hip, colsum_kernel and nn.dense against the float64 references
of tests/layer_reference.py, at the shapes that reach each kernel's tail, loop-around, alternate
branch and tie rule (1 GPU).  The same input sets and comparison helpers run on the project's CPU
path in tests/test_layer_reference_cpu.py, which also asserts the reach arithmetic.

Bounds (layer_reference): loss rows 1e-5, probabilities and dlogits / scale 3e-5, activations
1e-5, dense gradients 1e-4 (the project's bounds at logits in +-5: fast exp / log / tanh set
them); column sums 2^-20 sum|terms|; ``correct`` and every sentinel exactly."""
import pytest
import torch

import layer_reference as R
from distributedtensorflowexample_amd.ops import nn
from distributedtensorflowexample_amd.ops._ext import hip, ptr, stream_handle

pytestmark = pytest.mark.gpu

SENT = -7.0  # never a loss, a probability or a 0 / 1 flag


def _raw_xent(gpu, logits, labels, pad, ignore_index, scale, only_probs=False):
    """The raw binding with row strides ldl = ldy = ldd = C + pad, loss / correct one element
    longer than N and a probs buffer one element longer than N * C, all pre-filled with SENT."""
    N, C = logits.shape
    ld = C + pad
    lbuf = torch.full((N, ld), 99.0)
    lbuf[:, :C] = logits
    lbuf = lbuf.to(gpu)
    lab = ybuf = None
    if labels.dtype.is_floating_point:
        ybuf = torch.full((N, ld), 55.0)
        ybuf[:, :C] = labels
        ybuf = ybuf.to(gpu)
    else:
        lab = labels.to(torch.int32).to(gpu)
    loss = torch.full((N + 1,), SENT, device=gpu)
    correct = torch.full((N + 1,), SENT, device=gpu)
    d = torch.full((N, ld), SENT, device=gpu)
    probs = torch.full((N * C + 1,), SENT, device=gpu)
    nul = only_probs
    hip().softmax_xent(N, C, ptr(lbuf), ld, ptr(lab), ptr(ybuf), ld, int(ignore_index), float(scale),
                       0 if nul else ptr(loss), 0 if nul else ptr(d), ld,
                       0 if nul else ptr(correct), ptr(probs), stream_handle())
    torch.cuda.synchronize()
    return loss.cpu(), d.cpu(), correct.cpu(), probs.cpu()


def _check_raw(out, ref, N, C, only_probs=False):
    loss, d, correct, probs = out
    R.check_exact("probs sentinel", probs[N * C:], torch.tensor([SENT]))
    R.check_close("probs", probs[:N * C].view(N, C), ref.probs, atol=R.TOL_PROB)
    if only_probs:  # null loss / correct / dlogits: nothing else is written
        for name, t in (("loss", loss), ("correct", correct), ("dlogits", d)):
            R.check_exact(name + " untouched", t, torch.full_like(t, SENT))
        return
    # the partial last block writes nothing past row N - 1; padding columns come back untouched
    R.check_exact("loss sentinel", loss[N:], torch.tensor([SENT]))
    R.check_exact("correct sentinel", correct[N:], torch.tensor([SENT]))
    R.check_exact("dlogits padding", d[:, C:], torch.full_like(d[:, C:], SENT))
    R.check_xent(loss[:N], d[:, :C], correct[:N], ref)


@pytest.mark.parametrize("N,C", R.XENT_SHAPES)
def test_xent_int_labels(gpu, N, C):
    """Partial last block (every N here has N % 4 != 0), a second trip of the column loop
    (C > 64), ignored (-100) and out-of-range (-1, C, C + 3) rows, arg-max ties at (c, c + 1)
    and (c, c + 64): lowest index wins."""
    assert N % R.launch_constants().xent_rows != 0
    logits, ties = R.xent_logits(N, C)
    R.assert_gaps(logits, ties)
    lab, special = R.xent_int_labels(N, C, ties)
    if N >= 5:
        assert set(special) == set(R.SPECIAL_LABELS)
    ref = R.softmax_xent(logits, lab, scale=1.0 / N)
    L = logits.to(gpu)
    loss, d, correct = nn.softmax_xent_stats(L, lab.to(gpu))
    R.check_xent(loss, d, correct, ref)
    assert torch.equal(L.cpu(), logits)
    # the same through the raw binding: sentinels after the end, and the probs output
    _check_raw(_raw_xent(gpu, logits, lab, 0, -100, 1.0 / N), ref, N, C)


@pytest.mark.parametrize("N,C", R.XENT_SHAPES)
def test_xent_ignore_index_zero(gpu, N, C):
    """A non-negative ignore_index: rows labelled 0 are ignored, the others are not."""
    logits, ties = R.xent_logits(N, C)
    lab, zero_rows = R.xent_int_labels_ignore0(N, C, ties)
    assert (zero_rows or N == 2) and all(int(lab[r]) == 0 for r in zero_rows)  # (N = 2: tie rows)
    ref = R.softmax_xent(logits, lab, ignore_index=0, scale=1.0 / N)
    loss, d, correct = nn.softmax_xent_stats(logits.to(gpu), lab.to(gpu), ignore_index=0)
    R.check_xent(loss, d, correct, ref)
    for r in zero_rows:
        assert float(loss[r]) == 0.0 and float(correct[r]) == 0.0 and not bool(d[r].any())


@pytest.mark.parametrize("N,C", R.XENT_SHAPES)
def test_xent_dense_labels(gpu, N, C):
    """One-hot rows, soft rows summing to 1 / 0.7 / 1.3 (ysum != 1), an all-zero row, a row
    whose two largest labels are equal (lowest index is the label's arg-max), logit ties."""
    logits, ties = R.xent_logits(N, C)
    y, kinds = R.xent_dense_labels(N, C, ties)
    logits, want = R.aim_logits_at_label_ties(logits, y, kinds, ties)
    R.assert_gaps(logits, ties)
    ref = R.softmax_xent(logits, y, scale=1.0 / N)
    assert all(float(ref.correct[r]) == v for r, v in want.items())
    loss, d, correct = nn.softmax_xent_stats(logits.to(gpu), y.to(gpu))
    R.check_xent(loss, d, correct, ref)
    _check_raw(_raw_xent(gpu, logits, y, 0, -1, 1.0 / N), ref, N, C)


@pytest.mark.parametrize("dense_labels", [False, True])
def test_xent_no_grad_and_scale(gpu, dense_labels):
    N, C = 301, 10
    logits, ties = R.xent_logits(N, C)
    lab = R.xent_dense_labels(N, C, ties)[0] if dense_labels else R.xent_int_labels(N, C, ties)[0]
    ref = R.softmax_xent(logits, lab, scale=0.37)
    loss, d, correct = nn.softmax_xent_stats(logits.to(gpu), lab.to(gpu), want_grad=False)
    assert d is None
    R.check_xent(loss, None, correct, ref)
    loss, d, correct = nn.softmax_xent_stats(logits.to(gpu), lab.to(gpu), scale=0.37)
    R.check_xent(loss, d, correct, ref)


@pytest.mark.parametrize("N,C", [(301, 10), (6, 65)])
@pytest.mark.parametrize("dense_labels", [False, True])
def test_xent_raw_binding_row_strides(gpu, N, C, dense_labels):
    """ldl = ldy = ldd = C + 3 through _ext.hip().softmax_xent: padding columns of dlogits come
    back untouched, probs matches, and a run with only probs given writes nothing else."""
    logits, ties = R.xent_logits(N, C)
    lab = R.xent_dense_labels(N, C, ties)[0] if dense_labels else R.xent_int_labels(N, C, ties)[0]
    ref = R.softmax_xent(logits, lab, scale=0.5)
    _check_raw(_raw_xent(gpu, logits, lab, 3, -100, 0.5), ref, N, C)
    _check_raw(_raw_xent(gpu, logits, lab, 3, -100, 0.5, only_probs=True), ref, N, C, only_probs=True)


# Logits in +-40 (N = 301, C = 10, int labels, scale 1): the fast exponential's error grows with
# its argument.  Largest errors measured on an MI355X against the float64 reference, and the
# bounds set to four times them: loss rows 5.195e-06 -> 2.078e-05 (one float32 ulp of a loss
# near 40 is 3.8e-06), probabilities and dlogits 1.752e-07 -> 7.008e-07.
WIDE_SEEN = {"loss": 5.195e-06, "prob": 1.752e-07}
WIDE_HARD_LIMIT = 1e-4  # a fast-math exp does not explain a loss error above this


def test_xent_wide_range(gpu):
    N, C = 301, 10
    logits, ties = R.xent_logits(N, C, scale=40.0, seed=1)
    R.assert_gaps(logits, ties)
    lab, _ = R.xent_int_labels(N, C, ties)
    ref = R.softmax_xent(logits, lab, scale=1.0)
    loss, d, correct, probs = _raw_xent(gpu, logits, lab, 0, -100, 1.0)
    e_loss = float((loss[:N].double() - ref.loss).abs().max())
    e_prob = max(float((probs[:N * C].view(N, C).double() - ref.probs).abs().max()),
                 float((d.double() - ref.dlogits).abs().max()))
    print("wide-range softmax_xent: loss err %.3e, prob / dlogits err %.3e" % (e_loss, e_prob))
    assert e_loss <= WIDE_HARD_LIMIT, e_loss
    R.check_exact("correct", correct[:N], ref.correct)
    R.check_xent(loss[:N], d, correct[:N], ref, probs[:N * C].view(N, C),
                 tol_loss=4 * WIDE_SEEN["loss"], tol_prob=4 * WIDE_SEEN["prob"])


# ------------------------------------------------------------------ activations
@pytest.mark.parametrize("n", R.ACT_SIZES + list(R.ew_wrap_sizes()))
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_activation_fwd_bwd(gpu, n, act):
    """nn.activation / nn.act_backward: the scalar tail (n & 3), a lone tail (n < 4), the
    capped grid filled exactly (2048 * 256 * 4 + 3) and its second grid-stride pass (+ 7), every
    activation id; exact 0 / -0 (ReLU boundary), +-30 (saturation), +-1e-3; inputs unchanged."""
    full, wrap = R.ew_wrap_sizes()
    if n == full:
        assert R.ew_passes(n) == (R.launch_constants().ew_cap, 1) and n & 3 == 3
    if n == wrap:
        assert R.ew_passes(n) == (R.launch_constants().ew_cap, 2) and n & 3 == 3
    x, dy = R.act_inputs(n)
    X = x.to(gpu)
    y = nn.activation(X, act)
    assert y.shape == X.shape and y.data_ptr() != X.data_ptr()
    R.check_close("y", y, R.activation(x, act), atol=R.TOL_ACT)
    assert torch.equal(X.cpu(), x) and bool(torch.equal(torch.signbit(X.cpu()), torch.signbit(x)))
    s = R.activation(x, 1).float() if act == 1 else x
    DY, S = dy.to(gpu), s.to(gpu)
    dz = nn.act_backward(DY, S, act)
    R.check_close("dz", dz, R.activation_grad(dy, s, act), atol=R.TOL_ACT)
    assert torch.equal(DY.cpu(), dy) and torch.equal(S.cpu(), s)


@pytest.mark.parametrize("act", [1, 2, 3])
def test_activation_misaligned_and_strided_views(gpu, act):
    """A view 4 bytes off a 16-byte boundary and a strided view go through nn._aligned's copy:
    same values as a contiguous copy, the underlying buffers unchanged."""
    n = 1027
    x, dy = R.act_inputs(n)
    buf = torch.cat([torch.tensor([123.0]), x]).to(gpu)
    dbuf = torch.cat([torch.tensor([321.0]), dy]).to(gpu)
    off, doff = buf[1:], dbuf[1:]
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    wide = torch.stack([x, x + 1.0], dim=1).to(gpu)
    dwide = torch.stack([dy, dy - 1.0], dim=1).to(gpu)
    strided, dstrided = wide[:, 0], dwide[:, 0]
    assert not strided.is_contiguous()
    want = nn.activation(x.to(gpu), act)
    want_b = nn.act_backward(dy.to(gpu), x.to(gpu), act)
    R.check_close("y", want, R.activation(x, act), atol=R.TOL_ACT)
    for v, dv in ((off, doff), (strided, dstrided)):
        assert torch.equal(nn.activation(v, act), want)
        assert torch.equal(nn.act_backward(dv, v, act), want_b)
    assert torch.equal(buf.cpu(), torch.cat([torch.tensor([123.0]), x]))
    assert torch.equal(dbuf.cpu(), torch.cat([torch.tensor([321.0]), dy]))
    assert torch.equal(wide.cpu(), torch.stack([x, x + 1.0], dim=1))
    assert torch.equal(dwide.cpu(), torch.stack([dy, dy - 1.0], dim=1))


# ------------------------------------------------------------------ column sum, dense
@pytest.mark.parametrize("M,N", R.COLSUM_SHAPES)
@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_colsum(gpu, M, N, beta):
    """colsum_kernel: beta != 0 into a pre-filled out (beta == 0 must not read it: NaN there),
    two and three column blocks, N % 64 != 0, M < 4 (idle row groups), M % 4 != 0."""
    g, out0 = R.colsum_case(M, N)
    ref, mag = R.colsum(g, out0, beta)
    out = out0.to(gpu) if beta else torch.full((N,), float("nan"), device=gpu)
    G = g.to(gpu)
    got = nn.colsum(G, out=out, beta=beta)
    assert got.data_ptr() == out.data_ptr()
    R.check_sum("colsum", got, ref, mag)
    assert torch.equal(G.cpu(), g)
    R.check_sum("colsum (fresh out)", nn.colsum(G), *R.colsum(g))


@pytest.mark.parametrize("xshape,act,with_bias", R.DENSE_CASES)
def test_dense_autograd_acts_bias_3d(gpu, xshape, act, with_bias):
    """nn.dense forward / backward for relu, gelu (second GEMM for the pre-activation), no bias
    and a 3-D input, against float64 autograd."""
    x, w, b, dy = R.dense_case(xshape, with_bias)
    y64, dx64, dw64, db64 = R.dense(x, w, b, act, dy)
    xs = [t.to(gpu).requires_grad_() if t is not None else None for t in (x, w, b)]
    y = nn.dense(xs[0], xs[1], xs[2], act)
    assert tuple(y.shape) == tuple(xshape[:-1]) + (R.DENSE_OUT,)
    (y * dy.to(gpu)).sum().backward()
    R.check_close("y", y, y64, atol=R.TOL_DENSE_Y)
    for name, t, r in (("dx", xs[0], dx64), ("dw", xs[1], dw64), ("db", xs[2], db64)):
        if t is not None:
            assert t.grad.shape == t.shape
            R.check_close(name, t.grad, r, atol=R.TOL_DENSE_GRAD)
