"""float64 references for the small streaming kernels (loss, activations, BatchNorm, pools,
column sum), written from each operation's definition and independent of ``ops/``.

Four parts, shared by the CPU tier (tests/test_layer_reference_cpu.py) and the GPU tests
(tests/test_nn_layer_kernels_gpu.py, tests/test_cnn_layer_kernels_gpu.py):

* the references: plain torch float64, one function per operation.  bf16 and float32 kernel
  inputs are exact in float64, so a reference is the exact answer for the given inputs.  A
  function that feeds a tolerance also returns ``mag``, the sum of the absolute values of the
  terms its result is formed from;
* the comparison helpers (``check_*``): the bounds the kernels are held to;
* the input sets: deterministic builders, so both tiers see the same tensors;
* the launch arithmetic (``grid_once``, ``ew_grid``, ``grid_for``, the 65535-row cap, ...) with
  its constants read from the ``.hip`` sources: a test asserts with it that its shape reaches the
  branch it names, and fails loudly when a constant is retuned.

Bounds.  bf16 outputs: ``|out - ref| <= 2^-7 |ref| + 2^-20 mag`` -- one bf16 ulp (not half: a
kernel that associates its f32 arithmetic differently can land on the other side of a rounding
boundary) plus 16 f32 roundings of the terms.  f32 column sums: ``2^-20 sum|terms|``.
"""
import functools
import os
import re
import types

import numpy as np
import torch

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "csrc", "kernels")

BF16_ULP = 2.0 ** -7   # bf16 spacing relative to the value (8 significant bits)
F32_TERMS = 2.0 ** -20  # 16 float32 half-ulps of the summed magnitudes

# the project's absolute bounds for the f32 loss / activation kernels at logits in +-5
# (tests/test_kernels_gpu.py): fast exp / log / tanh, not float32 rounding, set them
TOL_LOSS = 1e-5
TOL_PROB = 3e-5     # probabilities and dlogits / scale
TOL_ACT = 1e-5
TOL_DENSE_Y = 2e-5
TOL_DENSE_GRAD = 1e-4
TOL_MEAN = 1e-5     # BatchNorm means (absolute)
TOL_RSTD = 1e-4     # rstd and variances (relative)


def f32(x):
    """A Python float holding ``x`` rounded to float32 (what a kernel receives)."""
    return float(np.float32(x))


def _d(t):
    return t.detach().cpu().double()


# =========================================================================== comparisons
def _worst(name, err, bound, extra=""):
    bound = bound.expand_as(err)
    bad = ~(err <= bound)  # (a NaN fails)
    if bool(bad.any()):
        excess = (err - bound).nan_to_num(nan=float("inf"))
        i = int(torch.where(bad, excess, torch.full_like(excess, float("-inf"))).reshape(-1).argmax())
        raise AssertionError("%s: %d of %d elements out of bound; worst at flat index %d: err %.3e, "
                             "bound %.3e%s" % (name, int(bad.sum()), err.numel(), i,
                                               float(err.reshape(-1)[i]),
                                               float(bound.reshape(-1)[i]), extra))
    ratio = err / bound.clamp_min(1e-300)
    return float(ratio.max()) if err.numel() else 0.0


def _same_shape(name, out, ref):
    if tuple(out.shape) != tuple(ref.shape):
        raise AssertionError("%s: shape %s, expected %s" % (name, tuple(out.shape), tuple(ref.shape)))


def check_bf16(name, out, ref, mag=None):
    """bf16 output against the exact answer: one bf16 ulp of ``ref`` + 2^-20 ``mag``.
    Returns the largest err / bound."""
    out = _d(out)
    _same_shape(name, out, ref)
    bound = BF16_ULP * ref.abs()
    if mag is not None:
        bound = bound + F32_TERMS * mag
    return _worst(name, (out - ref).abs(), bound)


def check_sum(name, out, ref, mag):
    """f32 sum against the exact sum: 2^-20 of the summed magnitudes."""
    out = _d(out)
    _same_shape(name, out, ref)
    return _worst(name, (out - ref).abs(), F32_TERMS * mag)


def check_close(name, out, ref, atol=0.0, rtol=0.0):
    out = _d(out)
    _same_shape(name, out, ref)
    return _worst(name, (out - ref).abs(), atol + rtol * ref.abs())


def check_exact(name, out, ref):
    """Exact comparison (``correct``, ``idx``, masked copies, sentinels)."""
    out, ref = _d(out), _d(ref)
    _same_shape(name, out, ref)
    bad = out != ref
    if bool(bad.any()) or bool(torch.isnan(out).any()):
        i = int(bad.reshape(-1).double().argmax())
        raise AssertionError("%s: %d of %d elements differ; first at flat index %d: %r != %r"
                             % (name, int(bad.sum()), out.numel(), i, float(out.reshape(-1)[i]),
                                float(ref.reshape(-1)[i])))


# =========================================================================== softmax cross-entropy
def first_argmax(t):
    """Index of the maximum of each row, the LOWEST index among equal maxima."""
    m = t.max(dim=1, keepdim=True).values
    idx = torch.arange(t.shape[1]).expand_as(t)
    return torch.where(t == m, idx, torch.full_like(idx, t.shape[1])).min(dim=1).values


def softmax_xent(logits, labels, ignore_index=-100, scale=1.0):
    """Per-row loss -sum_c y_c log softmax(l)_c, its gradient times ``scale``, the accuracy
    indicator argmax(l) == argmax(y) and the probabilities.

    ``labels`` int [N]: y = one-hot; a row whose label equals ``ignore_index`` or lies outside
    [0, C) is ignored: loss 0, gradient 0, correct 0.  ``labels`` float [N, C]: any dense y,
    d loss / d l = softmax(l) sum(y) - y.  Either arg-max: the lowest index among equal maxima."""
    l = _d(logits)
    N, C = l.shape
    scale = f32(scale)
    m = l.max(dim=1, keepdim=True).values
    e = torch.exp(l - m)
    se = e.sum(1, keepdim=True)
    p = e / se
    logp = (l - m) - torch.log(se)
    am = first_argmax(l)
    if labels.dtype.is_floating_point:
        y = _d(labels)
        loss = -(y * logp).sum(1)
        d = (p * y.sum(1, keepdim=True) - y) * scale
        correct = (am == first_argmax(y)).double()
    else:
        lab = labels.detach().cpu().long()
        valid = (lab != ignore_index) & (lab >= 0) & (lab < C)
        loss = torch.zeros(N, dtype=torch.float64)
        d = torch.zeros(N, C, dtype=torch.float64)
        correct = torch.zeros(N, dtype=torch.float64)
        for r in range(N):
            if not bool(valid[r]):
                continue  # ignored or out of range: loss 0, gradient 0, correct 0
            k = int(lab[r])
            loss[r] = -logp[r, k]
            d[r] = p[r] * scale
            d[r, k] -= scale
            correct[r] = 1.0 if int(am[r]) == k else 0.0
    return types.SimpleNamespace(loss=loss, dlogits=d, correct=correct, probs=p, scale=scale)


def check_xent(loss, d, correct, ref, probs=None, tol_loss=TOL_LOSS, tol_prob=TOL_PROB):
    """The loss kernel's outputs against :func:`softmax_xent`: loss rows and dlogits / scale
    (and probabilities) within the absolute bounds, ``correct`` exactly; ``d`` None = no
    gradient was asked for."""
    check_close("loss", loss, ref.loss, atol=tol_loss)
    check_exact("correct", correct, ref.correct)
    if d is not None:
        check_close("dlogits / scale", _d(d) / ref.scale, ref.dlogits / ref.scale, atol=tol_prob)
    if probs is not None:
        check_close("probs", probs, ref.probs, atol=tol_prob)


def top2_gap(t):
    """Per row: largest minus second largest value (inf for one column)."""
    t = _d(t)
    if t.shape[1] < 2:
        return torch.full((t.shape[0],), float("inf"), dtype=torch.float64)
    v = t.topk(2, dim=1).values
    return v[:, 0] - v[:, 1]


# =========================================================================== activations
GELU_K0 = 0.7978845608028654  # sqrt(2 / pi), the constants of elementwise.hip
GELU_K1 = 0.044715


def activation(x, act):
    """0 identity, 1 logistic sigmoid, 2 ReLU, 3 GELU (tanh form)."""
    x = x if x.dtype == torch.float64 else _d(x)  # (a float64 input keeps its autograd graph)
    if act == 1:
        return 1.0 / (1.0 + torch.exp(-x))
    if act == 2:
        return torch.where(x > 0, x, torch.zeros_like(x))
    if act == 3:
        return 0.5 * x * (1.0 + torch.tanh(GELU_K0 * (x + GELU_K1 * x ** 3)))
    return x.clone()


def activation_grad(dy, s, act):
    """dy * act'.  ``s`` is the saved forward OUTPUT for sigmoid (act' = s (1 - s)) and ReLU
    (act' = 1 where s > 0, 0 at s == 0), the PRE-activation for GELU, whose derivative is taken
    by float64 autograd of :func:`activation` (no second transcription of the formula)."""
    dy, s = _d(dy), _d(s)
    if act == 1:
        return dy * s * (1.0 - s)
    if act == 2:
        return torch.where(s > 0, dy, torch.zeros_like(dy))
    if act == 3:
        z = s.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(activation(z, 3).sum(), z)
        return dy * g
    return dy.clone()


def dense(x, w, b, act, dy):
    """y = act(x W^T + b) over the last axis and the gradients of sum(y dy) by float64
    autograd; returns (y, dx, dw, db or None)."""
    x, w = _d(x).requires_grad_(True), _d(w).requires_grad_(True)
    b = None if b is None else _d(b).requires_grad_(True)
    z = x @ w.t()
    if b is not None:
        z = z + b
    y = activation(z, act)
    grads = torch.autograd.grad((y * _d(dy)).sum(), [x, w] + ([b] if b is not None else []))
    return y.detach(), grads[0], grads[1], (grads[2] if b is not None else None)


DENSE_CASES = [  # (x shape, activation, bias): test_dense_autograd's sizes plus a 3-D input
    ((50, 40), 2, True), ((50, 40), 3, True), ((50, 40), 1, False), ((3, 5, 40), 1, True),
    ((3, 5, 40), 3, False)]
DENSE_OUT = 20


def dense_case(xshape, with_bias):
    sd = 700 + sum(xshape)
    x = uniform(*xshape, seed=sd)
    w = uniform(DENSE_OUT, xshape[-1], seed=sd + 1)
    b = uniform(DENSE_OUT, seed=sd + 2) if with_bias else None
    dy = uniform(*xshape[:-1], DENSE_OUT, seed=sd + 3, scale=2.0)
    return x, w, b, dy


# =========================================================================== BatchNorm
def bn_finalize(s, q, M, eps=1e-5, run_mean=None, run_var=None, momentum=0.9):
    """Batch statistics from the column sums ``s`` / ``q`` (sum, sum of squares over M rows):
    mean, biased variance clamped at 0, rstd = 1 / sqrt(var + eps); running statistics in the
    momentum form run = momentum run + (1 - momentum) new, the variance made unbiased (M / (M - 1),
    1 for M = 1)."""
    s, q = _d(s), _d(q)
    eps, momentum = f32(eps), f32(momentum)
    mean = s / M
    var = (q / M - mean * mean).clamp_min(0.0)
    out = types.SimpleNamespace(mean=mean, var=var, rstd=1.0 / torch.sqrt(var + eps),
                                run_mean=None, run_var=None)
    if run_mean is not None:
        unbias = M / (M - 1.0) if M > 1 else 1.0
        out.run_mean = momentum * _d(run_mean) + (1.0 - momentum) * mean
        out.run_var = momentum * _d(run_var) + (1.0 - momentum) * var * unbias
    return out


def bn_apply(x, mean, rstd, gamma, beta, res=None, relu=True):
    """y = act((x - mean) rstd gamma + beta [+ res]) over [..., C]; returns (y, mag) with
    mag = |x sc| + |mean sc| + |beta| + |res|, sc = rstd gamma."""
    x = _d(x)
    mean, rstd, gamma, beta = _d(mean), _d(rstd), _d(gamma), _d(beta)
    sc = rstd * gamma
    y = (x - mean) * sc + beta
    mag = (x * sc).abs() + (mean * sc).abs() + beta.abs()
    if res is not None:
        y = y + _d(res)
        mag = mag + _d(res).abs()
    if relu:
        y = y.clamp_min(0.0)
    return y, mag


def bn_bwd(dy, y, x, mean, rstd, gamma, relu=True):
    """Backward of y = act(bn(x) [+ res]) with batch statistics: de = dy masked by the GIVEN y
    (y > 0) when ``relu``; sum_dy = sum de, sum_dyxh = sum de xhat over the M rows;
    dx = gamma rstd (de - sum_dy / M - xhat sum_dyxh / M); dres = de."""
    C = x.shape[-1]
    dy2, x2 = _d(dy).reshape(-1, C), _d(x).reshape(-1, C)
    M = x2.shape[0]
    mean, rstd, gamma = _d(mean), _d(rstd), _d(gamma)
    de = torch.where(_d(y).reshape(-1, C) > 0, dy2, torch.zeros_like(dy2)) if relu else dy2
    xh = (x2 - mean) * rstd
    s1, s2 = de.sum(0), (de * xh).sum(0)
    a1, a2 = de.abs().sum(0), (de * xh).abs().sum(0)
    A = gamma * rstd
    dx = A * (de - s1 / M - xh * s2 / M)
    mag = A.abs() * (de.abs() + a1 / M + xh.abs() * a2 / M)
    return types.SimpleNamespace(dx=dx.reshape(x.shape), dres=de.reshape(x.shape), sum_dy=s1,
                                 sum_dyxh=s2, mag_dx=mag.reshape(x.shape), mag_dy=a1, mag_dyxh=a2)


# =========================================================================== pools
def pool_out(n):
    return (n + 2 - 3) // 2 + 1


def maxpool_fwd(x):
    """3x3 / stride 2 / pad 1 max pool over NHWC as a loop over the 9 taps in the order
    t = 3 kh + kw: a tap replaces the running maximum only when STRICTLY greater, so the first
    maximal tap wins; taps in the padding are not candidates.  Returns (y, idx = winning tap)."""
    x = _d(x)
    N, H, W, C = x.shape
    OH, OW = pool_out(H), pool_out(W)
    xp = torch.zeros(N, H + 2, W + 2, C, dtype=torch.float64)
    ok = torch.zeros(N, H + 2, W + 2, C, dtype=torch.bool)
    xp[:, 1:H + 1, 1:W + 1] = x
    ok[:, 1:H + 1, 1:W + 1] = True
    best = torch.full((N, OH, OW, C), float("-inf"), dtype=torch.float64)
    idx = torch.zeros(N, OH, OW, C, dtype=torch.uint8)
    for t in range(9):
        kh, kw = t // 3, t % 3
        v = xp[:, kh:kh + 2 * OH - 1:2, kw:kw + 2 * OW - 1:2]
        take = ok[:, kh:kh + 2 * OH - 1:2, kw:kw + 2 * OW - 1:2] & (v > best)
        best = torch.where(take, v, best)
        idx = torch.where(take, torch.full_like(idx, t), idx)
    return best, idx


def maxpool_bwd(dy, idx, x_shape):
    """Every output's gradient goes to the input pixel of its stored tap; an input pixel sums
    the (at most four) outputs that chose it."""
    N, H, W, C = x_shape
    dy = _d(dy)
    idx = idx.detach().cpu()
    OH, OW = pool_out(H), pool_out(W)
    dxp = torch.zeros(N, H + 2, W + 2, C, dtype=torch.float64)
    for t in range(9):
        kh, kw = t // 3, t % 3
        dxp[:, kh:kh + 2 * OH - 1:2, kw:kw + 2 * OW - 1:2] += torch.where(
            idx == t, dy, torch.zeros_like(dy))
    return dxp[:, 1:H + 1, 1:W + 1].contiguous()


def avgpool_fwd(x):
    """Mean over H x W; returns (y [N, C], mag = mean |x|)."""
    x = _d(x)
    return x.mean((1, 2)), x.abs().mean((1, 2))


def avgpool_bwd(dy, x_shape):
    N, H, W, C = x_shape
    return (_d(dy)[:, None, None, :] / (H * W)).expand(N, H, W, C).contiguous()


def colsum(g, out0=None, beta=0.0):
    """out = beta out0 + column sums of g; returns (out, mag = |beta out0| + sum |g|)."""
    g = _d(g)
    s, mag = g.sum(0), g.abs().sum(0)
    if beta != 0.0 and out0 is not None:
        s = s + f32(beta) * _d(out0)
        mag = mag + (f32(beta) * _d(out0)).abs()
    return s, mag


# =========================================================================== input sets
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(*shape, seed):
    return torch.randn(*shape, generator=_gen(seed))


def uniform(*shape, seed, scale=1.0):
    return (torch.rand(*shape, generator=_gen(seed)) * 2 - 1) * scale


# ---- softmax cross-entropy
XENT_SHAPES = [(1, 1), (5, 10), (301, 10), (7, 64), (6, 65), (3, 130), (2, 1003)]
XENT_GAP = 1e-3
SPECIAL_LABELS = ("ignore", "minus_one", "C", "C_plus_3")


def xent_logits(N, C, scale=5.0, seed=0):
    """f32 logits in +-scale.  The last row ties (c, c + 1) and the row before it (c, c + 64)
    where the shape has room (bit-equal maxima; (c, c + 64) puts both in one lane, on two loop
    trips); every other row's top-2 gap is at least XENT_GAP.  Returns (logits, ties) with
    ties = {row: (low index, high index)}."""
    l = uniform(N, C, seed=100 + seed + 7 * N + C, scale=scale)
    top = l.argmax(1)
    l[torch.arange(N), top] += 0.01 * scale
    ties = {}
    if C >= 2 and N >= 2:
        c = (3 * N) % (C - 1)
        ties[N - 1] = (c, c + 1)
    if C > 64 and N >= 2:
        c = (5 * N) % (C - 64)
        ties[N - 2] = (c, c + 64)
    for r, (a, b) in ties.items():
        l[r, a] = l[r, b] = l[r].max() + 0.05 * scale
    return l, ties


def assert_gaps(logits, ties):
    """The inputs' own property: tie rows are bit-equal at their pair, all others gapped."""
    gap = top2_gap(logits)
    for r in range(logits.shape[0]):
        if r in ties:
            a, b = ties[r]
            assert float(logits[r, a]) == float(logits[r, b]) == float(logits[r].max())
            assert int((logits[r] == logits[r].max()).sum()) == 2
        else:
            assert float(gap[r]) >= XENT_GAP, (r, float(gap[r]))


def xent_int_labels(N, C, ties, seed=0):
    """Valid random labels; a tie row is labelled with the HIGHER tied index (correct must be
    0: the arg-max is the lower); the first rows carry -100 (the default ignore_index), -1, C
    and C + 3 as far as the shape has rows left.  Returns (labels int32, {kind: row})."""
    lab = torch.randint(0, C, (N,), generator=_gen(200 + seed + N + C)).int()
    for r, (_, b) in ties.items():
        lab[r] = b
    free = [r for r in range(N) if r not in ties]
    special = {}
    if len(free) > 1 or (free and ties):
        vals = {"ignore": -100, "minus_one": -1, "C": C, "C_plus_3": C + 3}
        for kind, r in zip(SPECIAL_LABELS, free[:4]):
            lab[r] = vals[kind]
            special[kind] = r
    return lab, special


def xent_int_labels_ignore0(N, C, ties, seed=0):
    """Labels for a run with ignore_index = 0: every third free row is labelled 0."""
    lab = torch.randint(0, C, (N,), generator=_gen(300 + seed + N + C)).int()
    for r, (_, b) in ties.items():
        lab[r] = b
    zero_rows = [r for r in range(N) if r not in ties][::3]
    for r in zero_rows:
        lab[r] = 0
    return lab, zero_rows


DENSE_KINDS = ("onehot", "soft", "sum07", "sum13", "zero", "tie2")


def xent_dense_kinds(N, C):
    """Row kinds of the dense labels of a shape (every kind where N >= 6 and C >= 2)."""
    if C < 2:
        return ["onehot"] * N
    if N >= 6:
        return [DENSE_KINDS[r % 6] for r in range(N)]
    start = {5: 1, 3: 3, 2: 2}.get(N, 0)
    return [DENSE_KINDS[(start + r) % 6] for r in range(N)]


def xent_dense_labels(N, C, ties, seed=0):
    """f32 dense labels [N, C]: one-hot rows, soft rows summing to 1, to 0.7 and to 1.3, an
    all-zero row and a row whose two largest labels are bit-equal; a logit tie row is one-hot at
    the higher tied index.  Returns (labels, kinds)."""
    kinds = xent_dense_kinds(N, C)
    g = _gen(400 + seed + N + C)
    y = torch.zeros(N, C, dtype=torch.float64)
    for r in range(N):
        if r in ties:
            kinds[r] = "onehot"
            y[r, ties[r][1]] = 1.0
            continue
        k = kinds[r]
        j = int(torch.randint(0, C, (1,), generator=g))
        if k == "onehot":
            y[r, j] = 1.0
        elif k == "zero":
            pass
        else:
            row = torch.rand(C, generator=g, dtype=torch.float64)
            row[j] = 0.25 * C + 1.0  # a clear largest label
            if k == "tie2":
                row[(j + 1) % C] = row[j]
            row = row / row.sum() * {"soft": 1.0, "sum07": 0.7, "sum13": 1.3, "tie2": 1.0}[k]
            y[r] = row
    y = y.float()
    for r in range(N):
        if kinds[r] == "tie2" and r not in ties:
            top = y[r].topk(2).values
            assert float(top[0]) == float(top[1])
    return y, kinds


def aim_logits_at_label_ties(logits, y, kinds, ties):
    """On the rows whose two largest dense labels are equal, put the logits' arg-max on one of
    the two: alternately the lower index (correct = 1) and the higher (correct = 0: the labels'
    arg-max is the lower).  Returns (logits, {row: expected correct})."""
    l = logits.clone()
    want = {}
    for r, k in enumerate(kinds):
        if k != "tie2" or r in ties:
            continue
        pair = torch.where(y[r] == y[r].max())[0]
        assert pair.numel() == 2
        which = len(want) % 2
        l[r, int(pair[which])] = l[r].max() + 0.25
        want[r] = 1.0 - which
    return l, want


# ---- activations
ACT_SPECIALS = (0.0, -0.0, 30.0, -30.0, 1e-3, -1e-3)
ACT_SIZES = [1, 3, 4, 5, 1023, 1027]


def act_inputs(n, seed=0):
    """(x, dy): x in +-5 with the special values (exact 0, -0, +-30, +-1e-3) written at the
    start and at the END (the scalar tail), as many as n holds; dy in +-1."""
    x = uniform(n, seed=500 + seed + n % 97, scale=5.0)
    dy = uniform(n, seed=600 + seed + n % 97, scale=1.0)
    sp = torch.tensor(ACT_SPECIALS)
    k = min(n, len(sp))
    rot = torch.roll(sp, -(n % len(sp)))
    x[:k] = rot[:k]
    if n >= 2 * len(sp):
        x[n - len(sp):] = sp
    return x, dy


# ---- BatchNorm
BN_SETS = [(197, 8), (1500, 8), (197, 64), (37, 2056), (100, 96), (60, 96)]
BN_LARGE = (131073 + 76, 64)


@functools.lru_cache(maxsize=None)
def bn_case(M, C):
    """One BatchNorm input set: bf16 x [M, C] (mean ~1, std ~2), residual, dy; f32 affine; the
    column sums s / q as f32 (what the convolution epilogue hands over) and mean / rstd from
    them (f32, the kernels' inputs); y = relu(bn(x) + res) in bf16 for the backward's mask."""
    sd = 1000 + 31 * C + M % 1009
    x = (randn(M, C, seed=sd) * 2 + 1).to(BF)
    res = randn(M, C, seed=sd + 1).to(BF)
    dy = randn(M, C, seed=sd + 2).to(BF)
    gamma = randn(C, seed=sd + 3) * 0.1 + 1
    beta = randn(C, seed=sd + 4) * 0.1
    xd = x.double()
    s, q = xd.sum(0).float(), (xd * xd).sum(0).float()
    fin = bn_finalize(s, q, M)
    mean, rstd = fin.mean.float(), fin.rstd.float()
    y = bn_apply(x, mean, rstd, gamma, beta, res, True)[0].to(BF)
    return types.SimpleNamespace(M=M, C=C, x=x, res=res, dy=dy, gamma=gamma, beta=beta, s=s, q=q,
                                 mean=mean, rstd=rstd, y=y)


@functools.lru_cache(maxsize=None)
def bn_bwd_ref(M, C, relu):
    c = bn_case(M, C)
    return bn_bwd(c.dy, c.y, c.x, c.mean, c.rstd, c.gamma, relu)


@functools.lru_cache(maxsize=None)
def bn_apply_ref(M, C, with_res, relu):
    c = bn_case(M, C)
    return bn_apply(c.x, c.mean, c.rstd, c.gamma, c.beta, c.res if with_res else None, relu)


# a channel of M equal values v: q / M - mean^2 is exactly 0, and rounds NEGATIVE in float32
# however the compiler contracts the expression (asserted by f32_variances, CPU tier)
CLAMP_VALUE = 100.0
CLAMP_M = 221
BN_FINALIZE_CASES = [(1, CLAMP_M, True), (64, CLAMP_M, True), (257, CLAMP_M, True), (64, 1, False),
                     (257, 197, False)]  # (C, M, channel 0 clamped)


def f32_variances(s, q, M):
    """q / M - mean^2 of one channel in float32, every way the expression can be evaluated:
    (mean by reciprocal, no FMA), (FMA on q inv_m), (FMA on mean^2), (true division: the
    project's CPU path).  Also returns the reciprocal-form mean."""
    s, q = np.float32(s), np.float32(q)
    inv = np.float32(1.0) / np.float32(M)
    mu = np.float32(s * inv)
    qm = np.float32(q * inv)
    mm = np.float32(mu * mu)
    plain = np.float32(qm - mm)
    fma_q = np.float32(np.float64(q) * np.float64(inv) - np.float64(mm))
    fma_m = np.float32(np.float64(qm) - np.float64(mu) * np.float64(mu))
    mu_d = np.float32(s / np.float32(M))
    div = np.float32(np.float32(q / np.float32(M)) - np.float32(mu_d * mu_d))
    return [float(v) for v in (plain, fma_q, fma_m, div)], float(mu), float(mu_d)


def bn_finalize_case(C, M, clamp=True):
    """Column sums of x ~ N(1, 2) (bf16) over M rows, channel 0 made M equal large values when
    ``clamp``, and non-trivial running statistics."""
    x = (randn(M, C, seed=2000 + C + M) * 2 + 1).to(BF).double()
    if clamp:
        x[:, 0] = CLAMP_VALUE
    s, q = x.sum(0).float(), (x * x).sum(0).float()
    run_mean = randn(C, seed=2100 + C) * 0.5
    run_var = torch.rand(C, generator=_gen(2200 + C)) + 0.5
    return s, q, run_mean, run_var


# ---- pools
MAXPOOL_SHAPES = [(1, 1, 1, 8), (2, 2, 3, 8), (2, 15, 16, 64), (2, 16, 15, 64), (1, 16, 16, 264)]
MAXPOOL_ROWLOOP = (32768, 3, 2, 8)  # N * OH = 65536 rows forward, N * H = 98304 backward
MAXPOOL_KINDS = ("random", "ties", "negative")
AVGPOOL_SHAPES = [(2, 1, 1, 10), (3, 7, 7, 10), (2, 15, 16, 64)]
AVGPOOL_BWD_WRAP = (3, 37, 37, 512)


@functools.lru_cache(maxsize=None)
def maxpool_case(shape, kind):
    """(x, dy) bf16: random values; values from {0, 0.5, 1} (most windows tie, as after a
    ReLU); an all-negative image (padding must never win)."""
    sd = 3000 + sum(shape) + 17 * MAXPOOL_KINDS.index(kind)
    N, H, W, C = shape
    if kind == "ties":
        x = torch.randint(0, 3, shape, generator=_gen(sd)).float() * 0.5
    else:
        x = randn(*shape, seed=sd)
        if kind == "negative":
            x = -x.abs() - 0.25
    dy = randn(N, pool_out(H), pool_out(W), C, seed=sd + 1)
    return x.to(BF), dy.to(BF)


@functools.lru_cache(maxsize=None)
def maxpool_ref(shape, kind):
    x, dy = maxpool_case(shape, kind)
    y, idx = maxpool_fwd(x)
    return y, idx, maxpool_bwd(dy, idx, shape)


def avgpool_case(shape):
    N, H, W, C = shape
    return randn(*shape, seed=4000 + sum(shape)).to(BF), randn(N, C, seed=4001 + sum(shape)).to(BF)


# ---- column sum
COLSUM_SHAPES = [(1, 1), (3, 70), (50, 129), (257, 64)]


def colsum_case(M, N):
    return uniform(M, N, seed=5000 + M + N), uniform(N, seed=5001 + M + N, scale=3.0)


# =========================================================================== launch arithmetic
def _src(name):
    with open(os.path.join(KERNELS, name)) as f:
        return f.read()


def _find(text, pattern, what):
    m = re.search(pattern, text, re.S)
    if m is None:
        raise AssertionError("launch arithmetic: %s not found in the kernel source -- the code "
                             "changed, re-derive the reach conditions of the layer tests" % what)
    return m


@functools.lru_cache(maxsize=None)
def launch_constants():
    """The constants the reach conditions depend on, read from the .hip sources."""
    cnn, ew = _src("cnn.hip"), _src("elementwise.hip")
    sx, gf = _src("softmax_xent.hip"), _src("gemm_f32.hip")
    k = types.SimpleNamespace()
    k.ew_u = int(_find(cnn, r"constexpr int kEwU = (\d+);", "kEwU").group(1))
    k.once_block = int(_find(
        cnn, r"static unsigned grid_once\(long long chunks, int u\) \{\s*long long b = "
             r"\(chunks \+ (\d+)LL \* u - 1\) / \(\1LL \* u\);", "grid_once").group(1))
    m = _find(cnn, r"static unsigned grid_for\(long long n, int per = (\d+)\) \{\s*long long b = "
                   r"\(n \+ per - 1\) / per;\s*if \(b > (\d+)\) b = \2;", "grid_for")
    k.for_per, k.for_cap = int(m.group(1)), int(m.group(2))
    k.pool_rows_fwd = int(_find(cnn, r"void maxpool_fwd_launch\([^{]*\{.*?std::min\(N \* OH, (\d+)\)",
                                "maxpool_fwd row cap").group(1))
    k.pool_rows_bwd = int(_find(cnn, r"void maxpool_bwd_launch\([^{]*\{.*?std::min\(N \* H, (\d+)\)",
                                "maxpool_bwd row cap").group(1))
    m = _find(cnn, r"void bn_bwd_launch\([^{]*\{.*?tpr = cg < (\d+) \? cg : \1, rpp = \1 / tpr;\s*"
                   r"long long rpb = \(M \+ (\d+)\) / (\d+);\s*if \(rpb < rpp \* (\d+)\) rpb = rpp \* \4;",
              "bn_bwd rows per block")
    assert int(m.group(2)) + 1 == int(m.group(3))
    k.bwd_threads, k.bwd_blocks, k.bwd_min_rows = int(m.group(1)), int(m.group(3)), int(m.group(4))
    k.avg_block = 256
    _find(cnn, r"void avgpool_fwd_launch\([^{]*\{\s*hipLaunchKernelGGL\(avgpool_fwd_kernel, "
               r"dim3\(\(N \* C \+ 255\) / 256\), dim3\(256\)", "avgpool_fwd grid")
    k.fin_block = 256
    _find(cnn, r"hipLaunchKernelGGL\(bn_finalize_kernel, dim3\(\(C \+ 255\) / 256\), dim3\(256\)",
          "bn_finalize grid")
    m = _find(ew, r"static dim3 ew_grid\(long long n\) \{\s*long long b = \(\(n >> 2\) \+ (\d+)\) / "
                  r"(\d+);\s*if \(b > (\d+)\) b = \3;", "ew_grid")
    assert int(m.group(1)) + 1 == int(m.group(2))
    k.ew_block, k.ew_cap = int(m.group(2)), int(m.group(3))
    k.xent_rows = int(_find(sx, r"const int row = blockIdx\.x \* (\d+) \+ \(threadIdx\.x >> 6\);",
                            "softmax_xent rows per block").group(1))
    k.colsum_cols = int(_find(gf, r"void colsum_kernel\(.*?const int n = blockIdx\.x \* (\d+) \+ c;",
                              "colsum columns per block").group(1))
    k.colsum_groups = int(_find(gf, r"void colsum_kernel\(.*?for \(int m = g; m < M; m \+= (\d+)\)",
                                "colsum row groups").group(1))
    return k


def grid_once(chunks, u=None):
    k = launch_constants()
    u = k.ew_u if u is None else u
    per = k.once_block * u
    return max(1, min((chunks + per - 1) // per, 1 << 30))


def bn_stream_path(M, C):
    """'fast' (one channel group per thread) or 'general' (per-element channel) for the
    streaming BatchNorm kernels (bn_apply, bn_bwd_apply) at [M, C]."""
    cg = C // 8
    stride = grid_once(M * cg) * launch_constants().once_block
    return "fast" if stride % cg == 0 else "general"


def bn_bwd_reduce_plan(M, C):
    """bn_bwd_launch's reduce geometry: threads per row, rows per pass, rows per block, blocks,
    channel passes of the ``base`` loop, and whether rows per block came from M."""
    k = launch_constants()
    cg = C // 8
    tpr = min(cg, k.bwd_threads)
    rpp = k.bwd_threads // tpr
    from_m = (M + k.bwd_blocks - 1) // k.bwd_blocks
    rpb = max(from_m, rpp * k.bwd_min_rows)
    return types.SimpleNamespace(tpr=tpr, rpp=rpp, rpb=rpb, blocks=(M + rpb - 1) // rpb,
                                 passes=(cg + tpr - 1) // tpr, from_m=from_m > rpp * k.bwd_min_rows)


def ew_passes(n):
    """(blocks, grid-stride passes of the float4 loop) of the activation kernels at n."""
    k = launch_constants()
    n4 = n >> 2
    b = max(1, min((n4 + k.ew_block - 1) // k.ew_block, k.ew_cap))
    return b, (n4 + b * k.ew_block - 1) // (b * k.ew_block)


def grid_for_passes(n):
    """(blocks, grid-stride passes) of a scalar loop launched with grid_for(n)."""
    k = launch_constants()
    b = max(1, min((n + k.for_per - 1) // k.for_per, k.for_cap))
    return b, (n + b * k.for_per - 1) // (b * k.for_per)


def ew_wrap_sizes():
    """(the smallest n past 2048 * 256 * 4 with n % 4 == 3, the smallest such n whose float4
    loop really makes a second pass)."""
    k = launch_constants()
    full = k.ew_cap * k.ew_block * 4
    return full + 3, full + 7


def maxpool_plan(shape):
    """x blocks and grid rows / loop trips of the max pool forward and backward."""
    k = launch_constants()
    N, H, W, C = shape
    OH, OW = pool_out(H), pool_out(W)
    cg = C // 8
    return types.SimpleNamespace(
        xblocks_fwd=(OW * cg + 255) // 256, xblocks_bwd=(W * cg + 255) // 256,
        loops_fwd=N * OH > k.pool_rows_fwd, loops_bwd=N * H > k.pool_rows_bwd)
