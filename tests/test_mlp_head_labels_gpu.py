"""The label path and the packed unit pair of the MLP head (head_row,
csrc/kernels/mlp_step_3launch.h).

The head reads its row's label with a per-lane vector load issued ahead of the operand loads
and sums a lane's two hidden units as one pair.  These tests pin what that must not change:
every row uses ITS OWN label (labels passed as slices 1 and 3 elements into a larger tensor
whose neighbouring elements hold other classes), labels outside 0..9 keep their defined
behaviour, the padding of hbuf / dz1R / dlR stays exactly zero, and labels that change from
step to step give the same parameters from a captured graph and from the host loop.

Weights are the existing tests' 0.1-scaled ones.  Before any GPU output is looked at, the
float64 reference asserts that every softmax probability lies in (1e-3, 1 - 1e-3): dlogits =
(prob - onehot) / B is then negative at the label and positive elsewhere by a margin (>= 1e-3 /
B) four orders of magnitude above f32 rounding, so the sign patterns are exact.
"""
import pytest
import torch

from distributedtensorflowexample_amd.ops import init, mlp_step
from distributedtensorflowexample_amd.ops._ext import hip, ptr, stream_handle

pytestmark = pytest.mark.gpu

LR, KS, HP = 0.3, 28, mlp_step.HP
# max |hbuf - float64| of the parent build (two scalar sums, two 4-byte hbuf stores) on these
# inputs, measured on an MI355X, per batch size; the test allows twice that
HBUF_PARENT_ERR = {17: 1.936e-07, 100: 2.255e-07}
_REF = {}


def _pattern(row):
    """Neighbouring rows differ (step 3 mod 10)."""
    return (3 * row + 1) % 10


def _inputs(gpu, B, seed=4):
    p = torch.empty(mlp_step.NPARAM, device=gpu)
    init.fill_(p, "normal", 0.0, 1.0, seed=seed)
    p[mlp_step.OFF_B1:mlp_step.OFF_W2].zero_()
    p[mlp_step.OFF_B2:].zero_()
    p.mul_(0.1)
    g = torch.Generator().manual_seed(seed + B)
    x = torch.rand(B, 784, generator=g).to(gpu)
    return p, x


def _reference(gpu, B):
    """(p, x, h, logits, prob) with the float64 forward, once per batch size; the probabilities
    are checked to be clear of 0 and 1 before any test looks at a GPU result."""
    if B not in _REF:
        p, x = _inputs(gpu, B)
        h, logits = mlp_step.reference_forward(p.double().cpu(), x.double().cpu())
        prob = torch.softmax(logits, 1)
        assert float(prob.min()) > 1e-3 and float(prob.max()) < 1 - 1e-3
        _REF[B] = (p, x, h, logits, prob)
    return _REF[B]


def _label_slice(gpu, y, off):
    """`y` (int32 [B], CPU) as a slice starting `off` elements into a larger tensor: 4-byte but
    (off = 1, 3) not 8- or 16-byte aligned; the elements around it hold OTHER classes (the
    pattern continued, shifted by 5)."""
    B = y.numel()
    k = torch.arange(-off, B + 8 - off)
    big = ((_pattern(k) + 5) % 10).int()
    big[off:off + B] = y
    big = big.to(gpu)
    assert big.data_ptr() % 16 == 0
    v = big[off:off + B]
    assert v.is_contiguous() and v.data_ptr() % 8 != 0
    assert int(big[off - 1]) != int(y[0]) and int(big[off + B]) != int(y[-1])
    return v


def _head(gpu, p, x, yv, B, lean=True):
    """Copy + forward and one head on (p, x, labels): (workspace, dz1R, dlR, rowstat, hbuf)."""
    ws = mlp_step.StepWorkspace(B, gpu)
    pn = torch.empty_like(p)
    if lean:
        mlp_step.step_pipelined(p, pn, x, x, yv, ws, LR, apply=False)
    else:  # the kernels the lean pair wraps
        h, s = hip(), stream_handle()
        h.mlp_fwdapply(ptr(p), ptr(pn), 0.0, ptr(x), ptr(x), ptr(ws.buf), ptr(ws.ctr),
                       ptr(ws.stats), ws.stats_ring, B, 0, s, ks=KS)
        h.mlp_head2(ptr(pn), ptr(yv), ptr(ws.buf), B, s, 0, 1)
    torch.cuda.synchronize()
    o_dz, o_dl, BP = hip().mlp_rowmajor_layout(B)
    assert BP == (B + 15) // 16 * 16
    dz = ws.store[o_dz:o_dz + BP * HP].view(BP, HP)
    dl = ws.store[o_dl:o_dl + BP * 16].view(BP, 16)
    rs = ws.buf[-4 - 2 * BP:-4].view(BP, 2)
    hb = ws.buf[KS * BP * HP:(KS + 1) * BP * HP].view(BP, HP)
    return ws, dz, dl, rs, hb


def _assert_rows_use_their_label(dl, rs, y, logits, rows):
    """Exact: the only negative entry of dlR[row, :10] is at labels[row]; accuracy = (argmax ==
    label) on rows whose reference top-two logit gap exceeds 1e-3."""
    B = y.numel()
    neg = (dl[:B, :10] < 0).cpu()
    yl = y.long()
    top2 = logits.topk(2, 1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3
    acc = (logits.argmax(1) == yl).float()
    got = rs[:B, 1].cpu()
    for r in rows:
        assert int(neg[r].sum()) == 1 and bool(neg[r, yl[r]]), (r, int(yl[r]), neg[r])
        if bool(clear[r]):
            assert float(got[r]) == float(acc[r]), (r, int(yl[r]))


@pytest.mark.parametrize("lean", [True, False], ids=["lean", "generic"])
@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("B", [1, 16, 17, 100, 113])
def test_each_row_gets_its_own_label(gpu, B, off, lean):
    p, x, _, logits, _ = _reference(gpu, B)
    y = _pattern(torch.arange(B)).int()
    _, _, dl, rs, _ = _head(gpu, p, x, _label_slice(gpu, y, off), B, lean)
    _assert_rows_use_their_label(dl, rs, y, logits, range(B))


@pytest.mark.parametrize("B", [17, 100])
def test_head_matches_float64(gpu, B):
    """Loss (1e-4), dlR and dz1R (1e-6: the bounds of test_one_label_batch_matches_reference)
    and hbuf against float64.  hbuf: the parent build's maximum error on these inputs was
    measured as 1.936e-07 (B = 17) and 2.255e-07 (B = 100), HBUF_PARENT_ERR; twice that is
    allowed (this build measures the same two figures: its results are bit-identical)."""
    p, x, h, logits, prob = _reference(gpu, B)
    y = _pattern(torch.arange(B)).int()
    _, dz, dl, rs, hb = _head(gpu, p, x, _label_slice(gpu, y, 1), B)
    W2t = mlp_step.unflatten(p.double().cpu())[2]
    yl = y.long()
    loss = torch.logsumexp(logits, 1) - logits.gather(1, yl[:, None])[:, 0]
    dl_ref = (prob - torch.nn.functional.one_hot(yl, 10)) / B
    dz_ref = (dl_ref @ W2t) * h * (1 - h)
    e_loss = float((rs[:B, 0].double().cpu() - loss).abs().max())
    e_dl = float((dl[:B, :10].double().cpu() - dl_ref).abs().max())
    e_dz = float((dz[:B, :100].double().cpu() - dz_ref).abs().max())
    e_h = float((hb[:B, :100].double().cpu() - h).abs().max())
    print("B=%d: loss %.3e dl %.3e dz1 %.3e hbuf %.3e" % (B, e_loss, e_dl, e_dz, e_h))
    assert e_loss <= 1e-4 and e_dl <= 1e-6 and e_dz <= 1e-6
    assert e_h <= 2 * HBUF_PARENT_ERR[B]


@pytest.mark.parametrize("lean", [True, False], ids=["lean", "generic"])
def test_labels_out_of_range(gpu, lean):
    """Rows labelled -1, 10 and 2^31 - 1: no -1 term in dl (every entry >= 0), the label's
    logit taken as 0 (loss = logsumexp, 1e-4), accuracy 0; all other rows as usual."""
    B, bad = 17, {0: -1, 5: 10, 16: 2 ** 31 - 1}
    p, x, _, logits, _ = _reference(gpu, B)
    y = _pattern(torch.arange(B)).int()
    for r, v in bad.items():
        y[r] = v
    _, _, dl, rs, _ = _head(gpu, p, x, _label_slice(gpu, y, 1), B, lean)
    lse = torch.logsumexp(logits, 1)
    for r in bad:
        assert bool((dl[r, :10] >= 0).all()), (r, dl[r])
        assert abs(float(rs[r, 0]) - float(lse[r])) <= 1e-4
        assert float(rs[r, 1]) == 0.0
    yc = y.clone()
    for r in bad:
        yc[r] = 0  # (not looked at: only the other rows are checked)
    _assert_rows_use_their_label(dl, rs, yc, logits, [r for r in range(B) if r not in bad])


@pytest.mark.parametrize("B", [1, 17, 113])
def test_padding_stays_exact_zero(gpu, B):
    """hbuf rows >= B and units >= 100, and the dz1R / dlR paddings, are exactly 0 after the
    head (B = 113: the generic kernel, BP = 128 != HP = 112)."""
    p, x, h, _, _ = _reference(gpu, B)
    y = _pattern(torch.arange(B)).int()
    _, dz, dl, _, hb = _head(gpu, p, x, _label_slice(gpu, y, 3), B)
    assert float(hb[:B, :100].min()) > 0 and float(dl[:B, :10].abs().min()) > 0
    assert float(dz[:B, :100].abs().sum()) > 0
    for t, live in ((hb, 100), (dz, 100), (dl, 10)):
        assert int((t[B:] != 0).sum()) == 0 and int((t[:, live:] != 0).sum()) == 0


@pytest.mark.parametrize("B", [17, 100])
def test_labels_that_move_from_step_to_step(gpu, B):
    """3 pipelined steps over 3 batches with different labels and the flush, once from a
    captured graph and once through the host loop: bit-equal parameters, within 1e-4 of the
    float64 trajectory."""
    NB = 3
    p, _ = _inputs(gpu, B)
    g = torch.Generator().manual_seed(100 + B)
    x = torch.rand(NB * B, 784, generator=g).to(gpu)
    y = torch.randint(0, 10, (NB * B,), generator=g).int()
    assert not torch.equal(y[:B], y[B:2 * B]) and not torch.equal(y[B:2 * B], y[2 * B:])
    ref = p.double().cpu()
    for i in range(NB):
        gr, _, _ = mlp_step.reference_step(ref, x[i * B:(i + 1) * B].double().cpu(),
                                           y[i * B:(i + 1) * B])
        ref = ref - LR * gr
    y = y.to(gpu)

    def graphed():
        bufs = [p.clone(), torch.full_like(p, float("nan"))]
        ws = mlp_step.StepWorkspace(B, gpu, stats_ring=8)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=s):
            cur = 0
            for i in range(NB):
                xb, yb = x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]
                xp = x[(i - 1) * B:i * B] if i else xb
                mlp_step.step_pipelined(bufs[cur], bufs[cur ^ 1], xp, xb, yb, ws, LR, apply=i > 0)
                cur ^= 1
            mlp_step.flush_pipelined(bufs[cur], bufs[cur ^ 1], x[(NB - 1) * B:], ws, LR)
            cur ^= 1
        gph.replay()
        torch.cuda.synchronize()
        return bufs[cur]

    def looped():
        bufs = [p.clone(), torch.full_like(p, float("nan"))]
        ws = mlp_step.StepWorkspace(B, gpu, stats_ring=8)
        hip().mlp_run_pipelined(ptr(bufs[0]), ptr(bufs[1]), 0, 0, LR, ptr(x), ptr(y), NB, 0, NB,
                                ptr(ws.buf), ptr(ws.ctr), ptr(ws.stats), ws.stats_ring, B,
                                stream_handle(), 1)
        torch.cuda.synchronize()
        return bufs[(NB + 1) & 1]

    a, b = graphed(), looped()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    err = float((a.double().cpu() - ref).abs().max())
    print("B=%d: vs f64 after %d steps %.3e" % (B, NB, err))
    assert err <= 1e-4 and not torch.equal(a, p)
