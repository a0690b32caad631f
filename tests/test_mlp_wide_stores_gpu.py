"""The first launch of the lean single-GPU MLP step with its 16-byte W1 apply (mlp_lean_fwdapply,
csrc/kernels/mlp_step_fwdapply.h, fwdapply_block<.., A16>: one float4 of p_old / p_new / Wt per
live lane on all four waves, the partials exchanged through LDS in another layout) against the untouched
generic pair ``mlp_fwdapply(ks=28)`` + ``mlp_head2(single=1)``, BIT for bit, at what
tests/test_mlp_lean_step_gpu.py does not reach (the cases were chosen for the slab-store forms
measured with it, profiles/wide_wt_stores/, and hold for any form of the launch):

* batch 1 (one live row: every row clamp active), 17 (a second row tile with one live row), 128
  (two full prefetched row tiles on every wave, none in the late loop), 256 (MAXB: four row tiles
  per wave, two of them loaded in the late loop);
* a long trajectory at batch 100 and 37: a copy step, then 64 pending steps over 4 distinct
  batches, through ``mlp_run_pipelined`` and from a captured graph of 8 steps replayed 8 times.
  Every step rewrites every slab line with new values and the head reads them with plain loads, so
  a stale line in any cache changes the bits;
* the flush (``mlp_apply``) after an odd and after an even number of steps.

Compared: both ping-pong parameter buffers, the stats ring, global_step, dz1R, dlR, hbuf, rowstat
and the whole slab with its padding.
"""
import pytest
import torch

from distributedtensorflowexample_amd.ops import init, mlp_step
from distributedtensorflowexample_amd.ops._ext import hip, ptr, stream_handle

pytestmark = pytest.mark.gpu

NB, LR, KS = 4, 0.3, 28
HP = mlp_step.HP


def _setup(gpu, B, seed=23):
    p = torch.empty(mlp_step.NPARAM, device=gpu)
    init.fill_(p, "normal", 0.0, 1.0, seed=seed)
    p[mlp_step.OFF_B1:mlp_step.OFF_W2].zero_()
    p[mlp_step.OFF_B2:].zero_()
    p.mul_(0.1)
    g = torch.Generator().manual_seed(seed + B)
    x = torch.rand(NB * B, 784, generator=g).to(gpu)
    y = torch.randint(0, 10, (NB * B,), generator=g).to(gpu).int()
    return p, x, y


class _Run:
    """Ping-pong buffers + workspace of one run."""

    def __init__(self, gpu, p, B):
        self.B = B
        self.BP = (B + 15) // 16 * 16
        self.bufs = [p.clone(), torch.full_like(p, float("nan"))]
        self.ws = mlp_step.StepWorkspace(B, gpu, stats_ring=8)

    def regions(self):
        ws, BP = self.ws, self.BP
        dz, dl = ws.rowmajor_factors()
        return {"slab": ws.buf[:KS * BP * HP], "hbuf": ws.buf[KS * BP * HP:(KS + 1) * BP * HP],
                "rowstat": ws.buf[-4 - 2 * BP:-4], "dz1R": dz, "dlR": dl, "p0": self.bufs[0],
                "p1": self.bufs[1], "stats": ws.stats, "ctr": ws.ctr}

    def snapshot(self):
        return {k: v.clone() for k, v in self.regions().items()}


def _bits(t):
    return t.contiguous().view(-1).view(torch.int32)


def _assert_same(a, b, what):
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), "%s: %s differs" % (what, k)


def _batch(x, y, B, i):
    return x[(i % NB) * B:(i % NB + 1) * B], y[(i % NB) * B:(i % NB + 1) * B]


def _step(run, x, y, lean, cur, pos, pending):
    """One two-launch step on batch ``pos`` (bufs[cur] -> bufs[cur ^ 1]); ``pending``: the update
    of the step before it (on batch pos - 1) is applied and recorded, else a copy step."""
    h, s, ws, B = hip(), stream_handle(), run.ws, run.B
    xb, yb = _batch(x, y, B, pos)
    xp = _batch(x, y, B, pos - 1)[0] if pending else xb
    po, pn = run.bufs[cur], run.bufs[cur ^ 1]
    lr, on = (LR, 1) if pending else (0.0, 0)
    if lean:
        h.mlp_lean_fwdapply(ptr(po), ptr(pn), lr, ptr(xp), ptr(xb), ptr(ws.buf), ptr(ws.ctr),
                            ptr(ws.stats), ws.stats_ring, B, on, s)
        h.mlp_lean_head(ptr(pn), ptr(yb), ptr(ws.buf), B, s)
    else:
        h.mlp_fwdapply(ptr(po), ptr(pn), lr, ptr(xp), ptr(xb), ptr(ws.buf), ptr(ws.ctr),
                       ptr(ws.stats), ws.stats_ring, B, on, s, ks=KS)
        h.mlp_head2(ptr(pn), ptr(yb), ptr(ws.buf), B, s, 0, 1)


def _flush(run, x, y, lean, cur, last_pos):
    """The pending update of the step on batch ``last_pos``: bufs[cur] -> bufs[cur ^ 1]."""
    h, s, ws, B = hip(), stream_handle(), run.ws, run.B
    xp = _batch(x, y, B, last_pos)[0]
    po, pn = run.bufs[cur], run.bufs[cur ^ 1]
    if lean:  # the lean first launch's apply half alone
        h.mlp_apply(ptr(po), ptr(pn), LR, ptr(xp), ptr(ws.buf), ptr(ws.ctr), ptr(ws.stats),
                    ws.stats_ring, B, s)
    else:     # the generic kernel once more (its forward over x_prev is discarded)
        h.mlp_fwdapply(ptr(po), ptr(pn), LR, ptr(xp), ptr(xp), ptr(ws.buf), ptr(ws.ctr),
                       ptr(ws.stats), ws.stats_ring, B, 1, s, ks=KS)


def _steps_then_flush(gpu, p, x, y, B, lean, steps):
    """A copy step and steps - 1 pending steps, then the flush: (state before the flush, state
    after it).  The generic flush also runs a forward, so the slab is compared before it only."""
    run = _Run(gpu, p, B)
    for i in range(steps):
        _step(run, x, y, lean, i & 1, i, i > 0)
    torch.cuda.synchronize()
    before = run.snapshot()
    _flush(run, x, y, lean, steps & 1, steps - 1)
    torch.cuda.synchronize()
    after = run.snapshot()
    del after["slab"]
    assert run.ws.global_step() == steps
    return before, after


@pytest.mark.parametrize("B", [1, 17, 128, 256])
def test_edge_batches_bit_identical_to_generic_pair(gpu, B):
    assert hip().mlp_single_ks() == KS
    p, x, y = _setup(gpu, B)
    new = _steps_then_flush(gpu, p, x, y, B, True, 4)
    old = _steps_then_flush(gpu, p, x, y, B, False, 4)
    BP = (B + 15) // 16 * 16
    assert float(old[0]["slab"].view(KS, BP, HP)[:, :B, :100].abs().sum()) > 0
    assert not bool(torch.isnan(old[1]["p1"]).any()) and float(old[1]["stats"].abs().sum()) > 0
    _assert_same(new[0], old[0], "B=%d before the flush" % B)
    _assert_same(new[1], old[1], "B=%d after the flush" % B)


@pytest.mark.parametrize("steps", [3, 4])
@pytest.mark.parametrize("B", [37, 100])
def test_flush_after_odd_and_even_step_counts(gpu, B, steps):
    p, x, y = _setup(gpu, B)
    new = _steps_then_flush(gpu, p, x, y, B, True, steps)
    old = _steps_then_flush(gpu, p, x, y, B, False, steps)
    # the flush reads bufs[steps & 1] and writes the other buffer
    assert not bool(torch.isnan(old[1]["p0" if steps & 1 else "p1"]).any())
    _assert_same(new[0], old[0], "B=%d, %d steps, before the flush" % (B, steps))
    _assert_same(new[1], old[1], "B=%d, %d steps, after the flush" % (B, steps))


NLONG, NGRAPH = 64, 8


@pytest.fixture(scope="module")
def long_reference(gpu):
    """B -> (inputs, final state of the generic pair issued eagerly): a copy step on batch 3, then
    64 pending steps on batches 0, 1, 2, 3, 0, ...; computed once."""
    out = {}
    for B in (100, 37):
        p, x, y = _setup(gpu, B)
        run = _Run(gpu, p, B)
        _step(run, x, y, False, 0, NB - 1, False)
        for i in range(NLONG):
            _step(run, x, y, False, (i + 1) & 1, i, True)
        torch.cuda.synchronize()
        assert run.ws.global_step() == NLONG
        out[B] = (p, x, y, run.snapshot())
    return out


@pytest.mark.parametrize("B", [100, 37])
def test_long_trajectory_host_loop(gpu, long_reference, B):
    p, x, y, ref = long_reference[B]
    run = _Run(gpu, p, B)
    ws = run.ws
    for cur, pending, pos, n in ((0, 0, NB - 1, 1), (1, 1, 0, NLONG)):
        hip().mlp_run_pipelined(ptr(run.bufs[0]), ptr(run.bufs[1]), cur, pending, LR, ptr(x),
                                ptr(y), NB, pos, n, ptr(ws.buf), ptr(ws.ctr), ptr(ws.stats),
                                ws.stats_ring, B, stream_handle(), 0)
    torch.cuda.synchronize()
    assert float(ref["slab"].abs().sum()) > 0 and not bool(torch.isnan(ref["p0"]).any())
    _assert_same(run.snapshot(), ref, "host loop B=%d" % B)


@pytest.mark.parametrize("B", [100, 37])
def test_long_trajectory_graph_replays(gpu, long_reference, B):
    p, x, y, ref = long_reference[B]
    run = _Run(gpu, p, B)
    _step(run, x, y, True, 0, NB - 1, False)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):  # 8 steps: the parity and the batch position come round
        for i in range(NGRAPH):
            _step(run, x, y, True, (i + 1) & 1, i, True)
    for _ in range(NLONG // NGRAPH):
        g.replay()
    torch.cuda.synchronize()
    _assert_same(run.snapshot(), ref, "graph B=%d" % B)
