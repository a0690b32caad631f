"""The lean entry points of the single-GPU two-launch MLP step (mlp_lean_fwdapply /
mlp_lean_head, csrc/kernels/mlp_step_fwdapply.h: packed kernel arguments, workspace regions
derived from the base pointer, phase A's operands requested first) against the
kernels they wrap, ``mlp_fwdapply(ks=28)`` + ``mlp_head2(single=1)``.  No floating-point
operation or summation order differs, so everything is compared BIT for bit.

Batches: 16 (exactly one row tile), 37 (ragged last tile, generic kernels), 100 (the
compile-time 7-tile kernels), 130 (9 row tiles: past the two prefetched row tiles per wave).
Sequence: a copy step (nothing pending, lr = 0, no stats record), three pending steps, the flush.
"""
import pytest
import torch

from distributedtensorflowexample_amd.ops import init, mlp_step
from distributedtensorflowexample_amd.ops._ext import hip, ptr, stream_handle

pytestmark = pytest.mark.gpu

BATCHES = [16, 37, 100, 130]
NB, LR, KS = 4, 0.3, 28
HP = mlp_step.HP


def _setup(gpu, B, seed=11):
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
    """Ping-pong buffers + workspace of one run of the sequence."""

    def __init__(self, gpu, p, B):
        self.B = B
        self.bufs = [p.clone(), torch.full_like(p, float("nan"))]
        self.ws = mlp_step.StepWorkspace(B, gpu, stats_ring=8)
        self.slab_before_flush = None

    def regions(self):
        ws, B = self.ws, self.B
        BP = (B + 15) // 16 * 16
        dz, dl = ws.rowmajor_factors()
        hb = ws.buf[KS * BP * HP:(KS + 1) * BP * HP]
        rs = ws.buf[-4 - 2 * BP:-4]
        return {"dz1R": dz, "dlR": dl, "hbuf": hb, "rowstat": rs, "p0": self.bufs[0],
                "p1": self.bufs[1], "stats": ws.stats, "ctr": ws.ctr}

    def slab(self):
        BP = (self.B + 15) // 16 * 16
        return self.ws.buf[:KS * BP * HP].clone()


def _bits(t):
    return t.contiguous().view(-1).view(torch.int32)


def _batch(x, y, B, i):
    return x[(i % NB) * B:(i % NB + 1) * B], y[(i % NB) * B:(i % NB + 1) * B]


def _sequence(run, x, y, lean, steps=4):
    """steps two-launch steps from a non-pending state, then the flush."""
    h, s, ws, B = hip(), stream_handle(), run.ws, run.B
    cur = 0
    for i in range(steps):
        xb, yb = _batch(x, y, B, i)
        xp = _batch(x, y, B, i - 1)[0] if i else xb
        po, pn = run.bufs[cur], run.bufs[cur ^ 1]
        lr, on = (LR, 1) if i else (0.0, 0)
        if lean:
            h.mlp_lean_fwdapply(ptr(po), ptr(pn), lr, ptr(xp), ptr(xb), ptr(ws.buf), ptr(ws.ctr),
                                ptr(ws.stats), ws.stats_ring, B, on, s)
            h.mlp_lean_head(ptr(pn), ptr(yb), ptr(ws.buf), B, s)
        else:
            h.mlp_fwdapply(ptr(po), ptr(pn), lr, ptr(xp), ptr(xb), ptr(ws.buf), ptr(ws.ctr),
                           ptr(ws.stats), ws.stats_ring, B, on, s, ks=KS)
            h.mlp_head2(ptr(pn), ptr(yb), ptr(ws.buf), B, s, 0, 1)
        cur ^= 1
    if not torch.cuda.is_current_stream_capturing():
        run.slab_before_flush = run.slab()
    xp = _batch(x, y, B, steps - 1)[0]
    po, pn = run.bufs[cur], run.bufs[cur ^ 1]
    if lean:  # the flush: the lean first launch's apply half alone
        h.mlp_apply(ptr(po), ptr(pn), LR, ptr(xp), ptr(ws.buf), ptr(ws.ctr), ptr(ws.stats),
                    ws.stats_ring, B, s)
    else:     # the wrapped kernel once more (its forward over x_prev is discarded)
        h.mlp_fwdapply(ptr(po), ptr(pn), LR, ptr(xp), ptr(xp), ptr(ws.buf), ptr(ws.ctr),
                       ptr(ws.stats), ws.stats_ring, B, 1, s, ks=KS)


def _assert_same(a, b, what):
    ra, rb = a.regions(), b.regions()
    for k in ra:
        assert torch.equal(_bits(ra[k]), _bits(rb[k])), "%s: %s differs" % (what, k)


@pytest.fixture(scope="module")
def lean_runs(gpu):
    """B -> (inputs, the eager run of the sequence through the lean pair), computed once."""
    assert hip().mlp_single_ks() == KS  # (DTFX_MLP_KS=14 selects the 14-slice kernels instead)
    out = {}
    for B in BATCHES:
        p, x, y = _setup(gpu, B)
        run = _Run(gpu, p, B)
        _sequence(run, x, y, lean=True)
        torch.cuda.synchronize()
        out[B] = (p, x, y, run)
    return out


@pytest.mark.parametrize("B", BATCHES)
def test_lean_pair_bit_identical_to_wrapped_kernels(gpu, lean_runs, B):
    p, x, y, new = lean_runs[B]
    old = _Run(gpu, p, B)
    _sequence(old, x, y, lean=False)
    torch.cuda.synchronize()
    assert new.ws.global_step() == old.ws.global_step() == 4
    assert float(new.ws.stats[:4].abs().sum()) > 0 and not bool(torch.isnan(new.bufs[1]).any())
    _assert_same(new, old, "B=%d" % B)
    # the z1 slabs of the last step.  (The tile-major slab layout [28][7][BP][16] was measured
    # and not kept -- profiles/lean_step/README.md -- so both pairs index them [28][BP][112].)
    BP = (B + 15) // 16 * 16
    slab_old = old.slab_before_flush.view(KS, BP, HP)
    slab_new = new.slab_before_flush.view(KS, BP, HP)
    assert float(slab_old[:, :B, :100].abs().sum()) > 0
    assert torch.equal(_bits(slab_old), _bits(slab_new))


@pytest.mark.parametrize("B", [37, 100])
def test_lean_pair_in_graph_and_host_loop(gpu, lean_runs, B):
    """The same sequence replayed from a captured graph and issued by mlp_run_pipelined."""
    p, x, y, eager = lean_runs[B]
    graphed = _Run(gpu, p, B)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        _sequence(graphed, x, y, lean=True)
    g.replay()
    torch.cuda.synchronize()
    _assert_same(graphed, eager, "graph B=%d" % B)
    assert torch.equal(_bits(graphed.slab()), _bits(eager.slab_before_flush))

    looped = _Run(gpu, p, B)
    ws = looped.ws
    hip().mlp_run_pipelined(ptr(looped.bufs[0]), ptr(looped.bufs[1]), 0, 0, LR, ptr(x), ptr(y), NB,
                            0, 4, ptr(ws.buf), ptr(ws.ctr), ptr(ws.stats), ws.stats_ring, B,
                            stream_handle(), 1)
    torch.cuda.synchronize()
    _assert_same(looped, eager, "host loop B=%d" % B)
    assert torch.equal(_bits(looped.slab()), _bits(eager.slab_before_flush))
