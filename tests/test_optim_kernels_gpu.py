"""The parameter-update kernels against an independent float64 reference (torch.optim on CPU
float64 tensors with injected state, tests/optim_reference.py), at the sizes where each loop can
go wrong, and the split-K fold (segment table) optimizers called directly with hand-built tables.

Bound (optim_reference.bound): per step a value is rounded at most twice by half a float32 ulp,
so |gpu - ref| <= 2 * steps * 2^-23 * max(1, max|ref|), taken per region of the inputs."""
import numpy as np
import pytest
import torch

import optim_reference as R
from distributedtensorflowexample_amd.ops import cnn, optim
from distributedtensorflowexample_amd.ops import transformer as T

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
# one element past a full pass of each capped grid, plus a float4 remainder / scalar tail
N_FLAT_WRAP = 2048 * 256 * 4 + 1024 + 3   # sgd_, adam_ (float4 loop, 2048 blocks)
N_SCALAR_WRAP = 2048 * 256 + 259          # momentum_, scale_ (scalar loop, 2048 blocks)
N_ADAM_MIXED_WRAP = 4096 * 256 * 4 + 1028
N_SGD_MIXED_WRAP = 8192 * 256 * 4 + 1028


def _steps(n):
    return 2 if n > (1 << 19) else 10


# ------------------------------------------------------------------ flat kernels
@pytest.mark.parametrize("n,wd", [(n, wd) for n in (1, 2, 3, 4, 5, 1027) for wd in (0.0, 0.01)]
                         + [(N_FLAT_WRAP, 0.01)])
def test_sgd(gpu, n, wd):
    steps = _steps(n)
    p, g, _, _, regions = R.make_case(n, 10 + n % 97)
    P, G = p.to(gpu), g.to(gpu)
    ref = p.double()
    for _ in range(steps):
        optim.sgd_(P, G, 0.01, weight_decay=wd)
        ref, _ = R.sgd_step(ref, g, 0.01, wd=wd)
    R.assert_close("p", P, ref, steps, regions)
    assert torch.equal(G.cpu(), g)


@pytest.mark.parametrize("n,nesterov,wd",
                         [(n, nv, wd) for n in (1, 255, 257) for nv in (False, True)
                          for wd in (0.0, 0.01)]
                         + [(N_SCALAR_WRAP, False, 0.01), (N_SCALAR_WRAP, True, 0.0)])
def test_momentum(gpu, n, nesterov, wd):
    steps = _steps(n)
    p, g, buf, _, regions = R.make_case(n, 20 + n % 97)
    P, G, B = p.to(gpu), g.to(gpu), buf.to(gpu)
    ref, rbuf = p.double(), buf.double()
    for _ in range(steps):
        optim.momentum_(P, G, B, 0.01, 0.9, weight_decay=wd, nesterov=nesterov)
        ref, rbuf = R.sgd_step(ref, g, 0.01, wd=wd, mu=0.9, nesterov=nesterov, buf=rbuf)
    R.assert_close("p", P, ref, steps, regions)
    R.assert_close("buf", B, rbuf, steps, regions)


@pytest.mark.parametrize("n", [1, 255, 257, N_SCALAR_WRAP])
def test_scale(gpu, n):
    """x * a rounds once: the float64 product of two float32 values is exact, so the kernel must
    give its float32 rounding bit for bit."""
    x = R.make_case(n, 30)[0]
    a = R.f32(1.0 / 3.0)
    X = x.to(gpu)
    optim.scale_(X, a)
    assert torch.equal(X.cpu(), (x.double() * a).float())


_ADAM_HP = [(0.0, 0.9, 0.999, 1), (0.01, 0.9, 0.999, 1), (0.01, 0.8, 0.95, 1000)]


@pytest.mark.parametrize("adamw", [True, False])
@pytest.mark.parametrize("n,wd,b1,b2,step0",
                         [(n, 0.01, 0.9, 0.999, 1) for n in (1, 2, 3, 4, 5)]
                         + [(1027,) + hp for hp in _ADAM_HP]
                         + [(N_FLAT_WRAP, 0.01, 0.9, 0.999, 1000)])
def test_adam(gpu, n, wd, b1, b2, step0, adamw):
    steps = _steps(n)
    p, g, m, v, regions = R.make_case(n, 40 + n % 97)
    P, G, M, V = (t.to(gpu) for t in (p, g, m, v))
    ref, rm, rv = p.double(), m.double(), v.double()
    for s in range(step0, step0 + steps):
        optim.adam_(P, G, M, V, 1e-3, s, b1, b2, 1e-8, wd, adamw)
        ref, rm, rv = R.adam_step(ref, g, rm, rv, 1e-3, s, b1, b2, 1e-8, wd, adamw)
    R.assert_close("p", P, ref, steps, regions)
    R.assert_close("m", M, rm, steps, regions)
    R.assert_close("v", V, rv, steps, regions)


def test_adam_zero_moments_first_step(gpu):
    """From m = v = 0 at step 1 (what a fresh run does), with the zero / tiny / big blocks."""
    n = 1027
    p, g, m, v, regions = R.make_case(n, 50, moments=False)
    P, G, M, V = (t.to(gpu) for t in (p, g, m, v))
    optim.adam_(P, G, M, V, 1e-3, 1, weight_decay=0.01)
    ref, rm, rv = R.adam_step(p, g, m, v, 1e-3, 1, wd=0.01)
    R.assert_close("p", P, ref, 1, regions)
    R.assert_close("m", M, rm, 1, regions)
    R.assert_close("v", V, rv, 1, regions)
    # the zero block (make_case: the first 64 elements): the parameter only decays
    blk = 64
    assert not bool(g[:blk].any())
    assert not bool(M[:blk].any()) and not bool(V[:blk].any())
    decayed = p[:blk].double() * (1 - R.f32(1e-3) * R.f32(0.01))
    assert (P[:blk].cpu().double() - decayed).abs().max() <= R.bound(1, decayed)


# ------------------------------------------------------------------ mixed-precision kernels
@pytest.mark.parametrize("n,wd,gscale,b1,b2,step0",
                         [(n, wd, gs, 0.9, 0.999, s0) for n in (4, 1028)
                          for wd, gs, s0 in ((0.01, 0.5, 1), (0.0, 1.0, 1), (0.01, 0.5, 1000))]
                         + [(1028, 0.01, 0.5, 0.8, 0.95, 1),
                            (N_ADAM_MIXED_WRAP, 0.01, 0.5, 0.9, 0.999, 1000)])
def test_adam_mixed(gpu, n, wd, gscale, b1, b2, step0):
    steps = _steps(n)
    p, g, m, v, regions = R.make_case(n, 60 + n % 97)
    P, G, M, V = (t.to(gpu) for t in (p, g, m, v))
    pb = torch.zeros(n, device=gpu, dtype=BF)
    ref, rm, rv = p.double(), m.double(), v.double()
    for s in range(step0, step0 + steps):
        T.adam_mixed(P, G, M, V, pb, 1e-3, s, b1, b2, 1e-6, wd, gscale)
        assert torch.equal(pb, P.to(BF))
        ref, rm, rv = R.adam_mixed_step(ref, g, rm, rv, 1e-3, s, b1, b2, 1e-6, wd, gscale)
    R.assert_close("p", P, ref, steps, regions)
    R.assert_close("m", M, rm, steps, regions)
    R.assert_close("v", V, rv, steps, regions)


@pytest.mark.parametrize("n,wd,gscale", [(4, 1e-4, 0.5), (4, 0.0, 1.0), (1028, 1e-4, 0.5),
                                         (1028, 0.0, 1.0), (N_SGD_MIXED_WRAP, 1e-4, 0.5)])
def test_sgd_momentum_mixed(gpu, n, wd, gscale):
    steps = _steps(n)
    p, g, v, _, regions = R.make_case(n, 70 + n % 97)
    P, G, V = (t.to(gpu) for t in (p, g, v))
    pb = torch.zeros(n, device=gpu, dtype=BF)
    ref, rv = p.double(), v.double()
    for _ in range(steps):
        cnn.sgd_momentum_mixed(P, G, V, pb, 0.01, 0.9, wd, gscale)
        assert torch.equal(pb, P.to(BF))
        ref, rv = R.sgd_momentum_mixed_step(ref, g, rv, 0.01, 0.9, wd, gscale)
    R.assert_close("p", P, ref, steps, regions)
    R.assert_close("v", V, rv, steps, regions)


_EDGE_BF16 = R.EDGE_BF16


def _edge_master():
    bits = np.array(R.EDGE_BITS + [0x3F800000] * 2, dtype=np.uint32)  # 12: a float4 multiple
    return torch.from_numpy(bits.view(np.float32).copy())


def _bits32(t):
    return t.detach().cpu().view(torch.int32)


def _bits16(t):
    return t.detach().cpu().view(torch.int16)


@pytest.mark.parametrize("kernel", ["adam_mixed", "sgd_momentum_mixed", "cast_bf16"])
def test_bf16_copy_rounding_edges(gpu, kernel):
    """lr = 0, wd = 0: the master comes back bit for bit and the bf16 copy is its
    round-to-nearest-even conversion (the words torch's own conversion gives, see
    test_optim_reference_cpu.test_bf16_edge_patterns).  The gradient is positive: p - 0 * g keeps
    a master -0 only then (-0 - -0 is +0 in IEEE arithmetic, in the float64 reference too)."""
    p = _edge_master()
    n = p.numel()
    P = p.to(gpu)
    G = torch.linspace(0.1, 1, n).to(gpu)
    pb = torch.zeros(n, device=gpu, dtype=BF)
    if kernel == "adam_mixed":
        T.adam_mixed(P, G, torch.zeros_like(P), torch.zeros_like(P), pb, 0.0, 1, wd=0.0)
    elif kernel == "sgd_momentum_mixed":
        cnn.sgd_momentum_mixed(P, G, torch.zeros_like(P), pb, 0.0, 0.9, 0.0, 1.0)
    else:
        pb = T.cast_bf16(P)
    assert torch.equal(_bits32(P), _bits32(p))
    want = torch.from_numpy(np.array(_EDGE_BF16, dtype=np.uint16).view(np.int16).copy())
    assert torch.equal(_bits16(pb)[:10], want)
    assert torch.equal(_bits16(pb), _bits16(p.to(BF)))


# ------------------------------------------------------------------ device-side lr / step
def _capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    return graph


_LRS = [1e-3, 5e-4, 2e-3]


def test_counter_add(gpu):
    c = torch.tensor([5], device=gpu, dtype=torch.int32)
    optim.counter_add_(c)
    assert c.item() == 6
    optim.counter_add_(c, -3)
    assert c.item() == 3
    optim.counter_add_(c, 1)
    assert c.item() == 4
    with pytest.raises(TypeError):
        optim.counter_add_(torch.zeros(1, device=gpu, dtype=torch.int64))


@pytest.mark.parametrize("adamw", [True, False])
def test_adam_graph_lr_and_step_tensors(gpu, adamw):
    n = 1027
    p, g, m, v, regions = R.make_case(n, 80)
    P, G, M, V = (t.to(gpu) for t in (p, g, m, v))
    lr_t = torch.zeros(1, device=gpu)
    step_t = torch.ones(1, device=gpu, dtype=torch.int32)
    # load the kernels outside the capture (scratch copies; lr 0.5 / step 77 must not be used)
    optim.adam_(P.clone(), G, M.clone(), V.clone(), 0.5, 77, weight_decay=0.01, adamw=adamw,
                lr_tensor=lr_t, step_tensor=step_t.clone())
    optim.counter_add_(step_t.clone())
    torch.cuda.synchronize()

    def body():
        optim.adam_(P, G, M, V, 0.5, 77, weight_decay=0.01, adamw=adamw, lr_tensor=lr_t,
                    step_tensor=step_t)
        optim.counter_add_(step_t)

    graph = _capture(body)
    ref, rm, rv = p.double(), m.double(), v.double()
    for s, lr in enumerate(_LRS, start=1):
        lr_t.fill_(lr)
        graph.replay()
        ref, rm, rv = R.adam_step(ref, g, rm, rv, lr, s, wd=0.01, adamw=adamw)
    torch.cuda.synchronize()
    assert step_t.item() == 4
    R.assert_close("p", P, ref, 3, regions)
    R.assert_close("m", M, rm, 3, regions)
    R.assert_close("v", V, rv, 3, regions)


@pytest.mark.parametrize("kind", ["sgd", "momentum", "nesterov"])
def test_sgd_momentum_graph_lr_tensor(gpu, kind):
    n = 1027
    p, g, buf, _, regions = R.make_case(n, 81)
    P, G, B = p.to(gpu), g.to(gpu), buf.to(gpu)
    lr_t = torch.zeros(1, device=gpu)

    def run(pp, bb):
        if kind == "sgd":
            optim.sgd_(pp, G, 0.5, weight_decay=0.01, lr_tensor=lr_t)
        else:
            optim.momentum_(pp, G, bb, 0.5, 0.9, weight_decay=0.01,
                            nesterov=kind == "nesterov", lr_tensor=lr_t)

    run(P.clone(), B.clone())
    torch.cuda.synchronize()
    graph = _capture(lambda: run(P, B))
    ref, rbuf = p.double(), buf.double()
    for lr in _LRS:
        lr_t.fill_(lr)
        graph.replay()
        if kind == "sgd":
            ref, _ = R.sgd_step(ref, g, lr, wd=0.01)
        else:
            ref, rbuf = R.sgd_step(ref, g, lr, wd=0.01, mu=0.9, nesterov=kind == "nesterov",
                                   buf=rbuf)
    torch.cuda.synchronize()
    R.assert_close("p", P, ref, 3, regions)
    if kind != "sgd":
        R.assert_close("buf", B, rbuf, 3, regions)


def test_adam_mixed_graph_step_ptr(gpu):
    n = 1028
    p, g, m, v, regions = R.make_case(n, 82)
    P, G, M, V = (t.to(gpu) for t in (p, g, m, v))
    pb = torch.zeros(n, device=gpu, dtype=BF)
    step_t = torch.ones(1, device=gpu, dtype=torch.int32)
    T.adam_mixed(P.clone(), G, M.clone(), V.clone(), None, 1e-3, 77, gscale=0.5,
                 step_ptr=step_t.clone())
    optim.counter_add_(step_t.clone())
    torch.cuda.synchronize()

    def body():
        T.adam_mixed(P, G, M, V, pb, 1e-3, 77, gscale=0.5, step_ptr=step_t)
        optim.counter_add_(step_t)

    graph = _capture(body)
    ref, rm, rv = p.double(), m.double(), v.double()
    for s in (1, 2, 3):
        graph.replay()
        ref, rm, rv = R.adam_mixed_step(ref, g, rm, rv, 1e-3, s, gscale=0.5)
    torch.cuda.synchronize()
    assert step_t.item() == 4
    R.assert_close("p", P, ref, 3, regions)
    R.assert_close("m", M, rm, 3, regions)
    R.assert_close("v", V, rv, 3, regions)
    assert torch.equal(pb, P.to(BF))


# ------------------------------------------------------------------ segment tables (split-K fold)
# (lo4, hi4, S): starts at 0; touching segments; one float4; across the 256-thread boundary; ends
# at n4; every remainder of the 4 / 2 / 1 plane unroll; gaps in which g is read
SEG_N = 2800
SEG_ROWS = [(0, 5, 1), (5, 6, 2), (6, 40, 3), (250, 262, 4), (262, 263, 5), (300, 301, 6),
            (400, 450, 7), (450, 500, 8), (690, 700, 9)]
_NAN = float("nan")


class SegCase:
    """Synthetic split-K planes for a table of (lo4, hi4, S) rows over n elements.  Every second
    segment's plane stride exceeds its length; the padding between planes, a guard float4 behind
    the last plane and ``g`` inside every segment are NaN, so a read of the wrong place shows."""

    def __init__(self, n, rows, seed, dev):
        gen = torch.Generator().manual_seed(seed)
        self.n, self.rows = n, rows
        p, g, m, v, _ = R.make_case(n, seed)
        g = torch.randn(n, generator=gen)
        self.p, self.m, self.v = p, m, v
        self.g_sum64 = g.double().clone()      # float64 sum of the planes
        self.g_split = g.clone()               # float32 adds in split order
        self.g_in = g.clone()                  # what the kernel is given: NaN in the segments
        self.bufs, table = [], []
        for k, (lo4, hi4, S) in enumerate(rows):
            ln = (hi4 - lo4) * 4
            pl4 = (hi4 - lo4) + (3 if k % 2 else 0)
            buf = torch.full((S * pl4 * 4 + 4,), _NAN)
            planes = [torch.randn(ln, generator=gen) for _ in range(S)]
            acc32, acc64 = planes[0].clone(), planes[0].double()
            for q in range(S):
                buf[q * pl4 * 4:q * pl4 * 4 + ln] = planes[q]
                if q:
                    acc32 = acc32 + planes[q]
                    acc64 = acc64 + planes[q].double()
            self.g_split[lo4 * 4:hi4 * 4] = acc32
            self.g_sum64[lo4 * 4:hi4 * 4] = acc64
            self.g_in[lo4 * 4:hi4 * 4] = _NAN
            d = buf.to(dev)
            assert d.data_ptr() % 16 == 0
            self.bufs.append(d)
            table.append([lo4, hi4, d.data_ptr(), pl4, S])
        assert all(a[1] <= b[0] for a, b in zip(table, table[1:])) and table[-1][1] * 4 <= n
        self.segs = torch.tensor(table, dtype=torch.int64, device=dev)
        self.regions = [("all", torch.arange(n))]

    def state(self, dev):
        return [t.to(dev) for t in (self.p, self.m, self.v)]


def _adam_seg_run(c, gpu, g, segs, cuts=((0, None),)):
    P, M, V = c.state(gpu)
    pb = torch.zeros(c.n, device=gpu, dtype=BF)
    G = g.to(gpu)
    for lo, hi in cuts:
        sl = slice(lo, hi)
        T.adam_mixed(P[sl], G[sl], M[sl], V[sl], pb[sl], 1e-3, 3, gscale=0.5, segs=segs, base=lo)
    return P, M, V, pb


def _sgd_seg_run(c, gpu, g, segs):
    P, _, V = c.state(gpu)
    pb = torch.zeros(c.n, device=gpu, dtype=BF)
    cnn.sgd_momentum_mixed(P, g.to(gpu), V, pb, 0.01, 0.9, 1e-4, 0.5, segs=segs)
    return P, V, pb


def _check_adam_seg(c, gpu):
    out = _adam_seg_run(c, gpu, c.g_in, c.segs)
    ref, rm, rv = R.adam_mixed_step(c.p, c.g_sum64, c.m, c.v, 1e-3, 3, gscale=0.5)
    R.assert_close("p", out[0], ref, 1, c.regions)
    R.assert_close("m", out[1], rm, 1, c.regions)
    R.assert_close("v", out[2], rv, 1, c.regions)
    assert torch.equal(out[3], out[0].to(BF))
    # the plain kernel on the gradient summed in split order: the same update expression
    plain = _adam_seg_run(c, gpu, c.g_split, None)
    for a, b, name in zip(out, plain, "pmvb"):
        assert torch.equal(a, b), name


def _check_sgd_seg(c, gpu):
    out = _sgd_seg_run(c, gpu, c.g_in, c.segs)  # the case's ``v`` is the momentum buffer
    ref, rv = R.sgd_momentum_mixed_step(c.p, c.g_sum64, c.v, 0.01, 0.9, 1e-4, 0.5)
    R.assert_close("p", out[0], ref, 1, c.regions)
    R.assert_close("v", out[1], rv, 1, c.regions)
    assert torch.equal(out[2], out[0].to(BF))
    plain = _sgd_seg_run(c, gpu, c.g_split, None)
    for a, b, name in zip(out, plain, "pvb"):
        assert torch.equal(a, b), name


@pytest.fixture(scope="module")
def seg_case(gpu):
    return SegCase(SEG_N, SEG_ROWS, 90, gpu)


def test_adam_mixed_segments(gpu, seg_case):
    _check_adam_seg(seg_case, gpu)


def test_sgd_momentum_mixed_segments(gpu, seg_case):
    _check_sgd_seg(seg_case, gpu)


def test_adam_mixed_segments_in_buckets(gpu, seg_case):
    """Two launches over [0, 1200) and [1200, 2800) with base = lo (segment (300, 301) starts on
    the cut) are bit-identical to one launch: the same kernel, so exact equality."""
    c = seg_case
    whole = _adam_seg_run(c, gpu, c.g_in, c.segs)
    parts = _adam_seg_run(c, gpu, c.g_in, c.segs, cuts=((0, 1200), (1200, None)))
    for a, b, name in zip(whole, parts, "pmvb"):
        assert torch.equal(a, b), name
    assert bool(torch.isfinite(parts[0]).all())


def _many_rows(k):
    return [(2 * i, 2 * i + 1, 1 + i % 2) for i in range(k)]


@pytest.mark.parametrize("kernel", ["adam_mixed", "sgd_momentum_mixed"])
def test_segment_table_of_128(gpu, kernel):
    c = SegCase(128 * 2 * 4, _many_rows(128), 91, gpu)
    (_check_adam_seg if kernel == "adam_mixed" else _check_sgd_seg)(c, gpu)


@pytest.mark.parametrize("kernel", ["adam_mixed", "sgd_momentum_mixed"])
def test_segment_table_of_129_raises(gpu, kernel):
    c = SegCase(129 * 2 * 4, _many_rows(129), 92, gpu)
    with pytest.raises(RuntimeError, match="128 segments"):
        if kernel == "adam_mixed":
            _adam_seg_run(c, gpu, c.g_in, c.segs)
        else:
            _sgd_seg_run(c, gpu, c.g_in, c.segs)


@pytest.mark.parametrize("kernel,n,blocks", [("adam_mixed", N_ADAM_MIXED_WRAP, 4096),
                                             ("sgd_momentum_mixed", N_SGD_MIXED_WRAP, 8192)])
def test_segment_in_second_grid_pass(gpu, kernel, n, blocks):
    """A segment of 257 float4s, S = 2, that starts at the first float4 of the second pass of the
    capped grid (and ends at n4)."""
    lo4 = blocks * 256
    assert lo4 + 257 == n // 4
    c = SegCase(n, [(lo4, lo4 + 257, 2)], 93, gpu)
    (_check_adam_seg if kernel == "adam_mixed" else _check_sgd_seg)(c, gpu)


# ------------------------------------------------------------------ calls that must be rejected
def _mixed_call(kernel, P, G, M, V, pb, **kw):
    if kernel == "adam_mixed":
        T.adam_mixed(P, G, M, V, pb, 1e-3, 1, **kw)
    else:
        cnn.sgd_momentum_mixed(P, G, V, pb, 0.01, 0.9, 1e-4, 1.0, **kw)


def _bad_tables(good):
    n = good.shape[0]
    wide = torch.zeros(n, 6, dtype=torch.int64, device=good.device)
    return {
        "float": good.double(),
        "int32": good.int(),
        "cpu": good.cpu(),
        "one-dim": good.flatten(),
        "four-columns": good[:, :4].contiguous(),
        "row-stride-6": wide[:, :5],
        "column-major": good.t().contiguous().t(),
    }


@pytest.mark.parametrize("kernel", ["adam_mixed", "sgd_momentum_mixed"])
def test_bad_segment_tables_raise(gpu, seg_case, kernel):
    c = seg_case
    for name, bad in _bad_tables(c.segs).items():
        P, M, V = c.state(gpu)
        before = P.clone()
        pb = torch.zeros(c.n, device=gpu, dtype=BF)
        with pytest.raises(ValueError, match="segs"):
            _mixed_call(kernel, P, c.g_split.to(gpu), M, V, pb, segs=bad)
        assert torch.equal(P, before), name


@pytest.mark.parametrize("kernel,which",
                         [("adam_mixed", w) for w in ("p", "g", "m", "v", "pb")]
                         + [("sgd_momentum_mixed", w) for w in ("p", "g", "v", "pb")])
def test_misaligned_buffers_raise(gpu, kernel, which):
    """A slice that starts one element into a buffer (4 bytes; 2 for the bf16 copy) is rejected on
    the host, before any launch."""
    n = 16
    t = {k: torch.zeros(n + 4, device=gpu) for k in "pgmv"}
    t["pb"] = torch.zeros(n + 4, device=gpu, dtype=BF)
    args = {k: (x[1:n + 1] if k == which else x[:n]) for k, x in t.items()}
    with pytest.raises(RuntimeError, match="aligned"):
        _mixed_call(kernel, args["p"], args["g"], args["m"], args["v"], args["pb"])
    torch.cuda.synchronize()
    assert all(float(x.float().abs().sum()) == 0 for x in t.values())


@pytest.mark.parametrize("kernel", ["adam_mixed", "sgd_momentum_mixed"])
def test_length_not_multiple_of_4_raises(gpu, kernel):
    n = 1027
    t = [torch.zeros(n, device=gpu) for _ in range(4)]
    with pytest.raises(RuntimeError, match=r"multiple of 4|% 4"):
        _mixed_call(kernel, *t, torch.zeros(n, device=gpu, dtype=BF))
