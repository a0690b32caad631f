"""The BatchNorm, pooling and colpart_reduce kernels of cnn.hip against the float64 references
of tests/layer_reference.py, at the shapes that reach each kernel's alternate path (1 GPU).  The
same input sets and comparison helpers run on the project's CPU path in
tests/test_layer_reference_cpu.py.  Where a branch depends on launch arithmetic the test
asserts, from the constants in the .hip source, that its shape reaches it.

Bounds (layer_reference): bf16 outputs one bf16 ulp of the exact value + 2^-20 of the summed
term magnitudes; f32 column sums 2^-20 sum|terms|; means 1e-5, rstd / variances 1e-4 relative;
``dres``, ``y`` and ``idx`` of the max pool exactly."""
import pytest
import torch

import layer_reference as R
from distributedtensorflowexample_amd.ops import cnn

pytestmark = pytest.mark.gpu

# what each BatchNorm set is there for (asserted from the launch constants)
BN_PATH = {(197, 8): "fast", (1500, 8): "fast", (197, 64): "fast", (37, 2056): "general",
           (100, 96): "fast", (60, 96): "general", R.BN_LARGE: "fast"}


def _dev(c, gpu):
    return {k: v.to(gpu) for k, v in vars(c).items() if isinstance(v, torch.Tensor)}


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("M,C", R.BN_SETS)
def test_bn_apply(gpu, M, C, with_res, relu):
    """bn_apply_kernel: one channel group (C = 8), the fast path with a non-power-of-two group
    count (M = 100, C = 96: stride % 12 == 0), the general per-element channel loop (M = 60,
    C = 96 and C = 2056), residual and ReLU on and off."""
    assert R.bn_stream_path(M, C) == BN_PATH[(M, C)]
    c, g = R.bn_case(M, C), _dev(R.bn_case(M, C), gpu)
    ref, mag = R.bn_apply_ref(M, C, with_res, relu)
    y = cnn.bn_apply(g["x"], g["mean"], g["rstd"], g["gamma"], g["beta"],
                     g["res"] if with_res else None, relu)
    R.check_bf16("y", y, ref, mag)
    assert torch.equal(g["x"].cpu(), c.x) and torch.equal(g["res"].cpu(), c.res)


@pytest.mark.parametrize("M,C", [(100, 96), (60, 96), (197, 8)])
def test_bn_apply_stats(gpu, M, C):
    """The fused finalize + apply on the fast path with 12 channel groups, on the general loop
    and at C = 8: output, mean / rstd and running statistics from non-trivial starting values."""
    assert R.bn_stream_path(M, C) == BN_PATH[(M, C)]
    c, g = R.bn_case(M, C), _dev(R.bn_case(M, C), gpu)
    rm0 = R.randn(C, seed=1) * 0.5
    rv0 = torch.rand(C, generator=torch.Generator().manual_seed(2)) + 0.5
    fin = R.bn_finalize(c.s, c.q, M, 1e-5, rm0, rv0, 0.9)
    ref, mag = R.bn_apply(c.x, fin.mean, fin.rstd, c.gamma, c.beta, c.res, True)
    rm, rv = rm0.to(gpu), rv0.to(gpu)
    y, mean, rstd = cnn.bn_apply_stats(g["x"], g["s"], g["q"], M, g["gamma"], g["beta"], g["res"],
                                       True, 1e-5, rm, rv)
    R.check_bf16("y", y, ref, mag)
    R.check_close("mean", mean, fin.mean, atol=R.TOL_MEAN)
    R.check_close("rstd", rstd, fin.rstd, atol=1e-8, rtol=R.TOL_RSTD)
    R.check_close("run_mean", rm, fin.run_mean, atol=R.TOL_MEAN)
    R.check_close("run_var", rv, fin.run_var, atol=1e-8, rtol=R.TOL_RSTD)


BWD_MODES = {  # relu, want_dres, grads_zeroed
    "relu_dres_accumulate": (True, True, False),
    "plain_zeroed": (False, False, True),
    "relu_zeroed": (True, False, True),
    "plain_dres": (False, True, False),
}


def _check_bwd(M, C, relu, dx, dres, dg, db, dg0=None, db0=None):
    ref = R.bn_bwd_ref(M, C, relu)
    zero = torch.zeros(C, dtype=torch.float64)
    dg0 = zero if dg0 is None else dg0.double()
    db0 = zero if db0 is None else db0.double()
    # (dgamma0 + sum is one more f32 addition: its operand joins the magnitudes)
    R.check_sum("dgamma", dg, dg0 + ref.sum_dyxh, ref.mag_dyxh + dg0.abs())
    R.check_sum("dbeta", db, db0 + ref.sum_dy, ref.mag_dy + db0.abs())
    if dx is not None:
        R.check_bf16("dx", dx.reshape(M, C), ref.dx, ref.mag_dx)
    if dres is not None:
        R.check_exact("dres", dres.reshape(M, C), ref.dres)


@pytest.mark.parametrize("mode", list(BWD_MODES))
@pytest.mark.parametrize("M,C", R.BN_SETS)
def test_bn_bwd(gpu, M, C, mode):
    """bn_bwd_reduce / colpart_reduce / bn_bwd_apply: C = 8 (256 rows per pass; two blocks at
    M = 1500), 12 threads per row with idle threads (C = 96), the second channel pass (C = 2056),
    the general apply loop; relu / want_dres on and off; sums straight into zeroed slots, or
    added to non-zero dgamma / dbeta."""
    relu, want_dres, zeroed = BWD_MODES[mode]
    plan = R.bn_bwd_reduce_plan(M, C)
    assert R.bn_stream_path(M, C) == BN_PATH[(M, C)]
    assert plan.passes == (2 if C > 2048 else 1) and plan.rpp == 256 // min(C // 8, 256)
    assert not plan.from_m and plan.blocks == {(197, 8): 1, (1500, 8): 2}.get((M, C), plan.blocks)
    g = _dev(R.bn_case(M, C), gpu)
    dg0 = db0 = None
    if zeroed:
        dg, db = torch.zeros(C, device=gpu), torch.zeros(C, device=gpu)
    else:
        dg0, db0 = R.randn(C, seed=3) * 4, R.randn(C, seed=4) * 4
        dg, db = dg0.clone().to(gpu), db0.clone().to(gpu)
    dx, dres = cnn.bn_bwd(g["dy"], g["y"], g["x"], g["mean"], g["rstd"], g["gamma"], dg, db,
                          relu=relu, want_dres=want_dres, grads_zeroed=zeroed)
    assert (dres is not None) == want_dres
    _check_bwd(M, C, relu, dx, dres, dg, db, dg0, db0)


@pytest.mark.parametrize("M,C", [(197, 64), (37, 2056), (60, 96)])
def test_bn_bwd_reductions_only(gpu, M, C):
    """apply=False: the two sums only, (None, None) returned; with a ReLU mask it raises."""
    g = _dev(R.bn_case(M, C), gpu)
    dg, db = torch.zeros(C, device=gpu), torch.zeros(C, device=gpu)
    out = cnn.bn_bwd(g["dy"], g["y"], g["x"], g["mean"], g["rstd"], g["gamma"], dg, db,
                     relu=False, grads_zeroed=True, apply=False)
    assert out == (None, None)
    _check_bwd(M, C, False, None, None, dg, db)
    for kw in ({"relu": True}, {"relu": False, "want_dres": True}):
        with pytest.raises(ValueError):
            cnn.bn_bwd(g["dy"], g["y"], g["x"], g["mean"], g["rstd"], g["gamma"], dg, db,
                       grads_zeroed=True, apply=False, **kw)


def test_bn_rows_per_block_from_m(gpu):
    """M = 131073 + 76, C = 64: the smallest row count class where bn_bwd's rows per block come
    from M (129 > 4 * 32) -- forward (2050 blocks) and backward, the largest tensors here."""
    M, C = R.BN_LARGE
    plan = R.bn_bwd_reduce_plan(M, C)
    assert plan.from_m and plan.rpb == 129 and M % plan.rpb and R.bn_stream_path(M, C) == "fast"
    assert not R.bn_bwd_reduce_plan(131072, C).from_m and R.bn_bwd_reduce_plan(131073, C).from_m
    g = _dev(R.bn_case(M, C), gpu)
    ref, mag = R.bn_apply_ref(M, C, True, True)
    y = cnn.bn_apply(g["x"], g["mean"], g["rstd"], g["gamma"], g["beta"], g["res"], True)
    R.check_bf16("y", y, ref, mag)
    dg, db = torch.zeros(C, device=gpu), torch.zeros(C, device=gpu)
    dx, dres = cnn.bn_bwd(g["dy"], g["y"], g["x"], g["mean"], g["rstd"], g["gamma"], dg, db,
                          relu=True, want_dres=True, grads_zeroed=True)
    _check_bwd(M, C, True, dx, dres, dg, db)


@pytest.mark.parametrize("C,M,clamp", R.BN_FINALIZE_CASES)
def test_bn_finalize(gpu, C, M, clamp):
    """bn_finalize_kernel: C = 1, a partial second block (C = 257), M = 1 (unbias = 1), a channel
    of equal large values whose f32 variance rounds negative (the clamp gives rstd =
    rsqrt(eps)), running statistics from non-trivial starting values."""
    s, q, rm0, rv0 = R.bn_finalize_case(C, M, clamp)
    fin = R.bn_finalize(s, q, M, 1e-5, rm0, rv0, 0.9)
    rm, rv = rm0.to(gpu), rv0.to(gpu)
    mean, rstd = cnn.bn_finalize(s.to(gpu), q.to(gpu), M, 1e-5, rm, rv, 0.9)
    R.check_close("mean", mean, fin.mean, atol=R.TOL_MEAN)
    R.check_close("rstd", rstd, fin.rstd, atol=1e-8, rtol=R.TOL_RSTD)
    R.check_close("run_mean", rm, fin.run_mean, atol=R.TOL_MEAN)
    R.check_close("run_var", rv, fin.run_var, atol=1e-8, rtol=R.TOL_RSTD)
    if clamp:
        assert float(fin.var[0]) == 0.0
        assert all(v < 0 for v in R.f32_variances(float(s[0]), float(q[0]), M)[0][:3])
    # without running statistics nothing else is written
    mean2, rstd2 = cnn.bn_finalize(s.to(gpu), q.to(gpu), M, 1e-5)
    assert torch.equal(mean2, mean) and torch.equal(rstd2, rstd)


# ------------------------------------------------------------------ pools
def _maxpool(gpu, shape, kind):
    x, dy = R.maxpool_case(shape, kind)
    yr, idxr, dxr = R.maxpool_ref(shape, kind)
    X = x.to(gpu)
    y, idx = cnn.maxpool_fwd(X)
    R.check_exact("y", y, yr)
    R.check_exact("idx", idx, idxr)
    assert torch.equal(X.cpu(), x)
    # at most four bf16 addends summed in f32, rounded once: one bf16 ulp of the exact sum
    R.check_bf16("dx (own idx)", cnn.maxpool_bwd(dy.to(gpu), idx, shape), dxr)
    R.check_bf16("dx (reference idx)", cnn.maxpool_bwd(dy.to(gpu), idxr.to(gpu), shape), dxr)


@pytest.mark.parametrize("kind", R.MAXPOOL_KINDS)
@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES)
def test_maxpool(gpu, shape, kind):
    """H, W of 1 and 2, C = 8, odd and even extents, two x blocks forward / three backward
    (C = 264); random values, mostly tied windows (first valid tap wins), an all-negative image
    (padding never wins): y and idx exactly."""
    plan = R.maxpool_plan(shape)
    assert plan.xblocks_fwd == (2 if shape[3] == 264 else 1) and not plan.loops_fwd
    _maxpool(gpu, shape, kind)


def test_maxpool_row_loop(gpu):
    """N * OH = 65536 > 65535 grid rows forward, N * H = 98304 backward: both row loops."""
    plan = R.maxpool_plan(R.MAXPOOL_ROWLOOP)
    assert plan.loops_fwd and plan.loops_bwd
    _maxpool(gpu, R.MAXPOOL_ROWLOOP, "ties")


@pytest.mark.parametrize("shape", R.AVGPOOL_SHAPES)
def test_avgpool(gpu, shape):
    """HW = 1, C % 8 != 0, N * C % 256 != 0 (a partial block)."""
    N, H, W, C = shape
    assert (N * C) % R.launch_constants().avg_block
    x, dy = R.avgpool_case(shape)
    ref, mag = R.avgpool_fwd(x)
    R.check_bf16("y", cnn.avgpool_fwd(x.to(gpu)), ref, mag)
    dref = R.avgpool_bwd(dy, shape)
    R.check_bf16("dx", cnn.avgpool_bwd(dy.to(gpu), shape), dref, dref.abs())


def test_avgpool_bwd_second_pass(gpu):
    """2,102,784 elements > 8192 * 256: the backward's second grid-stride pass."""
    shape = R.AVGPOOL_BWD_WRAP
    N, H, W, C = shape
    assert R.grid_for_passes(N * H * W * C) == (R.launch_constants().for_cap, 2)
    _, dy = R.avgpool_case(shape)
    dref = R.avgpool_bwd(dy, shape)
    R.check_bf16("dx", cnn.avgpool_bwd(dy.to(gpu), shape), dref, dref.abs())
