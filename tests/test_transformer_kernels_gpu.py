"""transformer.hip and flash_attn.hip against the float64 references of
tests/transformer_reference.py (1 GPU): attention (every dense forward / backward variant and the
flash kernels), LayerNorm, the embedding kernels, mlm_xent and act_grad, at the shapes that reach
each kernel's tiles, tails, routes and tie rules.  The same input sets and checks run on the
project's CPU path in tests/test_transformer_reference_cpu.py, which also asserts the reach
arithmetic.

Every kernel output is a ``Guarded`` tensor: NaN before the launch (a skipped tile or row cannot
pass on stale data), or the non-zero values an accumulating kernel must add to, between guard rows
that must come back untouched.  Each backward gets the reference's forward results rounded to the
kernel's input types, so it does not depend on the forward kernel.

Bounds (transformer_reference): one bf16 ulp + 2^-20 of the summed magnitudes, + 2^-8 of the
magnitudes behind every MFMA operand rounded to bf16 (P, dS); dQ, dK and dV each against its own.
Largest err / bound measured against the float64 reference on an MI355X, per kernel family:
dense attention forward 0.668, backward 0.696; flash forward 0.759, backward 0.658; LayerNorm
forward 0.498, backward 0.498 (the H = 768 kernel 0.498); embedding 0.498; mlm_xent 0.438;
act_grad 0.497.  (0.5 is the half ulp of a correctly rounded bf16 output.)  No kernel exceeded a
bound.  The module prints these figures when it finishes (``pytest -s``).
"""
import pytest
import torch

import layer_reference as L
import transformer_reference as R
from distributedtensorflowexample_amd.ops import transformer as ops
from distributedtensorflowexample_amd.ops._ext import hip, ptr, stream_handle

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    print("\nlargest err / bound per kernel family: " +
          ", ".join("%s %.3f" % kv for kv in sorted(R.RATIOS.items()) if kv[0] != "cpu"))


def _g(gpu, t):
    return None if t is None else t.to(gpu)


def _nan(gpu, shape, dtype):
    return R.Guarded(shape, dtype, gpu)


def _acc(gpu, init):
    return R.Guarded(tuple(init.shape), F32, gpu, fill=init)


def _done(*outs):
    """Synchronise, check every output's guards, return the bodies on the CPU."""
    torch.cuda.synchronize()
    return [None if o is None else o.check_guards("output %d" % i).cpu() for i, o in enumerate(outs)]


def _offset_view(gpu, t):
    """``t`` as a view that starts 4 bytes into a larger f32 buffer (a slice of a flat
    parameter buffer): not 16-byte aligned."""
    buf = torch.zeros(t.numel() + 8, device=gpu)
    v = buf[1:1 + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _aligned16(*ts):
    a = 0
    for t in ts:
        a |= t.data_ptr()
    return a % 16 == 0


# =========================================================================== attention
class _variants:
    def __init__(self, fwd=None, bwd=None):
        self.fwd, self.bwd = fwd, bwd

    def __enter__(self):
        h = hip()
        if self.fwd is not None:
            h.attn_fwd_set_variant(1 if self.fwd == "rp" else 0)
            h.attn_set_swizzle(1 if self.fwd == "lds_swz" else 0)
        if self.bwd is not None:
            var, swz, pf = R.BWD_VARIANTS[self.bwd]
            h.attn_bwd_set_variant(var)
            h.attn_set_swizzle(swz)
            h.attn_bwd_set_pf(pf)

    def __exit__(self, *exc):
        h = hip()
        h.attn_fwd_set_variant(-1)
        h.attn_bwd_set_variant(-1)
        h.attn_set_swizzle(-1)
        h.attn_bwd_set_pf(-1)


class _dev:
    """The GPU copies of one attention case's kernel inputs."""

    def __init__(self, gpu, c):
        self.qkv, self.dout, self.kmask, self.o = (_g(gpu, t) for t in (c.qkv, c.dout, c.kmask, c.o))
        self.lse = R.lse_padded(c.lse, c.S).to(gpu)  # NaN in the pitch's padding


def _attn_fwd(gpu, c, d, flash):
    out = _nan(gpu, (c.B * c.S, c.nh * 64), BF)
    lse = _nan(gpu, (c.B * c.nh, R.lse_ld(c.S)), F32)
    if flash:
        hip().flash_fwd(c.B, c.S, c.nh, ptr(d.qkv), ptr(out.t), ptr(lse.t), lse.t.shape[1],
                        ptr(d.kmask), float(c.scale), stream_handle())
    else:
        hip().attn_fwd(c.B, c.S, c.nh, ptr(d.qkv), ptr(out.t), ptr(lse.t), ptr(d.kmask),
                       float(c.scale), stream_handle())
    o, l = _done(out, lse)
    R.check_attn_fwd(o, l[:, :c.S], c.fwd, family="flash_fwd" if flash else "attention_fwd")


def _attn_bwd(gpu, c, d, flash):
    dqkv = _nan(gpu, tuple(c.qkv.shape), BF)
    dbias = _acc(gpu, c.dbias0)
    if flash:
        scratch = _nan(gpu, tuple(d.lse.shape), F32)
        hip().flash_bwd(c.B, c.S, c.nh, ptr(d.qkv), ptr(d.o), ptr(d.dout), ptr(d.lse), d.lse.shape[1],
                        ptr(d.kmask), float(c.scale), ptr(dqkv.t), ptr(dbias.t), ptr(scratch.t),
                        stream_handle())
        g, db, D = _done(dqkv, dbias, scratch)
        Dref = (c.o.double() * c.dout.double()).view(c.B, c.S, c.nh, 64).sum(-1).permute(0, 2, 1)
        Dmag = (c.o.double() * c.dout.double()).abs().view(c.B, c.S, c.nh, 64).sum(-1).permute(0, 2, 1)
        L.check_sum("D scratch", D[:, :c.S], Dref.reshape(c.B * c.nh, c.S), Dmag.reshape(c.B * c.nh, c.S))
    else:
        hip().attn_bwd(c.B, c.S, c.nh, ptr(d.qkv), ptr(d.o), ptr(d.dout), ptr(d.lse), ptr(d.kmask),
                       float(c.scale), ptr(dqkv.t), ptr(dbias.t), stream_handle())
        g, db = _done(dqkv, dbias)
    R.check_attn_bwd(g, c.bwd, c.nh, db, family="flash_bwd" if flash else "attention_bwd")


@pytest.mark.parametrize("kind", R.MASK_KINDS)
@pytest.mark.parametrize("S", R.DENSE_S)
def test_dense_attention(gpu, S, kind):
    """Every forward variant (register P, P through LDS, swizzled) and every backward variant
    (8 / 4 waves, two halves, persistent on one block per pair and on 3 blocks, swizzled halves,
    halves with the V warm-up, both together) at both scales, dbias added to non-zero values."""
    p = R.attn_plan(S)
    assert (p.key_tiles, p.fwd_waves, p.halves) == R.DENSE_REACH[S]
    for scale in R.ATTN_SCALES:
        c = R.attn_case(R.DENSE_B, S, R.DENSE_NH, kind, scale)
        d = _dev(gpu, c)
        for v in R.FWD_VARIANTS:
            with _variants(fwd=v):
                _attn_fwd(gpu, c, d, False)
        for v in R.BWD_VARIANTS:
            with _variants(bwd=v):
                _attn_bwd(gpu, c, d, False)


@pytest.mark.parametrize("S", [128, 33])
@pytest.mark.parametrize("B,nh", R.PERSIST_PAIRS)
def test_persistent_backward_uneven_and_even_grids(gpu, B, nh, S):
    """The 3-block persistent grid with 4 pairs (blocks of 2, 1 and 1) and with 12 (4 each)."""
    _, most, least = R.persist_plan(B * nh, "persist3")
    assert (most, least) == ((2, 1) if B * nh == 4 else (4, 4))
    for kind in ("prefix", "holes"):
        c = R.attn_case(B, S, nh, kind, 0.125)
        d = _dev(gpu, c)
        for v in ("persist3", "persist"):
            with _variants(bwd=v):
                _attn_bwd(gpu, c, d, False)


@pytest.mark.parametrize("kind", R.MASK_KINDS)
@pytest.mark.parametrize("S", R.FLASH_S)
def test_flash_attention(gpu, monkeypatch, S, kind):
    """The flash kernels at one to four 64-key tiles, ragged and whole, both scales; lse and the
    D scratch inside S; dbias added to non-zero values.  Once more through the public wrappers
    (DTFX_ATTN=flash below the switch point)."""
    assert R.flash_plan(R.FLASH_B, S, R.FLASH_NH).tiles == R.FLASH_REACH[S]
    for scale in R.ATTN_SCALES:
        c = R.attn_case(R.FLASH_B, S, R.FLASH_NH, kind, scale)
        d = _dev(gpu, c)
        _attn_fwd(gpu, c, d, True)
        _attn_bwd(gpu, c, d, True)
    if S <= 128:
        monkeypatch.setenv("DTFX_ATTN", "flash")
    o, lse = ops.attn_fwd(d.qkv, c.B, S, c.nh, d.kmask, scale)
    R.check_attn_fwd(o, lse[:, :S], c.fwd, family="flash_fwd")
    db = c.dbias0.to(gpu)
    g = ops.attn_bwd(d.qkv, d.o, d.dout, d.lse, c.B, S, c.nh, d.kmask, scale, dbias=db)
    R.check_attn_bwd(g, c.bwd, c.nh, db, family="flash_bwd")


@pytest.mark.parametrize("case,nwg,route", list(zip(R.FLASH_GRID_CASES, R.FLASH_GRIDS, R.FLASH_GRID_ROUTES)))
def test_flash_attention_grid_routes(gpu, case, nwg, route):
    """Grids of 1 and 7 (block ids as dealt), 9 and 13 (ragged XCD remap) and 16 (even remap)."""
    B, nh, S = case
    p = R.flash_plan(B, S, nh)
    assert (p.nwg, p.route) == (nwg, route)
    c = R.attn_case(B, S, nh, "holes", 0.2)
    d = _dev(gpu, c)
    _attn_fwd(gpu, c, d, True)
    _attn_bwd(gpu, c, d, True)


def test_dense_attention_public_wrappers(gpu):
    c = R.attn_case(R.DENSE_B, 77, R.DENSE_NH, "holes", 0.2)
    d = _dev(gpu, c)
    o, lse = ops.attn_fwd(d.qkv, c.B, c.S, c.nh, d.kmask, c.scale)
    R.check_attn_fwd(o, lse[:, :c.S], c.fwd)
    db = c.dbias0.to(gpu)
    g = ops.attn_bwd(d.qkv, d.o, d.dout, d.lse, c.B, c.S, c.nh, d.kmask, c.scale, dbias=db)
    R.check_attn_bwd(g, c.bwd, c.nh, db)


# =========================================================================== LayerNorm
def _ln_fwd(gpu, T, H, aligned):
    c = R.ln_case(T, H)
    gamma, beta = (_g(gpu, c.gamma), _g(gpu, c.beta)) if aligned else (
        _offset_view(gpu, c.gamma), _offset_view(gpu, c.beta))
    # the launcher routes gamma / beta off a 16-byte boundary to layernorm_fwd_kernel
    assert R.ln_fwd_plan(T, H, _aligned16(gamma, beta)).kernel == ("rows" if aligned else "one_row")
    y, mean, rstd = _nan(gpu, (T, H), BF), _nan(gpu, (T,), F32), _nan(gpu, (T,), F32)
    x = c.x.to(gpu)
    hip().layernorm_fwd(T, H, ptr(x), ptr(gamma), ptr(beta), 1e-12, ptr(y.t), ptr(mean.t),
                        ptr(rstd.t), stream_handle())
    R.check_layernorm_fwd(*_done(y, mean, rstd), R.ln_fwd_ref(T, H))


@pytest.mark.parametrize("H", R.LN_H)
def test_layernorm_forward(gpu, H):
    """1..4 column chunks on both sides of each boundary, T around the 16-row block, on the
    4-rows-per-wave kernel (aligned gamma / beta) and the one-row kernel (4-byte-offset views):
    the same bounds on both routes."""
    for T in R.LN_FWD_T:
        for aligned in (True, False):
            _ln_fwd(gpu, T, H, aligned)


def _ln_bwd(gpu, T, H, with_dres, with_dxsum, slots=2, h768=0, aligned=True):
    c = R.ln_case(T, H)
    mean, rstd = R.ln_stats(T, H)
    gamma = _g(gpu, c.gamma) if aligned else _offset_view(gpu, c.gamma)
    plan = R.ln_bwd_plan(T, H, slots, h768, _aligned16(gamma))
    dx = _nan(gpu, (T, H), BF)
    dg, db = _acc(gpu, c.dgamma0), _acc(gpu, c.dbeta0)
    ds = _acc(gpu, c.dxsum0) if with_dxsum else None
    dres = c.dres.to(gpu) if with_dres else None
    dy, x, mean, rstd = (t.to(gpu) for t in (c.dy, c.x, mean, rstd))
    h = hip()
    h.ln_bwd_set_slots(slots)
    h.ln_bwd_set_h768(h768)
    try:
        h.layernorm_bwd(T, H, ptr(dy), ptr(x), ptr(mean), ptr(rstd),
                        ptr(gamma), ptr(dres), ptr(dx.t), ptr(dg.t), ptr(db.t),
                        ptr(None if ds is None else ds.t), stream_handle())
        outs = _done(dx, dg, db, ds)
    finally:
        h.ln_bwd_set_slots(-1)
        h.ln_bwd_set_h768(-1)
    R.check_layernorm_bwd(*outs, R.ln_bwd_ref(T, H, with_dres, with_dxsum),
                          family="layernorm_bwd_h768" if plan.kernel == "h768" else "layernorm_bwd")
    return plan


@pytest.mark.parametrize("H", R.LN_H)
def test_layernorm_backward(gpu, H):
    """Row counts around the 8 (and 4) waves of a block and the 16-row block, 2 and 3 row slots,
    with and without dres and dxsum, all three accumulators added to non-zero values."""
    for T in R.LN_BWD_T:
        for slots in (2, 3):
            for with_dres, with_dxsum in ((True, True), (False, False), (True, False), (False, True)):
                plan = _ln_bwd(gpu, T, H, with_dres, with_dxsum, slots)
                assert plan.kernel == "generic" and plan.ns == (3 if slots == 3 and plan.nc <= 2 else 2)


@pytest.mark.parametrize("aligned", [True, False])
def test_layernorm_backward_h768_kernel(gpu, aligned):
    """layernorm_bwd_h768_kernel, and its fall-back to the generic kernel when gamma is a
    4-byte-offset view (its f32x4 gamma loads need 16-byte alignment)."""
    for T in R.LN_BWD_T:
        for with_dres, with_dxsum in ((True, True), (False, False)):
            plan = _ln_bwd(gpu, T, 768, with_dres, with_dxsum, 2, 1, aligned)
            assert plan.kernel == ("h768" if aligned else "generic")


@pytest.mark.parametrize("T,H", R.LN_BWD_LARGE)
def test_layernorm_backward_past_the_8192_row_switch(gpu, T, H):
    """64 rows per block (32 on the H = 768 kernel) with a ragged last block of 3 rows; every
    wave's rows exceed its slots, so the refill loads run."""
    for slots in (2, 3):
        plan = _ln_bwd(gpu, T, H, True, True, slots)
        assert (plan.rpb, plan.last_rows, plan.refills) == (64, 3, True)
    if H == 768:
        plan = _ln_bwd(gpu, T, H, True, True, 2, 1)
        assert (plan.kernel, plan.rpb, plan.last_rows, plan.refills) == ("h768", 32, 3, True)


def test_layernorm_public_wrappers(gpu):
    T, H = 33, 1032
    c = R.ln_case(T, H)
    y, mean, rstd = ops.layernorm_fwd(c.x.to(gpu), c.gamma.to(gpu), c.beta.to(gpu))
    R.check_layernorm_fwd(y, mean, rstd, R.ln_fwd_ref(T, H))
    m32, r32 = R.ln_stats(T, H)
    dg, db, ds = c.dgamma0.to(gpu), c.dbeta0.to(gpu), c.dxsum0.to(gpu)
    dx = ops.layernorm_bwd(c.dy.to(gpu), c.x.to(gpu), m32.to(gpu), r32.to(gpu), c.gamma.to(gpu), dg, db,
                           c.dres.to(gpu), ds)
    R.check_layernorm_bwd(dx, dg, db, ds, R.ln_bwd_ref(T, H, True, True))


# =========================================================================== embeddings
def _embedding(gpu, B, S, H, ids_kind, tt_kind):
    c = R.embed_case(B, S, H, ids_kind, tt_kind)
    ids, tt = c.ids.to(gpu), _g(gpu, c.tt)
    x, y = _nan(gpu, (c.T, H), BF), _nan(gpu, (c.T, H), BF)
    mean, rstd = _nan(gpu, (c.T,), F32), _nan(gpu, (c.T,), F32)
    word, pos, typ, gamma, beta, dx = (t.to(gpu) for t in (c.word, c.pos, c.type_, c.gamma, c.beta, c.dx))
    hip().embed_ln_fwd(c.T, S, H, ptr(ids), ptr(tt), ptr(word), ptr(pos), ptr(typ), ptr(gamma),
                       ptr(beta), 1e-12, ptr(x.t), ptr(y.t), ptr(mean.t), ptr(rstd.t), stream_handle())
    xo, yo, mo, ro = _done(x, y, mean, rstd)
    ref = R.embed_ln_fwd(c.ids, c.tt, c.word, c.pos, c.type_, c.gamma, c.beta, S)
    L.check_exact("x", xo, ref.x)
    R.check_layernorm_fwd(yo, mo, ro, ref, family="embedding")
    dw, dp, dt = _acc(gpu, c.dword0), _acc(gpu, c.dpos0), _acc(gpu, c.dtype0)
    hip().embed_bwd(B, S, H, ptr(ids), ptr(tt), ptr(dx), ptr(dw.t), ptr(dp.t), ptr(dt.t), stream_handle())
    R.check_embed_bwd(*_done(dw, dp, dt), R.embed_bwd(c.ids, c.tt, c.dx, c.dword0, c.dpos0, c.dtype0, B, S),
                      c.dpos0, S)


@pytest.mark.parametrize("B,S,H", R.embed_shapes())
def test_embedding_forward_backward(gpu, B, S, H):
    """Ragged last blocks (T % 4 != 0), the second 768-column pass of the word gradient, the
    second chunk trip (H > 1024) and batch trip (B > 32) of the position / type gradient; ids
    random, all equal (every atomic on one row) and {0, V - 1}; token types given, all 0, all 1
    and absent; the saved x exactly; the dpos rows past seq_len exactly as they were; every
    gradient added to non-zero values."""
    p = R.embed_plan(B, S, H)
    assert p.ragged_rows == ((B * S) % 4 != 0) and p.word_passes == (H + 767) // 768
    assert p.chunk_trips == (2 if H > 1024 else 1) and p.batch_trips == (2 if B > 32 else 1)
    for ids_kind, tt_kind in R.embed_kinds():
        _embedding(gpu, B, S, H, ids_kind, tt_kind)


def test_embedding_public_wrappers(gpu):
    c = R.embed_case(9, 4, 776, "random", "given")
    dev = [t.to(gpu) for t in (c.ids, c.tt, c.word, c.pos, c.type_, c.gamma, c.beta)]
    x, y, mean, rstd = ops.embed_ln_fwd(*dev, c.S)
    ref = R.embed_ln_fwd(c.ids, c.tt, c.word, c.pos, c.type_, c.gamma, c.beta, c.S)
    L.check_exact("x", x, ref.x)
    R.check_layernorm_fwd(y, mean, rstd, ref, family="embedding")
    g = [t.to(gpu) for t in (c.dword0, c.dpos0, c.dtype0)]
    ops.embed_bwd(dev[0], dev[1], c.dx.to(gpu), *g, c.B, c.S)
    R.check_embed_bwd(*g, R.embed_bwd(c.ids, c.tt, c.dx, c.dword0, c.dpos0, c.dtype0, c.B, c.S), c.dpos0, c.S)


# =========================================================================== mlm_xent
def _xent(gpu, logits, lab, C, ld, regs, want_kernel=None):
    N = logits.shape[0]
    lp = R.xent_padded(logits, ld).to(gpu)
    loss, correct = _nan(gpu, (N,), F32), _nan(gpu, (N,), F32)
    dl = _nan(gpu, (N, ld), BF)
    bf = logits.dtype == BF
    if want_kernel is not None:
        assert R.xent_plan(C, ld, bf, regs, _aligned16(lp, dl.t)).kernel == want_kernel
    labels = lab.to(gpu)
    h = hip()
    h.xent_set_regs(regs)
    try:
        h.mlm_xent(N, C, ptr(lp), ld, ptr(labels), float(R.XENT_SCALE), ptr(loss.t), ptr(correct.t),
                   ptr(dl.t), ld, stream_handle(), bf)
        outs = _done(loss, correct, dl)
    finally:
        h.xent_set_regs(-1)
    R.check_mlm_xent(*outs, R.mlm_xent(lp.cpu(), lab, C, R.XENT_SCALE, ld), C)
    return outs


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", R.XENT_C)
def test_mlm_xent(gpu, C, dtype):
    """Both kernels at the chunk edges, with ld = C rounded up to 8, ld % 8 == 4 (the register
    kernel falls back) and ld far above C (padding that would win the arg-max if read); arg-max
    ties inside a chunk, across lanes, waves, one thread's chunks and against the tails, labelled
    on either tied index; labels 0, C - 1 and -100; a batch with every row ignored."""
    logits, lab, _ = R.xent_case(C, dtype)
    ld8, ld4 = R.xent_lds(C)
    bf = dtype == BF
    for regs in (1, 0):
        _xent(gpu, logits, lab, C, ld8, regs, "regs" if bf and regs else "two_pass")
        _xent(gpu, logits, lab, C, ld4, regs, "two_pass")
        _xent(gpu, logits, lab, C, ld8 + 1024, regs, "regs" if bf and regs else "two_pass")
        loss, correct, dl = _xent(gpu, logits, torch.full_like(lab, -100), C, ld8, regs)
        for name, t in (("loss", loss), ("correct", correct), ("dlogits", dl)):
            L.check_exact("all rows ignored: " + name, t, torch.zeros_like(t))


def test_mlm_xent_past_the_register_kernel_columns(gpu):
    N, C = R.XENT_BIG
    logits, lab, ties = R.xent_case(C, BF, N)
    assert len(ties) == N
    for regs in (1, 0):
        _xent(gpu, logits, lab, C, C, regs, "two_pass")


def test_mlm_xent_public_wrapper(gpu):
    C = 2049
    for dtype in (F32, BF):
        logits, lab, _ = R.xent_case(C, dtype)
        ld = R.xent_lds(C)[0]
        lp = R.xent_padded(logits, ld)
        loss, correct, dl = ops.mlm_xent(lp.to(gpu), lab.to(gpu), C, R.XENT_SCALE)
        R.check_mlm_xent(loss, correct, dl, R.mlm_xent(lp, lab, C, R.XENT_SCALE, ld), C)


# =========================================================================== act_grad
@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_act_grad(gpu, act):
    """One to two blocks, +-0, the saturated range, and the first size past the 4096-block cap
    (its last group of 8 is a second grid-stride pass)."""
    sizes = R.ACT_N + (R.act_grad_wrap_size(),)
    assert [R.act_grad_blocks(n)[1] for n in sizes] == [1, 1, 1, 1, 2]
    for n in sizes:
        u, dy = R.act_case(n)
        dx = _nan(gpu, (n,), BF)
        dyg, ug = dy.to(gpu), u.to(gpu)
        hip().act_grad_bf16(n, {"gelu": 1, "relu": 2}[act], ptr(dyg), ptr(ug), ptr(dx.t), stream_handle())
        R.check_act_grad(_done(dx)[0], R.act_grad(dy, u, act), dy)
    u, dy = R.act_case(2056)
    R.check_act_grad(ops.act_grad(dy.to(gpu), u.to(gpu), act), R.act_grad(dy, u, act), dy)
