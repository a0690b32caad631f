"""float64 references for the transformer kernels (csrc/kernels/transformer.hip and
flash_attn.hip): LayerNorm, embedding + LayerNorm, attention, ``act_grad`` and ``mlm_xent``,
written from each operation's definition.  Nothing here imports ``ops/``.

Shared by the CPU tier (tests/test_transformer_reference_cpu.py) and the GPU tests
(tests/test_transformer_kernels_gpu.py); the conventions are those of tests/layer_reference.py:

* one function per operation, plain torch float64.  Each BACKWARD is the exact function of the
  kernel's inputs: it takes the ``mean`` / ``rstd``, ``o``, ``lse`` tensors the kernel is given
  (the tests hand the kernel the reference's forward results rounded to the kernel's input
  types), so a backward test does not depend on the forward kernel.  Every function returns,
  next to its result, the magnitudes its bound is made of;
* the bounds: one bf16 ulp ``2^-7 |ref|`` for a bf16 output plus ``2^-20`` times the summed
  magnitudes for the f32 arithmetic, plus one named term for every place a kernel rounds an MFMA
  operand to bf16 (P before P.V and P^T.dO, dS before dS.K and dS^T.Q);
* deterministic input builders, so both tiers see the same tensors;
* the launch arithmetic with its constants read from the ``.hip`` sources: a GPU case asserts
  with it that its shape reaches the branch it names;
* ``Guarded``: an output that sits inside a larger buffer, pre-filled with NaN (or with the
  values an accumulating kernel must add to) between guard rows that must come back untouched.
"""
import functools
import math
import types

import torch

import layer_reference as L
from layer_reference import BF, BF16_ULP, F32_TERMS, TOL_ACT, TOL_LOSS, TOL_PROB, TOL_RSTD, _d, f32

HD = 64                   # head dimension of every attention kernel
P_ROUND = 2.0 ** -8       # one bf16 rounding of an MFMA operand in [0, 1] scale: P, dS (relative)
EXP_REL = 2.0 ** -16      # fast exp of the backward's P = exp(s - lse), relative
F32_HALF_ULP2 = 2.0 ** -23  # the f32 rounding of score * scale + mask, relative to |s| + |mask|
TOL_LSE = 1e-4            # __expf / __logf in the log-sum-exp (test_attention_fwd_register_p_matches_lds_p)

RATIOS = {}  # kernel family -> largest err / bound seen by the checks below


def _note(family, ratio):
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    return ratio


def check_bound(name, out, ref, bound):
    """|out - ref| <= bound element by element (a NaN fails); returns the largest err / bound."""
    out = _d(out)
    L._same_shape(name, out, ref)
    return L._worst(name, (out - ref).abs(), bound)


# =========================================================================== LayerNorm
def layernorm_fwd(x, gamma, beta, eps=1e-12):
    """y = (x - mean) rstd gamma + beta over the last axis, biased variance, rstd =
    1 / sqrt(var + eps).  mag_y counts x-hat as (|x| + |mean|) rstd: a row with a large mean is
    bounded by its conditioning."""
    x, gamma, beta = _d(x), _d(gamma), _d(beta)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    y = (x - mean[:, None]) * rstd[:, None] * gamma + beta
    mag_y = (x.abs() + mean.abs()[:, None]) * rstd[:, None] * gamma.abs() + beta.abs()
    return types.SimpleNamespace(y=y, mean=mean, rstd=rstd, mag_y=mag_y, mag_mean=x.abs().mean(1))


def check_layernorm_fwd(y, mean, rstd, ref, family="layernorm_fwd"):
    r = [check_bound("mean", mean, ref.mean, F32_TERMS * ref.mag_mean),
         L.check_close("rstd", rstd, ref.rstd, rtol=TOL_RSTD),
         L.check_bf16("y", y, ref.y, ref.mag_y)]
    return _note(family, max(r))


def layernorm_bwd(dy, x, mean, rstd, gamma, dres=None, dgamma0=None, dbeta0=None, dxsum0=None):
    """dx = rstd (g - mean(g) - xhat mean(g xhat)) [+ dres], g = dy gamma, xhat = (x - mean) rstd
    with the GIVEN mean / rstd; dgamma = dgamma0 + sum dy xhat, dbeta = dbeta0 + sum dy,
    dxsum = dxsum0 + sum dx (the unrounded dx) over the rows."""
    dy, x, gamma = _d(dy), _d(x), _d(gamma)
    mean, rstd = _d(mean)[:, None], _d(rstd)[:, None]
    H = x.shape[1]
    xh = (x - mean) * rstd
    xm = (x.abs() + mean.abs()) * rstd  # x-hat's magnitude before the cancellation
    g = dy * gamma
    s2 = (g * xh).mean(1, keepdim=True)
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * s2)
    # first order in the roundings: x-hat's error (2^-24 xm) meets the exact s2, s2's error
    # (2^-24 mean |g| xm) the exact x-hat
    mag = rstd * (g.abs() + g.abs().mean(1, keepdim=True) + xm * s2.abs()
                  + xh.abs() * (g.abs() * xm).mean(1, keepdim=True))
    if dres is not None:
        dx = dx + _d(dres)
        mag = mag + _d(dres).abs()
    z = torch.zeros(H, dtype=torch.float64)
    i0, i1, i2 = (z if t is None else _d(t) for t in (dgamma0, dbeta0, dxsum0))
    return types.SimpleNamespace(
        dx=dx, mag_dx=mag,
        dgamma=i0 + (dy * xh).sum(0), mag_dgamma=i0.abs() + (dy.abs() * xm).sum(0),
        dbeta=i1 + dy.sum(0), mag_dbeta=i1.abs() + dy.abs().sum(0),
        dxsum=i2 + dx.sum(0), mag_dxsum=i2.abs() + mag.sum(0))


def check_layernorm_bwd(dx, dgamma, dbeta, dxsum, ref, family="layernorm_bwd"):
    r = [L.check_bf16("dx", dx, ref.dx, ref.mag_dx),
         L.check_sum("dgamma", dgamma, ref.dgamma, ref.mag_dgamma),
         L.check_sum("dbeta", dbeta, ref.dbeta, ref.mag_dbeta)]
    if dxsum is not None:
        r.append(L.check_sum("dxsum", dxsum, ref.dxsum, ref.mag_dxsum))
    return _note(family, max(r))


# =========================================================================== embeddings
def embed_ln_fwd(ids, tt, word, pos, type_, gamma, beta, seq_len, eps=1e-12):
    """x = word[ids] + pos[t mod seq_len] + type[tt] (tt None: type 0) rounded ONCE to bf16 --
    the sum of three bf16 values is exact in float64 -- then LayerNorm of that bf16 x."""
    ids = ids.detach().cpu().long().view(-1)
    T = ids.numel()
    t = torch.zeros_like(ids) if tt is None else tt.detach().cpu().long().view(-1)
    p = torch.arange(T) % seq_len
    xs = _d(word)[ids] + _d(pos)[p] + _d(type_)[t]
    x = xs.to(BF)
    ref = layernorm_fwd(x, gamma, beta, eps)
    ref.x = x.double()
    ref.x_exact_sum = xs
    return ref


def embed_bwd(ids, tt, dx, dword0, dpos0, dtype0, batch, seq_len):
    """dword[v] = dword0[v] + sum of the dx rows with id v; dpos[s] = dpos0[s] + sum over the
    batch of dx[b, s] for s < seq_len and dpos0[s] beyond; dtype[k] = dtype0[k] + sum of the rows
    of type k (tt None: all type 0).  The kernel forms the type-0 sum of a position as (all rows)
    - (type-1 rows), so dtype[0]'s magnitude counts the type-1 rows twice."""
    ids = ids.detach().cpu().long().view(-1)
    g = _d(dx)
    H = g.shape[1]
    t = torch.zeros_like(ids) if tt is None else tt.detach().cpu().long().view(-1)
    dword, dpos, dtyp = _d(dword0).clone(), _d(dpos0).clone(), _d(dtype0).clone()
    mw, mp, mt = dword.abs(), dpos.abs(), dtyp.abs()
    dword.index_add_(0, ids, g)
    mw.index_add_(0, ids, g.abs())
    dpos[:seq_len] += g.view(batch, seq_len, H).sum(0)
    mp[:seq_len] += g.abs().view(batch, seq_len, H).sum(0)
    dtyp.index_add_(0, t, g)
    one = (g.abs() * (t == 1)[:, None]).sum(0)
    mt[0] += g.abs().sum(0) + one
    mt[1] += one
    return types.SimpleNamespace(dword=dword, dpos=dpos, dtype=dtyp, mag_dword=mw, mag_dpos=mp,
                                 mag_dtype=mt)


def check_embed_bwd(dword, dpos, dtyp, ref, dpos0, seq_len, family="embedding"):
    r = [L.check_sum("dword", dword, ref.dword, ref.mag_dword),
         L.check_sum("dpos", dpos, ref.dpos, ref.mag_dpos),
         L.check_sum("dtype", dtyp, ref.dtype, ref.mag_dtype)]
    L.check_exact("dpos rows past seq_len", _d(dpos)[seq_len:], _d(dpos0)[seq_len:])
    return _note(family, max(r))


# =========================================================================== attention
def _split(qkv, B, S, nh):
    t = _d(qkv).view(B, S, 3, nh, HD).permute(2, 0, 3, 1, 4)  # [3, B, nh, S, d]
    return t[0], t[1], t[2]


def _heads(t, B, S, nh):
    return _d(t).view(B, S, nh, HD).permute(0, 2, 1, 3)  # [B, nh, S, d]


def _merge(t, B, S, nh):
    return t.permute(0, 2, 1, 3).reshape(B * S, nh * HD)


def _merge3(dq, dk, dv, B, S, nh):
    return torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B * S, 3 * nh * HD)


def _mask(kmask, B, S):
    """(additive mask [B, 1, 1, S], its magnitude with 0 at the -inf keys, which carry P = 0)."""
    if kmask is None:
        m = torch.zeros(B, 1, 1, S, dtype=torch.float64)
    else:
        m = _d(kmask).view(B, 1, 1, S)
    return m, torch.where(torch.isinf(m), torch.zeros_like(m), m.abs())


def attn_fwd(qkv, B, S, nh, kmask=None, scale=0.125):
    """o = softmax(q k^T scale + mask) v per (sequence, head), lse = logsumexp of the scores.
    qkv [B S, 3 nh 64] (Q | K | V, head-major); returns o [B S, nh 64], lse [B nh, S],
    mag_o = sum_k p_k |v_k| and mag_lse = |lse| + sum_k p_k (scale sum_d |q_d||k_d| + |mask_k|):
    d lse / d s_k = p_k."""
    q, k, v = _split(qkv, B, S, nh)
    scale = f32(scale)
    m, mabs = _mask(kmask, B, S)
    s = q @ k.transpose(-1, -2) * scale + m
    mx = s.max(-1, keepdim=True).values
    e = torch.exp(s - mx)
    l = e.sum(-1, keepdim=True)
    p = e / l
    lse = (mx + torch.log(l)).squeeze(-1)
    smag = (q.abs() @ k.abs().transpose(-1, -2)) * scale + mabs
    return types.SimpleNamespace(
        o=_merge(p @ v, B, S, nh), mag_o=_merge(p @ v.abs(), B, S, nh), p=p,
        lse=lse.reshape(B * nh, S), mag_lse=(lse.abs() + (p * smag).sum(-1)).reshape(B * nh, S))


def check_attn_fwd(o, lse, ref, family="attention_fwd"):
    """o: one bf16 ulp + P rounded to bf16 (2^-8 sum_k p_k |v_k|).  lse (already cut to
    [B nh, S]): 2^-20 of its magnitudes + the fast exp / log's 1e-4."""
    r = [check_bound("o", o, ref.o, BF16_ULP * ref.o.abs() + P_ROUND * ref.mag_o),
         check_bound("lse", lse, ref.lse, F32_TERMS * ref.mag_lse + TOL_LSE)]
    return _note(family, max(r))


def attn_bwd(qkv, o, dout, lse, B, S, nh, kmask=None, scale=0.125, dbias0=None):
    """The exact backward of the given (qkv, o, dout, lse): p = exp(q k^T scale + mask - lse),
    D = sum_d dO o, dp = dO v^T, ds = p (dp - D), dV = p^T dO, dK = scale ds^T q,
    dQ = scale ds k; g in the qkv layout.  ``lse`` [B nh, >= S].

    Per-element error model of ds (e_ds): the f32 sums dp and D, 2^-20 p (sum_d |dO||v| +
    sum_d |dO||o|); the fast exp, 2^-16 |ds|; the f32 rounding of score * scale + mask before the
    exp, 2^-23 (|s| + |mask|) |ds| (at mask = -10000 the f32 spacing is 1e-3 in the exponent).
    ``extra`` is each output's bound WITHOUT its own bf16 rounding:
      dV: 2^-8 sum_q p |dO|                      (P rounded to bf16)
      dK: scale sum_q (2^-8 |ds| + e_ds) |q|     (dS rounded to bf16)
      dQ: scale sum_k (2^-8 |ds| + e_ds) |k|
    ``mag``: the summed magnitudes of each output.  dbias = dbias0 + column sums of g, bound
    sum_rows extra + 2^-20 (sum_rows mag + |dbias0|)."""
    q, k, v = _split(qkv, B, S, nh)
    do, of = _heads(dout, B, S, nh), _heads(o, B, S, nh)
    scale = f32(scale)
    m, mabs = _mask(kmask, B, S)
    lv = _d(lse).view(B, nh, -1)[..., :S, None]
    raw = q @ k.transpose(-1, -2) * scale
    p = torch.exp(raw + m - lv)
    Dr = (do * of).sum(-1, keepdim=True)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - Dr)
    dv = p.transpose(-1, -2) @ do
    dk = ds.transpose(-1, -2) @ q * scale
    dq = ds @ k * scale
    e_ds = (p * F32_TERMS * (do.abs() @ v.abs().transpose(-1, -2) + (do * of).abs().sum(-1, keepdim=True))
            + EXP_REL * ds.abs() + F32_HALF_ULP2 * (raw.abs() + mabs) * ds.abs())
    w = P_ROUND * ds.abs() + e_ds
    x_dv = P_ROUND * (p.transpose(-1, -2) @ do.abs())
    x_dk = w.transpose(-1, -2) @ q.abs() * scale
    x_dq = w @ k.abs() * scale
    m_dv = p.transpose(-1, -2) @ do.abs()
    m_dk = ds.abs().transpose(-1, -2) @ q.abs() * scale
    m_dq = ds.abs() @ k.abs() * scale
    g = _merge3(dq, dk, dv, B, S, nh)
    extra = _merge3(x_dq, x_dk, x_dv, B, S, nh)
    mag = _merge3(m_dq, m_dk, m_dv, B, S, nh)
    b0 = torch.zeros(3 * nh * HD, dtype=torch.float64) if dbias0 is None else _d(dbias0)
    return types.SimpleNamespace(g=g, extra=extra, mag=mag, p=p, ds=ds, dbias=b0 + g.sum(0),
                                 bound_dbias=extra.sum(0) + F32_TERMS * (mag.sum(0) + b0.abs()))


def third(t, which, nh):
    """The dQ (0), dK (1) or dV (2) columns of a tensor in the qkv layout."""
    return t[..., which * nh * HD:(which + 1) * nh * HD]


def check_attn_bwd(dqkv, ref, nh, dbias=None, family="attention_bwd"):
    """dQ, dK and dV each against its own bound (one bf16 ulp + ``extra``), dbias against its."""
    out = _d(dqkv)
    L._same_shape("dqkv", out, ref.g)
    r = []
    for i, name in enumerate(("dQ", "dK", "dV")):
        gi = third(ref.g, i, nh)
        r.append(check_bound(name, third(out, i, nh), gi, BF16_ULP * gi.abs() + third(ref.extra, i, nh)))
    if dbias is not None:
        r.append(check_bound("dbias", dbias, ref.dbias, ref.bound_dbias))
    return _note(family, max(r))


# =========================================================================== act_grad / mlm_xent
def act_grad(dy, u, act):
    """dy act'(u), act in {"gelu" (tanh form), "relu"}; the derivative by float64 autograd."""
    return L.activation_grad(dy, u, {"gelu": 3, "relu": 2}[act])


def check_act_grad(dx, ref, dy, family="act_grad"):
    return _note(family, check_bound("act_grad", dx, ref, BF16_ULP * ref.abs() + TOL_ACT * _d(dy).abs()))


def mlm_xent(logits, labels, C, scale, ld):
    """layer_reference.softmax_xent over the first C columns; dlogits [N, ld] with the columns
    [C, ld) zero.  Also lse's magnitude for the loss bound."""
    l = _d(logits)[:, :C]
    ref = L.softmax_xent(l, labels, scale=scale)
    d = torch.zeros(l.shape[0], ld, dtype=torch.float64)
    d[:, :C] = ref.dlogits
    ref.dlogits_ld = d
    lab = labels.detach().cpu().long()
    valid = (lab >= 0) & (lab < C)
    ly = l.gather(1, lab.clamp(0, C - 1)[:, None]).squeeze(1)
    ref.mag_loss = torch.where(valid, (ref.loss + ly).abs() + ly.abs(), torch.zeros_like(ly))
    return ref


def check_mlm_xent(loss, correct, dl, ref, C, family="mlm_xent"):
    """loss: the fast exp / log's 1e-5 + 2^-20 (|lse| + |logit_y|); dlogits / scale: 3e-5 + one
    bf16 ulp; ``correct`` and the [C, ld) columns exactly."""
    L.check_exact("correct", correct, ref.correct)
    L.check_exact("dlogits columns [C, ld)", _d(dl)[:, C:], ref.dlogits_ld[:, C:])
    want = ref.dlogits_ld / ref.scale
    r = [check_bound("loss", loss, ref.loss, TOL_LOSS + F32_TERMS * ref.mag_loss),
         check_bound("dlogits / scale", _d(dl) / ref.scale, want, TOL_PROB + BF16_ULP * want.abs())]
    return _note(family, max(r))


# =========================================================================== guarded outputs
SENT = -6144.0  # exact in bf16 and f32; never a result of these tests


class Guarded:
    """A contiguous tensor of ``shape`` inside a larger flat buffer.  The body starts as ``fill``
    (NaN: every element must be written; a tensor: the values an accumulating kernel adds to),
    the guard rows before and after it as SENT and must come back untouched."""

    def __init__(self, shape, dtype, device="cpu", fill=float("nan"), guard=None):
        n = int(math.prod(shape))
        row = int(shape[-1]) if len(shape) else 1
        self.guard = guard if guard is not None else (max(64, row) + 63) // 64 * 64  # keeps 128-B alignment
        self.buf = torch.full((2 * self.guard + n,), SENT, dtype=dtype, device=device)
        self.t = self.buf[self.guard:self.guard + n].view(*shape)
        if torch.is_tensor(fill):
            self.t.copy_(fill.to(dtype))
        else:
            self.t.fill_(fill)

    def check_guards(self, name):
        b = self.buf.detach().cpu()
        for part, g in (("before", b[:self.guard]), ("after", b[b.numel() - self.guard:])):
            L.check_exact("%s: guard %s the output" % (name, part), g, torch.full_like(g, SENT))
        return self.t


# =========================================================================== input sets
def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- LayerNorm
LN_MEANS = (0.0, 0.5, -3.0, 30.0, -30.0, 7.0)
LN_SPREADS = (1.0, 0.01, 2.0, 0.25, 0.5)


def ln_rows(T):
    """(row means, row spreads): every pair of LN_MEANS x LN_SPREADS within 30 rows; a spread is
    raised to |mean| / 128 (one bf16 ulp of the mean at least), below which a bf16 row would be
    constant -- ill-conditioned at eps = 1e-12 for any f32 implementation."""
    r = torch.arange(T)
    mu = torch.tensor(LN_MEANS, dtype=torch.float64)[r % len(LN_MEANS)]
    sp = torch.tensor(LN_SPREADS, dtype=torch.float64)[r % len(LN_SPREADS)]
    return mu, torch.maximum(sp, mu.abs() / 128)


@functools.lru_cache(maxsize=None)
def ln_case(T, H):
    """bf16 x [T, H] with the row offsets and spreads of ln_rows (columns 0 / 1 of a row hold
    mean +- spread: no row is constant), dy, dres bf16; f32 gamma ~ 1, beta ~ 0; non-zero
    initial values for the three accumulators."""
    sd = 6000 + 13 * H + T % 1013
    mu, sp = ln_rows(T)
    x = L.randn(T, H, seed=sd).double() * sp[:, None] + mu[:, None]
    x[:, 0], x[:, 1] = mu + sp, mu - sp
    x = x.to(BF)
    assert bool((x.double().var(1, unbiased=False) > 0).all())
    return types.SimpleNamespace(
        T=T, H=H, x=x, dy=L.randn(T, H, seed=sd + 1).to(BF), dres=L.randn(T, H, seed=sd + 2).to(BF),
        gamma=L.randn(H, seed=sd + 3) * 0.1 + 1, beta=L.randn(H, seed=sd + 4) * 0.1,
        dgamma0=L.uniform(H, seed=sd + 5, scale=3.0), dbeta0=L.uniform(H, seed=sd + 6, scale=3.0),
        dxsum0=L.uniform(H, seed=sd + 7, scale=3.0))


@functools.lru_cache(maxsize=None)
def ln_fwd_ref(T, H):
    c = ln_case(T, H)
    return layernorm_fwd(c.x, c.gamma, c.beta)


def ln_stats(T, H):
    """The reference's mean / rstd rounded to f32: the backward kernels' inputs."""
    ref = ln_fwd_ref(T, H)
    return ref.mean.float(), ref.rstd.float()


@functools.lru_cache(maxsize=None)
def ln_bwd_ref(T, H, with_dres, with_dxsum):
    c = ln_case(T, H)
    mean, rstd = ln_stats(T, H)
    return layernorm_bwd(c.dy, c.x, mean, rstd, c.gamma, c.dres if with_dres else None,
                         c.dgamma0, c.dbeta0, c.dxsum0 if with_dxsum else None)


LN_H = (8, 504, 512, 520, 768, 1024, 1032, 1536, 1544, 2048)
LN_FWD_T = (1, 15, 16, 17)
LN_BWD_T = (1, 8, 9, 17, 33)
LN_BWD_LARGE = ((8195, 8), (8195, 520), (8195, 768))

# ---- embeddings
EMB_H = (8, 768, 776, 1032, 2048)
EMB_BS = ((1, 1), (7, 5), (8, 3), (9, 4), (33, 3))
EMB_V = 50
EMB_EXTRA_POS = 3  # rows of the position table past seq_len
EMB_IDS = ("random", "equal", "ends")
EMB_TT = ("given", "zeros", "ones", None)


def embed_shapes():
    """Every (B, S) x H."""
    return [(B, S, H) for H in EMB_H for B, S in EMB_BS]


def embed_kinds():
    """Every id kind x token-type kind."""
    return [(i, t) for i in EMB_IDS for t in EMB_TT]


def _grid10(*shape, seed, scale):
    """bf16 values that are multiples of 2^-10 in +-scale: sums of three are exact in f32."""
    v = torch.round(L.uniform(*shape, seed=seed, scale=scale).double() * 1024) / 1024
    out = v.to(BF)
    assert bool(((out.double() * 1024) % 1 == 0).all())
    return out


@functools.lru_cache(maxsize=4)
def embed_case(B, S, H, ids_kind="random", tt_kind="given"):
    """ids int32 [B S] (random with 0 and V - 1 present where T >= 2; all equal; alternating 0 /
    V - 1), token types (random 0 / 1, all 0, all 1, None), bf16 tables whose entries are
    multiples of 2^-10 (word, pos) or small offsets (type), so that word + pos + type is exact in
    f32 and its bf16 rounding is the single rounding of the exact sum; a position table
    EMB_EXTRA_POS rows longer than seq_len; dx bf16; non-zero initial gradients."""
    T, V = B * S, EMB_V
    sd = 7000 + 31 * H + 7 * B + S
    g = _gen(sd)
    if ids_kind == "random":
        ids = torch.randint(0, V, (T,), generator=g)
        if T >= 2:
            ids[0], ids[T - 1] = V - 1, 0
    elif ids_kind == "equal":
        ids = torch.full((T,), 7)
    else:
        ids = torch.where(torch.arange(T) % 2 == 0, 0, V - 1)
    tt = {"given": torch.randint(0, 2, (T,), generator=g), "zeros": torch.zeros(T, dtype=torch.long),
          "ones": torch.ones(T, dtype=torch.long), None: None}[tt_kind]
    if tt_kind == "given" and T >= 2:
        tt[0], tt[1] = 0, 1
    P = S + EMB_EXTRA_POS
    return types.SimpleNamespace(
        B=B, S=S, H=H, T=T, V=V, P=P, ids=ids.int(), tt=None if tt is None else tt.int(),
        word=_grid10(V, H, seed=sd + 1, scale=2.0), pos=_grid10(P, H, seed=sd + 2, scale=2.0),
        type_=_grid10(2, H, seed=sd + 3, scale=1.0),
        gamma=L.randn(H, seed=sd + 4) * 0.1 + 1, beta=L.randn(H, seed=sd + 5) * 0.1,
        dx=L.randn(T, H, seed=sd + 6).to(BF),
        dword0=L.uniform(V, H, seed=sd + 7, scale=2.0), dpos0=L.uniform(P, H, seed=sd + 8, scale=2.0),
        dtype0=L.uniform(2, H, seed=sd + 9, scale=2.0))


# ---- attention
MASK_KINDS = ("none", "prefix", "first", "holes", "inf", "padded")
MASKED = -10000.0
ATTN_SCALES = (0.125, 0.2)
DENSE_S = (1, 15, 16, 17, 33, 63, 64, 65, 127, 128)
FLASH_S = (1, 15, 63, 64, 65, 129, 192, 193)
FLASH_GRIDS = (1, 7, 9, 13, 16)  # workgroups: identity (<= 8), ragged (% 8 != 0), even
# (B, nh, S) whose flash grid ceil(S / 64) * B * nh is 1, 7, 9, 13 and 16
FLASH_GRID_CASES = ((1, 1, 33), (1, 7, 64), (3, 1, 129), (1, 13, 17), (2, 2, 193))
DENSE_B, DENSE_NH = 3, 2
FLASH_B, FLASH_NH = 3, 2
# S -> (16-key tiles, forward waves with live queries, 64-query halves) the dense cases name
DENSE_REACH = {1: (1, 1, 1), 15: (1, 1, 1), 16: (1, 1, 1), 17: (2, 1, 1), 33: (3, 2, 1),
               63: (4, 2, 1), 64: (4, 2, 1), 65: (5, 3, 2), 127: (8, 4, 2), 128: (8, 4, 2)}
FLASH_REACH = {1: 1, 15: 1, 63: 1, 64: 1, 65: 2, 129: 3, 192: 3, 193: 4}  # S -> 64-key tiles
FLASH_GRID_ROUTES = ("identity", "identity", "ragged", "ragged", "even")
PERSIST_PAIRS = ((2, 2), (3, 4))  # (B, nh): 4 pairs on 3 blocks (uneven) and 12
FWD_VARIANTS = ("rp", "lds", "lds_swz")
# name -> (attn_bwd_set_variant, attn_set_swizzle, attn_bwd_set_pf)
BWD_VARIANTS = {"w8": (0, 0, 0), "w4": (1, 0, 0), "half": (2, 0, 0), "persist": (3, 0, 0),
                "persist3": (4, 0, 0), "half_swz": (2, 1, 0), "half_pf": (2, 0, 1),
                "half_swz_pf": (2, 1, 1)}


def attn_mask(kind, B, S):
    """Additive key mask f32 [B, S] (None for "none"):
    prefix  0 on the first n_b keys, -10000 after (n = S, S - 5, S / 2, ...);
    first   -10000 on the FIRST keys: the whole first 64-key tile and 3 b more at S >= 129,
            about a third of the keys below (nothing at S = 1);
    holes   -10000 on a random ~30 % of the keys, +-1.5 on half of the live ones;
    inf     -inf on a random ~30 % (sequence 0 at S > 64: on its whole first 64-key tile, which
            an online softmax meets with a running maximum of -inf), 0 elsewhere;
    padded  sequence 0 all -10000 (softmax over the bare scores), the others a prefix.
    Every sequence of holes / inf keeps at least one live key."""
    if kind == "none":
        return None
    key = torch.arange(S)[None, :]
    g = _gen(8000 + 17 * S + B + 101 * MASK_KINDS.index(kind))
    prefix_n = torch.tensor([max(1, n) for n in (S, S - 5, S // 2, S - 1, S // 3)] * (B // 5 + 1))[:B]
    if kind == "prefix":
        return torch.where(key < prefix_n[:, None], 0.0, MASKED)
    if kind == "first":
        b = torch.arange(B)
        n0 = 64 + 3 * b if S >= 129 else torch.clamp(max(1, S // 3) + b, max=S - 1)
        return torch.where(key < n0[:, None], MASKED, 0.0)
    if kind == "padded":
        m = torch.where(key < prefix_n[:, None], 0.0, MASKED)
        m[0] = MASKED
        return m
    dead = torch.rand(B, S, generator=g) < 0.3
    if kind == "inf" and S > 64:
        dead[0, :64] = True
    for b in range(B):
        dead[b, S - 1 - (7 * b) % min(S, 5)] = False
    if kind == "inf":
        return torch.where(dead, float("-inf"), 0.0)
    add = torch.where(torch.rand(B, S, generator=g) < 0.5, 0.0, 1.5) * torch.where(
        torch.rand(B, S, generator=g) < 0.5, -1.0, 1.0)
    return torch.where(dead, torch.full((B, S), MASKED), add).float()


@functools.lru_cache(maxsize=None)
def attn_case(B, S, nh, kind, scale):
    """qkv, dout bf16 ~ N(0, 1), the mask, the float64 forward and the backward of its results
    rounded to the kernels' input types (o bf16; lse f32 [B nh, S]), with a non-zero dbias0."""
    sd = 9000 + 7 * S + 3 * B + nh + 11 * MASK_KINDS.index(kind)
    qkv = L.randn(B * S, 3 * nh * HD, seed=sd).to(BF)
    dout = L.randn(B * S, nh * HD, seed=sd + 1).to(BF)
    kmask = attn_mask(kind, B, S)
    fwd = attn_fwd(qkv, B, S, nh, kmask, scale)
    o, lse = fwd.o.to(BF), fwd.lse.float()
    dbias0 = L.uniform(3 * nh * HD, seed=sd + 2, scale=4.0)
    bwd = attn_bwd(qkv, o, dout, lse, B, S, nh, kmask, scale, dbias0)
    return types.SimpleNamespace(B=B, S=S, nh=nh, kind=kind, scale=scale, qkv=qkv, dout=dout,
                                 kmask=kmask, fwd=fwd, o=o, lse=lse, dbias0=dbias0, bwd=bwd)


def lse_ld(S):
    """Row pitch of the lse buffer (the wrappers' rule: 128 up to S = 128, then 64-key tiles)."""
    return max(128, (S + 63) // 64 * 64)


def lse_padded(lse, S, fill=float("nan")):
    """lse [B nh, S] inside a [B nh, lse_ld(S)] buffer whose padding is ``fill``."""
    out = torch.full((lse.shape[0], lse_ld(S)), fill, dtype=torch.float32)
    out[:, :S] = lse
    return out


# ---- mlm_xent
XENT_C = (1, 7, 8, 9, 2047, 2048, 2049, 4100)
XENT_BIG = (2, 32776)  # (N, C): past the register kernel's 32768 columns
XENT_SCALE = 1.0 / 37


def xent_tie_pairs(C):
    """Index pairs (a < b) that put two equal maxima: in one 8-logit chunk (a, a + 1); in
    neighbouring lanes (a, a + 8); in two waves (a, a + 512: 64 threads of 8 logits apart); in
    one thread's chunks, (a, a + 2048) for the register kernel, (a, a + 1024) and, on its next
    loop trip, (a, a + 4096) for the two-pass kernel; in the body and in the C % 8 / C % 4 tail
    (3, C - 1)."""
    pairs = []
    for a, step in ((2, 1), (5, 8), (11, 512), (17, 1024), (20, 2048), (1, 4096)):
        if a + step < C - (1 if C % 8 else 0):
            pairs.append((a, a + step))
    if C % 8 and C >= 5:
        pairs.append((3, C - 1))
    if not pairs and C >= 2:
        pairs.append((0, 1))
    return pairs


@functools.lru_cache(maxsize=None)
def xent_case(C, dtype, N=None):
    """Logits in +-5 (as ``dtype``) with one clear maximum per row, except the tie rows: every
    pair of xent_tie_pairs twice, labelled with its first index (correct = 1) and with its
    second (correct = 0: the lowest index is the arg-max).  Then rows labelled arg-max, 0, C - 1,
    -100 and a random class.  A given N keeps the first N of these rows, the widest pair first.
    Returns (logits [N, C], labels int32, ties {row: pair})."""
    pairs = xent_tie_pairs(C)
    if N is not None:
        pairs = sorted(pairs, key=lambda p: p[0] - p[1])
    specs = [("tie", p, w) for p in pairs for w in (0, 1)]
    specs += [("argmax",), ("label", 0), ("label", C - 1), ("ignore",), ("random",)]
    N = len(specs) if N is None else N
    specs = specs[:N]
    assert len(specs) == N
    g = _gen(10000 + C)
    l = (torch.rand(N, C, generator=g) * 10 - 5).to(dtype).float()
    lab = torch.zeros(N, dtype=torch.int32)
    ties = {}
    for r, sp in enumerate(specs):
        top = float(l[r].max()) + 0.5
        am = int(l[r].argmax())
        if sp[0] == "tie":
            (a, b), which = sp[1], sp[2]
            l[r, a] = l[r, b] = top
            ties[r] = (a, b)
            lab[r] = (a, b)[which]
        else:
            l[r, am] = top
            lab[r] = {"argmax": am, "label": sp[1] if len(sp) > 1 else 0, "ignore": -100,
                      "random": int(torch.randint(0, C, (1,), generator=g))}[sp[0]]
    l = l.to(dtype)
    for r in range(N):  # the inputs' own property
        n_max = int((l[r] == l[r].max()).sum())
        if r in ties:
            a, b = ties[r]
            assert n_max == 2 and float(l[r, a]) == float(l[r, b]) == float(l[r].max())
        else:
            assert n_max == 1
    return l, lab, ties


def xent_lds(C):
    """(C rounded up to 8; the same + 4: ld % 8 == 4)."""
    ld8 = (C + 7) // 8 * 8
    return ld8, ld8 + 4


def xent_padded(logits, ld, fill=99.0):
    """[N, C] logits inside [N, ld] rows whose padding would win every arg-max if read."""
    out = torch.full((logits.shape[0], ld), fill, dtype=logits.dtype)
    out[:, :logits.shape[1]] = logits
    return out


# ---- act_grad
ACT_N = (8, 2040, 2048, 2056)


def act_case(n):
    x, dy = L.act_inputs(n)
    return x.to(BF), dy.to(BF)


# =========================================================================== launch arithmetic
@functools.lru_cache(maxsize=None)
def launch_constants():
    """The constants the reach conditions depend on, read from the .hip sources."""
    tr, fl, cm = L._src("transformer.hip"), L._src("flash_attn.hip"), L._src("common.h")
    F = L._find
    k = types.SimpleNamespace()
    m = F(tr, r"constexpr int SP = (\d+), D = (\d+);", "attention SP / D")
    k.sp, k.d = int(m.group(1)), int(m.group(2))
    assert k.d == HD
    k.half = int(F(tr, r"constexpr int HQ = (\d+);", "queries per half").group(1))
    k.fwd_rows_per_wave = int(F(tr, r"const int row = (\d+) \* wave \+ 16 \* i \+ cl;",
                                "forward rows per wave").group(1))
    k.key_tile = int(F(tr, r"constexpr int NT = NW \* 64, RPW = SP / NW, NI = RPW / (\d+);",
                       "backward rows per wave").group(1))
    k.persist_test_blocks = int(F(tr, r"nb = var == 4 \? (\d+) : blocks;", "3-block grid").group(1))
    k.persist_blocks = int(F(tr, r'getenv\("DTFX_ATTN_BWD_BLOCKS"\);\s*return e && std::atoi\(e\) > 0 \? '
                                 r"std::atoi\(e\) : (\d+);", "persistent grid").group(1))
    # LayerNorm forward
    m = F(tr, r"void layernorm_fwd_launch\(.*?const int nc = \(H \+ (\d+)\) / (\d+);", "ln fwd nc")
    assert int(m.group(1)) + 1 == int(m.group(2))
    k.lnf_cols = int(m.group(2))
    k.lnf_rows = int(F(tr, r'getenv\("DTFX_LN_FWD_ROWS"\);\s*return e \? atoi\(e\) : (\d+);',
                       "ln fwd rows per wave").group(1))
    k.lnf_waves = int(F(tr, r"const int per_block = (\d+) \* rows;", "ln fwd waves").group(1))
    k.lnf_align = int(F(tr, r"!\(\(\(uintptr_t\)gamma \| \(uintptr_t\)beta\) & (\d+)\)",
                        "ln fwd alignment route").group(1)) + 1
    F(tr, r"hipLaunchKernelGGL\(layernorm_fwd_kernel, dim3\(\(T \+ 3\) / 4\), dim3\(256\)", "one-row grid")
    # LayerNorm backward
    m = F(tr, r"const int rpb7 = rpb_env > 0 \? rpb_env : \(T >= (\d+) \? (\d+) : (\d+)\);", "h768 rpb")
    k.ln_switch, k.h768_rpb_big, k.h768_rpb = (int(m.group(i)) for i in (1, 2, 3))
    m = F(tr, r"const int rpb = rpb_env > 0 \? rpb_env : \(T >= (\d+) \? (\d+) : (\d+)\);", "ln bwd rpb")
    assert int(m.group(1)) == k.ln_switch
    k.lnb_rpb_big, k.lnb_rpb = int(m.group(2)), int(m.group(3))
    F(tr, r"const int nc = \(H / 8 \+ 63\) / 64;", "ln bwd nc")
    m = F(tr, r"constexpr int NWV = NC <= 2 \? (\d+) : (\d+);", "ln bwd waves")
    k.lnb_waves_small, k.lnb_waves_big = int(m.group(1)), int(m.group(2))
    k.lnb_slots = int(F(tr, r'getenv\("DTFX_LN_SLOTS"\);\s*return e \? std::max\(1, std::min\(3, '
                            r"atoi\(e\)\)\) : (\d+);", "ln bwd slots").group(1))
    F(tr, r"if \(H == 768 && \(g_ln_h768 >= 0 \? g_ln_h768 : h768_env\) == 1 && "
          r"!\(\(\(uintptr_t\)gamma\) & 15\)\)", "h768 route")
    F(tr, r"if \(nc == 1 && slots >= 3\) DTFX_LNB\(1, 3\);\s*else if \(nc == 2 && slots >= 3\) "
          r"DTFX_LNB\(2, 3\);", "3-slot route")
    # embeddings
    k.word_cols = 64 * int(F(tr, r"constexpr int U = (\d+);  // loads in flight per lane.*?"
                                 r"c0 \+= 64 \* U\)", "word gradient pass").group(1))
    k.pos_chunks = int(F(tr, r"for \(int ch = t; ch < nch; ch \+= (\d+)\)", "pos/type chunks").group(1))
    k.pos_batch = int(F(tr, r"for \(int b0 = stream; b0 < Bn; b0 \+= (\d+)\)", "pos/type batch rows").group(1))
    F(tr, r"hipLaunchKernelGGL\(embed_word_bwd_kernel, dim3\(\(T \+ 3\) / 4\), dim3\(256\)", "word grid")
    F(tr, r"hipLaunchKernelGGL\(embed_ln_fwd_kernel, dim3\(\(T \+ 3\) / 4\), dim3\(256\)", "embed grid")
    # mlm_xent
    k.xent_chunks = int(F(tr, r"constexpr int kXentChunks = (\d+);", "kXentChunks").group(1))
    F(tr, r"logits_bf16 && regs && ldl % 8 == 0 && ldd % 8 == 0 && ldd <= 256 \* 8 \* kXentChunks &&\s*"
          r"!\(\(\(uintptr_t\)logits \| \(uintptr_t\)dl\) & 15\)", "register-kernel route")
    k.xent_pass = 256 * 4 * int(F(tr, r"constexpr int U = (\d+);\s*for \(int i0 = t; i0 < C4; "
                                      r"i0 \+= 256 \* U\)", "two-pass kernel trip").group(1))
    k.xent_reg_pass = 256 * 8
    # act_grad
    k.act_cap = int(F(tr, r"void act_grad_bf16_launch\(.*?long long blocks = \(n / 8 \+ 255\) / 256;\s*"
                          r"if \(blocks > (\d+)\) blocks = \1;", "act_grad block cap").group(1))
    # flash
    k.flash_tile = int(F(fl, r"constexpr int D = 64, T = (\d+);", "flash tile").group(1))
    F(fl, r"dim3\(\(S \+ T - 1\) / T, Bn \* nh\)", "flash grid")
    k.xcd = int(F(cm, r"int xcd_remap\(int orig, int nwg\) \{\s*constexpr int kXcd = (\d+);\s*"
                      r"if \(nwg <= kXcd\) return orig;\s*const int q = nwg / kXcd, r = nwg % kXcd;\s*"
                      r"const int xcd = orig % kXcd, pos = orig / kXcd;\s*return \(xcd < r \? xcd \* "
                      r"\(q \+ 1\) : r \* \(q \+ 1\) \+ \(xcd - r\) \* q\) \+ pos;", "xcd_remap").group(1))
    return k


def attn_plan(S):
    """Dense attention at S: 16-key tiles, forward waves with live queries (32 rows each),
    backward waves with live rows (4- and 8-wave kernels), 64-query halves, ragged tails."""
    k = launch_constants()
    up = lambda a, b: (a + b - 1) // b
    return types.SimpleNamespace(
        key_tiles=up(S, k.key_tile), ragged_tile=S % k.key_tile != 0,
        fwd_waves=up(S, k.fwd_rows_per_wave), bwd_waves4=up(S, k.sp // 4), bwd_waves8=up(S, k.sp // 8),
        halves=up(S, k.half), ragged_half=S % k.half != 0)


def persist_plan(pairs, variant):
    """(blocks, pairs of the busiest block, pairs of the idlest) of the persistent backward."""
    k = launch_constants()
    nb = min(pairs, k.persist_test_blocks if variant == "persist3" else k.persist_blocks)
    per = [len(range(b, pairs, nb)) for b in range(nb)]
    return nb, max(per), min(per)


def xcd_remap(orig, nwg):
    k = launch_constants().xcd
    if nwg <= k:
        return orig
    q, r = nwg // k, nwg % k
    xcd, pos = orig % k, orig // k
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + pos


def flash_plan(B, S, nh):
    """Grid of the flash kernels and the route their block-id remap takes."""
    k = launch_constants()
    tiles = (S + k.flash_tile - 1) // k.flash_tile
    nwg = tiles * B * nh
    route = "identity" if nwg <= k.xcd else "even" if nwg % k.xcd == 0 else "ragged"
    return types.SimpleNamespace(tiles=tiles, nwg=nwg, route=route, ragged_tile=S % k.flash_tile != 0)


def ln_fwd_plan(T, H, aligned):
    """Kernel ("rows": R rows per wave, f32x4 gamma / beta; "one_row": layernorm_fwd_kernel),
    column chunks per lane, blocks and whether the last block / wave is ragged."""
    k = launch_constants()
    nc = (H + k.lnf_cols - 1) // k.lnf_cols
    if aligned and k.lnf_rows in (2, 4):
        per = k.lnf_waves * k.lnf_rows
        return types.SimpleNamespace(kernel="rows", nc=nc, blocks=(T + per - 1) // per,
                                     ragged=T % k.lnf_rows != 0 or T % per != 0, full_chunks=H % k.lnf_cols == 0)
    return types.SimpleNamespace(kernel="one_row", nc=nc, blocks=(T + 3) // 4, ragged=T % 4 != 0,
                                 full_chunks=H % k.lnf_cols == 0)


def ln_bwd_plan(T, H, slots=None, h768=0, gamma_aligned=True):
    """Kernel, column chunks, row slots, waves, rows per block (the 8192 switch), blocks, rows of
    the last block, and whether a wave's rows exceed its slots (the refill load runs)."""
    k = launch_constants()
    slots = k.lnb_slots if slots is None else max(1, min(3, slots))
    if H == 768 and h768 == 1 and gamma_aligned:
        kernel, nc, ns, waves = "h768", 3, 1, 8
        rpb = k.h768_rpb_big if T >= k.ln_switch else k.h768_rpb
    else:
        nc = (H // 8 + 63) // 64
        ns = 3 if nc <= 2 and slots >= 3 else 2
        kernel, waves = "generic", (k.lnb_waves_small if nc <= 2 else k.lnb_waves_big)
        rpb = k.lnb_rpb_big if T >= k.ln_switch else k.lnb_rpb
    blocks = (T + rpb - 1) // rpb
    last = T - (blocks - 1) * rpb
    rows_per_wave = (min(rpb, T) + waves - 1) // waves
    return types.SimpleNamespace(kernel=kernel, nc=nc, ns=ns, waves=waves, rpb=rpb, blocks=blocks,
                                 last_rows=last, ragged_last=last != rpb, refills=rows_per_wave > ns)


def embed_plan(B, S, H):
    """Ragged last block of the 4-rows-per-block kernels, 768-column passes of the word
    gradient, 128-chunk trips and 32-row batch trips of the position / type gradient."""
    k = launch_constants()
    return types.SimpleNamespace(
        ragged_rows=(B * S) % 4 != 0, word_passes=(H + k.word_cols - 1) // k.word_cols,
        chunk_trips=(H // 8 + k.pos_chunks - 1) // k.pos_chunks,
        batch_trips=(B + k.pos_batch - 1) // k.pos_batch)


def xent_plan(C, ld, bf16, regs, aligned=True):
    """Kernel ("regs" / "two_pass"), chunks of 2048 logits a register-kernel thread holds, trips
    of the two-pass kernel's 4096-logit loop, and the tails (C % 8, C % 4)."""
    k = launch_constants()
    use_regs = bool(bf16 and regs == 1 and ld % 8 == 0 and ld <= k.xent_reg_pass * k.xent_chunks and aligned)
    return types.SimpleNamespace(
        kernel="regs" if use_regs else "two_pass", reg_chunks=(C // 8 + 255) // 256,
        trips=((C // 4) + k.xent_pass // 4 - 1) // (k.xent_pass // 4), tail8=C % 8, tail4=C % 4)


def act_grad_blocks(n):
    """(blocks, grid-stride passes) of act_grad at n elements."""
    k = launch_constants()
    n8 = n // 8
    b = min((n8 + 255) // 256, k.act_cap)
    return b, (n8 + b * 256 - 1) // (b * 256)


def act_grad_wrap_size():
    """The first n past the block cap: its last 8-element group is a second pass."""
    return launch_constants().act_cap * 256 * 8 + 8
