"""float64 references for the parameter-update kernels, independent of the project's formulas.

The update rules come from ``torch.optim`` (SGD, Adam, AdamW) run on float64 CPU tensors with
the optimizer state injected, so a run can start from non-zero moments and any step number.
Hyper-parameters are rounded to float32 first and widened again: that is what a kernel receives.
"""
import numpy as np
import torch

ULP = 2.0 ** -23  # float32 spacing at 1

# float32 patterns at the bf16 rounding edges: ties to even (down, up), just below / above a
# tie, a negative tie, the largest finite value (rounds to inf), -0, and denormals; and the bf16
# words round-to-nearest-even makes of them
EDGE_BITS = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0x7F7FFFFF, 0x80000000,
             0x00000001, 0x00008000, 0x00018000]
EDGE_BF16 = [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0xBF80, 0x7F80, 0x8000, 0x0000, 0x0000, 0x0002]


def f32(x):
    """A Python float holding ``x`` rounded to float32."""
    return float(np.float32(x))


def _param(p, g):
    q = p.detach().double().clone().requires_grad_(True)
    q.grad = g.detach().double().clone()
    return q


def sgd_step(p, g, lr, wd=0.0, mu=0.0, nesterov=False, buf=None):
    """One torch.optim.SGD step; returns (p, momentum buffer or None), both float64."""
    q = _param(p, g)
    opt = torch.optim.SGD([q], lr=f32(lr), momentum=f32(mu), dampening=0.0,
                          weight_decay=f32(wd), nesterov=bool(nesterov), foreach=False)
    if buf is not None:
        opt.state[q]["momentum_buffer"] = buf.detach().double().clone()
    opt.step()
    return q.detach(), opt.state[q].get("momentum_buffer")


def adam_step(p, g, m, v, lr, step, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, adamw=True):
    """One torch.optim.Adam / AdamW step number ``step`` (1-based); returns float64 (p, m, v)."""
    q = _param(p, g)
    cls = torch.optim.AdamW if adamw else torch.optim.Adam
    opt = cls([q], lr=f32(lr), betas=(f32(b1), f32(b2)), eps=f32(eps), weight_decay=f32(wd),
              amsgrad=False, foreach=False)
    st = opt.state[q]
    st["step"] = torch.tensor(float(step - 1))
    st["exp_avg"] = m.detach().double().clone()
    st["exp_avg_sq"] = v.detach().double().clone()
    opt.step()
    assert int(st["step"].item()) == step
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]


def adam_mixed_step(p, g, m, v, lr, step, b1=0.9, b2=0.999, eps=1e-6, wd=0.01, gscale=1.0):
    """transformer.adam_mixed: AdamW on the scaled gradient."""
    return adam_step(p, g.double() * f32(gscale), m, v, lr, step, b1, b2, eps, wd, adamw=True)


def sgd_momentum_mixed_step(p, g, v, lr, mu=0.9, wd=0.0, gscale=1.0):
    """cnn.sgd_momentum_mixed: L2-decayed momentum SGD on the scaled gradient."""
    return sgd_step(p, g.double() * f32(gscale), lr, wd=wd, mu=mu, nesterov=False, buf=v)


def bound(steps, ref):
    """|kernel - ref| allowed after ``steps`` steps: per step the value is rounded at most twice,
    by half a float32 ulp each (the update itself is a few lr, computed to ~1e-6 relative)."""
    return 2.0 * steps * ULP * max(1.0, float(ref.abs().max()))


def make_case(n, seed, moments=True):
    """Inputs for an update kernel: float32 CPU tensors p, g, m0, v0 and ``regions``, a list of
    (name, index tensor).  |p| stays below ~5.  With n >= 8 three blocks sit at the front and
    (n > 4096) again at the very end, so the last grid pass and the scalar tail see them too:
      zero : g = m = v = 0            (the parameter only decays, nothing may become NaN)
      tiny : g = +-1e-20, m = v = 0   (g * g underflows in float32)
      big  : g = +-1e4
    The big block is its own region: its values are ~1e4 times the others' and every bound is
    taken from the region's own max-abs."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    if moments:
        m = 0.1 * torch.randn(n, generator=gen)
        v = 0.01 + 0.1 * torch.rand(n, generator=gen)  # |m| / sqrt(v) stays O(1)
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    blk = min(64, n // 8)
    big = torch.zeros(n, dtype=torch.bool)
    if blk:
        sign = torch.ones(blk)
        sign[1::2] = -1
        starts = [0] + ([n - 3 * blk] if n > 4096 else [])
        for s in starts:
            g[s:s + blk] = 0
            g[s + blk:s + 2 * blk] = 1e-20 * sign
            m[s:s + 2 * blk] = 0
            v[s:s + 2 * blk] = 0
            g[s + 2 * blk:s + 3 * blk] = 1e4 * sign
            big[s + 2 * blk:s + 3 * blk] = True
    regions = [("rest", (~big).nonzero().flatten())]
    if blk:
        regions.append(("big", big.nonzero().flatten()))
    return p, g, m, v, regions


def assert_close(name, out, ref, steps, regions):
    """``out`` (float32, any device) against ``ref`` (float64) at ``bound`` per region."""
    out = out.detach().cpu()
    assert out.dtype == torch.float32
    assert bool(torch.isfinite(out).all()), "%s: non-finite values" % name
    for rname, idx in regions:
        r = ref[idx]
        err = float((out[idx].double() - r).abs().max())
        tol = bound(steps, r)
        assert err <= tol, "%s[%s]: max error %.3e > %.3e" % (name, rname, err, tol)
