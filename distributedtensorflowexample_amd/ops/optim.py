"""Flat multi-tensor optimizer kernels (one launch per optimizer step).

Parameters of a model live in ONE flat f32 buffer (``models.flat``), so the
SGD of ``GradientDescentOptimizer`` (worker.py:71, ``ApplyGradientDescent`` x4
on the ps, worker.py:79) is a single dwordx4 kernel over 79,510 elements.
"""
from __future__ import annotations

import torch

from ._ext import check_gpu_f32, hip, ptr, stream_handle


def sgd_(p, g, lr, weight_decay=0.0, lr_tensor=None):
    if not p.is_cuda:
        with torch.no_grad():
            if weight_decay:
                p.add_(p, alpha=-float(lr) * weight_decay)
            p.add_(g, alpha=-float(lr if lr_tensor is None else lr_tensor.item()))
        return p
    check_gpu_f32(p, g, lr_tensor)
    hip().sgd(p.numel(), ptr(p), ptr(g), float(lr), ptr(lr_tensor), float(weight_decay),
              stream_handle())
    return p


def momentum_(p, g, buf, lr, momentum=0.9, weight_decay=0.0, nesterov=False, lr_tensor=None):
    if not p.is_cuda:
        with torch.no_grad():
            l = float(lr if lr_tensor is None else lr_tensor.item())
            gg = g + weight_decay * p
            buf.mul_(momentum).add_(gg)
            p.add_(gg + momentum * buf if nesterov else buf, alpha=-l)
        return p
    check_gpu_f32(p, g, buf, lr_tensor)
    hip().momentum(p.numel(), ptr(p), ptr(g), ptr(buf), float(lr), ptr(lr_tensor),
                   float(momentum), float(weight_decay), bool(nesterov), stream_handle())
    return p


def adam_(p, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
          adamw=True, lr_tensor=None, step_tensor=None):
    """Bias-corrected Adam/AdamW.  ``step`` is 1-based (after increment)."""
    if not p.is_cuda:
        with torch.no_grad():
            l = float(lr if lr_tensor is None else lr_tensor.item())
            t = int(step if step_tensor is None else step_tensor.item())
            gg = g if adamw else g + weight_decay * p
            m.mul_(beta1).add_(gg, alpha=1 - beta1)
            v.mul_(beta2).addcmul_(gg, gg, value=1 - beta2)
            bc1 = 1 - beta1 ** t
            bc2 = 1 - beta2 ** t
            denom = v.sqrt() / (bc2 ** 0.5) + eps
            if adamw:
                p.mul_(1 - l * weight_decay)
            p.addcdiv_(m, denom, value=-l / bc1)
        return p
    check_gpu_f32(p, g, m, v, lr_tensor)
    if step_tensor is not None and step_tensor.dtype != torch.int32:
        raise TypeError("step_tensor must be int32")
    hip().adam(p.numel(), ptr(p), ptr(g), ptr(m), ptr(v), float(lr), ptr(lr_tensor),
               float(beta1), float(beta2), float(eps), float(weight_decay), bool(adamw),
               int(step), ptr(step_tensor), stream_handle())
    return p


def _layerwise_args(name, p, segments, partials, *planes, lr_tensor=None):
    """The GPU checks both layer-wise functions share -> (segment table, partials)."""
    from . import layerwise

    seg = layerwise.check_segments(segments, p.numel())
    check_gpu_f32(p, *planes, lr_tensor)
    for t in (p,) + planes:
        if t.numel() != p.numel():
            raise ValueError("%s: every plane must have p's %d elements" % (name, p.numel()))
        if t.data_ptr() % 16:
            raise ValueError("%s: buffers must be 16-byte aligned" % name)
    nb = layerwise.num_blocks(seg)
    if partials is None:  # (a caller that captures a graph or steps in a loop brings its own)
        partials = torch.empty(2 * nb, device=p.device, dtype=torch.float32)
    check_gpu_f32(partials)
    if partials.numel() < 2 * nb or partials.data_ptr() % 8:
        raise ValueError("%s: partials must hold 2 floats for each of the %d workgroups, 8-byte "
                         "aligned (got %d floats)" % (name, nb, partials.numel()))
    return seg, partials


def _segment_ratio(num, den, scale=1.0):
    """``scale * num / den`` where both are > 0, else 1 (the trust-ratio fallback), in f32."""
    return scale * num / den if (float(num) > 0.0 and float(den) > 0.0) else num.new_tensor(1.0)


def lars_(p, g, buf, lr, segments, momentum=0.9, eta=0.001, weight_decay=0.0, lr_tensor=None,
          partials=None):
    """LARS (``ops/layerwise.py``): per segment ``r = eta |p| / (|g| + wd |p|)``, then
    ``momentum_``'s arithmetic on ``g' = r (g + wd p)``.  ``segments``: the boundaries
    ``(0, ..., n)``, at most 8 segments, each start a multiple of 4.  GPU: two launches;
    ``partials`` (f32, ``2 * layerwise.num_blocks(segments)``) is scratch for the norms."""
    if not p.is_cuda:
        from . import layerwise

        seg = layerwise.check_segments(segments, p.numel())
        with torch.no_grad():
            l = float(lr if lr_tensor is None else lr_tensor.item())
            for a, b in zip(seg, seg[1:]):
                pn, gn = p[a:b].norm(), g[a:b].norm()
                r = _segment_ratio(pn, gn + weight_decay * pn, float(eta))
                buf[a:b].mul_(momentum).add_(r * (g[a:b] + weight_decay * p[a:b]))
                p[a:b].add_(buf[a:b], alpha=-l)
        return p
    seg, partials = _layerwise_args("lars_", p, segments, partials, g, buf, lr_tensor=lr_tensor)
    hip().lars(seg, ptr(p), ptr(g), ptr(buf), ptr(partials), float(lr), ptr(lr_tensor),
               float(momentum), float(eta), float(weight_decay), stream_handle())
    return p


def lamb_(p, g, m, v, lr, step, segments, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
          step_tensor=None, lr_tensor=None, partials=None):
    """LAMB (``ops/layerwise.py``): Adam's bias-corrected direction plus ``wd p`` is ``u``; per
    segment ``r = |p| / |u|``; ``p -= lr r u``.  ``step`` is 1-based, as ``adam_``'s; ``segments``
    and ``partials`` as ``lars_``'s."""
    if not p.is_cuda:
        from . import layerwise

        seg = layerwise.check_segments(segments, p.numel())
        with torch.no_grad():
            l = float(lr if lr_tensor is None else lr_tensor.item())
            t = int(step if step_tensor is None else step_tensor.item())
            m.mul_(beta1).add_(g, alpha=1 - beta1)
            v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
            u = (m / (1 - beta1 ** t)) / (v.sqrt() / ((1 - beta2 ** t) ** 0.5) + eps)
            u.add_(p, alpha=weight_decay)
            for a, b in zip(seg, seg[1:]):
                r = _segment_ratio(p[a:b].norm(), u[a:b].norm())
                p[a:b].sub_(u[a:b] * (l * r))
        return p
    seg, partials = _layerwise_args("lamb_", p, segments, partials, g, m, v, lr_tensor=lr_tensor)
    if step_tensor is not None and step_tensor.dtype != torch.int32:
        raise TypeError("step_tensor must be int32")
    hip().lamb(seg, ptr(p), ptr(g), ptr(m), ptr(v), ptr(partials), float(lr), ptr(lr_tensor),
               float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
               ptr(step_tensor), stream_handle())
    return p


def ema_(shadow, p, decay, num_updates=False, step=0, step_tensor=None):
    """Moving average of the parameters (``ops/ema.py``), in place on ``shadow``:
    ``shadow -= (1 - d_t) * (shadow - p)`` with ``d_t = decay`` or, with ``num_updates``,
    ``min(decay, (1 + t) / (10 + t))``.  ``t`` is 1-based (after increment): ``step``, or the
    int32 device counter ``step_tensor`` (graph-capturable, as ``adam_`` reads it).  ``decay``
    may be an ``ops.ema.EMA`` (``num_updates`` is then its own): a caller that applies it every
    step validates once and passes the object."""
    from . import ema as ema_mod

    e = decay if isinstance(decay, ema_mod.EMA) else ema_mod.EMA(decay, num_updates)
    if shadow.numel() != p.numel():
        raise ValueError("ema_: shadow and p must have the same number of elements")
    if not shadow.is_cuda:
        with torch.no_grad():
            t = int(step if step_tensor is None else step_tensor.item())
            shadow.sub_(shadow - p, alpha=float(e.one_minus_decay_f32(t)))
        return shadow
    check_gpu_f32(shadow, p)
    if step_tensor is not None and step_tensor.dtype != torch.int32:
        raise TypeError("step_tensor must be int32")
    omd, nu = e.words()
    hip().ema(shadow.numel(), ptr(shadow), ptr(p), omd, bool(nu), int(step), ptr(step_tensor),
              stream_handle())
    return shadow


def clip_by_global_norm_(g, clip_norm, partials, pre=1.0, gnorm=None, have_partials=False):
    """Clipping by the global norm (``ops/clip.py``), in place on the flat gradient ``g``, fused
    with the averaging ``scale_`` does: ``g *= pre * clip_norm / max(norm, clip_norm)``, ``norm =
    pre * |g|`` (so ``norm <= clip_norm`` and ``pre == 1`` leave ``g``'s bits alone).  ``gnorm``
    (optional, one f32) receives ``norm``.  GPU: ``partials`` is scratch of
    ``clip.num_partials(g.numel())`` floats (``None`` allocates it; a caller that captures a graph
    brings its own), filled by one launch and re-added by the scale launch;
    ``have_partials=True`` skips the first launch -- the large-batch reduce launch already left the
    sums of squares of this very gradient there (``mlp_large_batch.step_grad(partials=...)``)."""
    from . import clip as clip_mod

    c = clip_mod.resolve(clip_norm)
    if c is None:
        raise ValueError("clip_by_global_norm_: clip_norm must be > 0 (0 is no clipping: do not "
                         "call)")
    pre = float(pre)
    if not (pre > 0.0 and pre < float("inf")):
        raise ValueError("clip_by_global_norm_: pre must be finite and > 0, got %r" % (pre,))
    if not g.is_cuda:
        with torch.no_grad():
            norm = g.norm() * pre
            if gnorm is not None:
                gnorm.fill_(float(norm))
            g.mul_(pre * c / max(float(norm), c))
        return g
    check_gpu_f32(g, gnorm)
    n, nb = g.numel(), clip_mod.num_partials(g.numel())
    if g.data_ptr() % 16:
        raise ValueError("clip_by_global_norm_: the gradient must be 16-byte aligned")
    if partials is None:
        if have_partials:
            raise ValueError("clip_by_global_norm_: have_partials needs the partials")
        partials = torch.empty(nb, device=g.device, dtype=torch.float32)
    check_gpu_f32(partials)
    if partials.numel() < nb:
        raise ValueError("clip_by_global_norm_: partials must hold one float for each of the %d "
                         "workgroups (got %d)" % (nb, partials.numel()))
    if gnorm is not None and gnorm.numel() < 1:
        raise ValueError("clip_by_global_norm_: gnorm must hold one float")
    h, s = hip(), stream_handle()
    if not have_partials:
        h.gnorm_partials(n, ptr(g), ptr(partials), s)
    h.clip_scale(n, ptr(g), ptr(partials), nb, c, pre, ptr(gnorm), s)
    return g


def scale_(x, a):
    if not x.is_cuda:
        x.mul_(a)
        return x
    check_gpu_f32(x)
    hip().scale(x.numel(), ptr(x), float(a), stream_handle())
    return x


def counter_add_(c, d=1):
    """In-place device add on an int32 scalar counter (capture-safe)."""
    if not c.is_cuda:
        c.add_(d)
        return c
    if c.dtype != torch.int32:
        raise TypeError("counter must be int32")
    hip().counter_add(ptr(c), int(d), stream_handle())
    return c
