"""Layer-wise adaptive rates of the fused MLP trainer (``--optimizer lars | lamb``): the definition.

At a batch of 4,096 rows or more one global rate either diverges in the tensor with the largest
gradient-to-weight ratio or starves the others; LARS (You et al. 2017, on momentum SGD) and LAMB
(You et al. 2019, on Adam) scale every tensor's step by a *trust ratio* of norms.

The flat buffer is cut into *segments*, one per tensor, given as boundaries ``(0, ..., n)``; the
MLP's are ``mlp_segments()`` (W1t, b1, W2t, b2).  ``|x|`` is the Euclidean norm over one segment,
``wd`` = ``--weight_decay``, ``lr`` the rate of the step (a constant or the scheduled rate).

* lars (``mu`` = ``--momentum``, ``eta`` = ``--lars_eta``): per segment ``r = eta |p| / (|g| + wd
  |p|)`` when ``|p| > 0`` and the denominator is > 0, else ``r = 1``; per element ``g' = r (g + wd
  p); accum = mu accum + g'; p -= lr accum`` -- ``momentum_``'s arithmetic on ``g'``.  No Nesterov.
* lamb (``b1, b2, eps`` = the ``--adam_*`` flags, ``t`` the 1-based step): ``m = b1 m + (1 - b1) g;
  v = b2 v + (1 - b2) g^2; u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + wd p``; per segment
  ``r = |p| / |u|`` when both norms are > 0, else ``r = 1``; ``p -= lr r u``.  The decay is inside
  ``u`` by definition, so ``--adamw`` has no meaning and an explicit ``--noadamw`` is refused.

Biases are segments like any other (they start at zero and take ``r = 1`` until they move); there
is no exclusion list and no clipping function other than the identity.  Slots: lars one plane
(``Momentum``), lamb two (``m``, ``v``) -- ``parallel/gpu_ps_optim.SLOT_NAMES``.

On the device each rule is two launches over a segment-aligned grid (``csrc/kernels/optim.hip``):
a workgroup owns ``BLOCK`` = 1,024 consecutive elements of one segment, so a table has at most
``MAX_SEGMENTS`` = 8 segments, each starting at a multiple of 4 elements (only the buffer's end
may be ragged), and the caller owns ``2 * num_blocks(segments)`` floats of partial sums.

ResNet-50 (``--model resnet50 --optimizer lars``) takes the same lars rule with an exclusion list
-- ``lars_mixed_update`` below is its definition -- through kernels of its own
(``csrc/kernels/lars_mixed.hip``, ``ops.cnn.lars_momentum_mixed``): any number of tensors, the
bf16 working copy and the split-K gradient planes of its flat buffer.
"""
from __future__ import annotations

import math

KINDS = ("lars", "lamb")
MAX_SEGMENTS = 8
BLOCK = 1024
DEFAULT_ETA = 0.001


def is_layerwise(kind):
    return str(kind) in KINDS


def check_eta(eta):
    """``lars_eta`` as a finite float > 0, else ValueError."""
    try:
        e = float(eta)
    except (TypeError, ValueError):
        raise ValueError("lars_eta must be a number, got %r" % (eta,))
    if not math.isfinite(e) or e <= 0.0:
        raise ValueError("lars_eta must be finite and > 0, got %r" % (eta,))
    return e


def check_segments(segments, n=None):
    """The boundaries ``(0, ..., n)`` as a tuple of ints the kernels take, else ValueError."""
    seg = tuple(int(s) for s in segments)
    if not 2 <= len(seg) <= MAX_SEGMENTS + 1:
        raise ValueError("layerwise: a segment table has 1..%d segments, got %d"
                         % (MAX_SEGMENTS, len(seg) - 1))
    if seg[0] != 0 or any(b <= a for a, b in zip(seg, seg[1:])):
        raise ValueError("layerwise: segment boundaries must start at 0 and increase, got %r"
                         % (seg,))
    for a in seg[:-1]:
        if a % 4:
            raise ValueError("layerwise: every segment must start at a multiple of 4 elements, "
                             "got %d" % a)
    if n is not None and seg[-1] != int(n):
        raise ValueError("layerwise: the segments end at %d, the buffer has %d elements"
                         % (seg[-1], int(n)))
    return seg


def num_blocks(segments):
    """Workgroups of the segment-aligned grid = pairs of partial sums the caller provides."""
    seg = check_segments(segments)
    return sum((b - a + BLOCK - 1) // BLOCK for a, b in zip(seg, seg[1:]))


def mlp_segments():
    """The MLP's four tensors in the flat layout, from ``csrc/kernels/mlp_model.h``."""
    from ._ext import hip

    return tuple(int(s) for s in hip().mlp_segments())


class Layerwise:
    """One validated (kind, weight_decay, eta) with the kind's hyper-parameters: the float64
    definition (``update``) and the keyword arguments ``ops.optim.lars_`` / ``lamb_`` take."""

    def __init__(self, kind, weight_decay=0.0, eta=DEFAULT_ETA, momentum=0.9, beta1=0.9,
                 beta2=0.999, epsilon=1e-8, nesterov=False, adamw=True):
        from . import weight_decay as weight_decay_mod

        if kind not in KINDS:
            raise ValueError("layerwise: kind must be one of %s, got %r" % ("|".join(KINDS), kind))
        if nesterov:
            raise ValueError("nesterov needs optimizer momentum, got %r" % (kind,))
        if kind == "lamb" and not adamw:
            raise ValueError("adamw=False has no meaning with optimizer lamb: its weight decay is "
                             "inside the update direction by definition")
        self.kind = kind
        self.wd = weight_decay_mod.check(weight_decay)
        self.eta = check_eta(eta)
        self.momentum, self.beta1, self.beta2 = float(momentum), float(beta1), float(beta2)
        self.epsilon = float(epsilon)

    def __repr__(self):
        return "Layerwise(%r, weight_decay=%r, eta=%r)" % (self.kind, self.wd, self.eta)

    @property
    def kw(self):
        """The hyper-parameter keywords of this kind's ``ops.optim`` function."""
        if self.kind == "lars":
            return dict(momentum=self.momentum, eta=self.eta, weight_decay=self.wd)
        return dict(beta1=self.beta1, beta2=self.beta2, eps=self.epsilon, weight_decay=self.wd)

    def update(self, p, g, slots, lr, t, segments):
        """The definition in float64 -> ``(p_new, [slots_new])`` (new tensors; inputs untouched).
        ``slots``: lars ``[accum]``, lamb ``[m, v]``; ``t``: the 1-based step (lamb only)."""
        import torch

        f64 = torch.float64
        p, g = p.detach().to(f64), g.detach().to(f64)
        slots = [s.detach().to(f64) for s in slots]
        seg = check_segments(segments, p.numel())
        lr, wd = float(lr), self.wd
        p_new = p.clone()
        if self.kind == "lars":
            accum = slots[0].clone()
            for a, b in zip(seg, seg[1:]):
                pn, gn = float(p[a:b].norm()), float(g[a:b].norm())
                den = gn + wd * pn
                r = self.eta * pn / den if (pn > 0.0 and den > 0.0) else 1.0
                accum[a:b] = self.momentum * slots[0][a:b] + r * (g[a:b] + wd * p[a:b])
                p_new[a:b] = p[a:b] - lr * accum[a:b]
            return p_new, [accum]
        b1, b2, t = self.beta1, self.beta2, int(t)
        m = b1 * slots[0] + (1.0 - b1) * g
        v = b2 * slots[1] + (1.0 - b2) * g * g
        u = (m / (1.0 - b1 ** t)) / ((v / (1.0 - b2 ** t)).sqrt() + self.epsilon) + wd * p
        for a, b in zip(seg, seg[1:]):
            pn, un = float(p[a:b].norm()), float(u[a:b].norm())
            r = pn / un if (pn > 0.0 and un > 0.0) else 1.0
            p_new[a:b] = p[a:b] - lr * r * u[a:b]
        return p_new, [m, v]


def resolve(kind, weight_decay=0.0, eta=DEFAULT_ETA, **kw):
    """``None`` for a kind that is not layer-wise (today's code paths, untouched), else a
    validated ``Layerwise``."""
    return Layerwise(kind, weight_decay, eta, **kw) if is_layerwise(kind) else None


def from_flags(flags):
    """The ``Layerwise`` of ``--optimizer lars | lamb`` with ``--lars_eta``, ``--weight_decay``,
    ``--momentum`` and the ``--adam_*`` flags (validated), or ``None`` for another optimizer.
    ``--nesterov`` and an explicit ``--noadamw`` are refused.  ``--lars_eta`` is validated for
    every optimizer, so a bad value is never silently ignored."""
    from ..parallel import gpu_ps_optim

    d = gpu_ps_optim.DEFAULTS
    kind = getattr(flags, "optimizer", "sgd")
    try:
        eta = check_eta(getattr(flags, "lars_eta", DEFAULT_ETA))
    except ValueError as e:
        raise ValueError("--lars_eta: %s" % e)
    if not is_layerwise(kind):
        return None
    if getattr(flags, "nesterov", False):
        raise ValueError("--nesterov needs --optimizer momentum, got --optimizer %s" % kind)
    if kind == "lamb" and not getattr(flags, "adamw", True):
        raise ValueError("--noadamw has no meaning with --optimizer lamb: its weight decay is "
                         "inside the update direction by definition")
    try:
        return Layerwise(kind, getattr(flags, "weight_decay", 0.0) or 0.0, eta,
                         momentum=float(getattr(flags, "momentum", d["momentum"])),
                         beta1=float(getattr(flags, "adam_beta1", d["beta1"])),
                         beta2=float(getattr(flags, "adam_beta2", d["beta2"])),
                         epsilon=float(getattr(flags, "adam_epsilon", d["epsilon"])))
    except ValueError as e:
        raise ValueError("--weight_decay: %s" % e)


def lars_mixed_update(p, g, v, lr, tensors, momentum=0.9, wd=0.0, eta=DEFAULT_ETA, gscale=1.0):
    """The definition, in float64, of ResNet-50's LARS step (``ops.cnn.lars_momentum_mixed``)
    -> ``(p_new, v_new)`` (new tensors; inputs untouched; the bf16 copy is ``bf16(p_new)``,
    round-to-nearest-even).

    ``tensors``: ``(start, length, adapted)`` per tensor of the flat buffer, tiling it in order;
    ``g``: the gradient buffer, a folded tensor's range holding the sum of its split-K planes in
    plane order.  Per tensor ``g = gscale * G``; adapted tensors (2 or more dimensions: convolution
    and fc weights) take ``r = eta |p| / (|g| + wd |p|)`` when ``|p| > 0`` and the denominator is
    > 0, else ``r = 1``, and ``g' = r (g + wd p)``; excluded ones (1-D: BatchNorm scales / offsets,
    biases) take ``r = 1`` and no decay, ``g' = g``.  Then ``sgd_momentum_mixed``'s arithmetic on
    ``g'``: ``v = mu v + g'; p -= lr v``.  No Nesterov, no clipping function.

    This differs from the MLP's lars above only in the exclusion list (there every segment is
    adapted and decayed, biases included)."""
    import torch

    f64 = torch.float64
    p, g, v = (x.detach().to(f64).cpu() for x in (p, g, v))
    lr, mu, wd, eta, gscale = (float(x) for x in (lr, momentum, wd, eta, gscale))
    p_new, v_new = p.clone(), v.clone()
    at = 0
    for start, length, adapted in tensors:
        a, b = int(start), int(start) + int(length)
        if a != at or b <= a:
            raise ValueError("lars_mixed_update: the tensors must tile the buffer in order")
        at = b
        gs = gscale * g[a:b]
        if adapted:
            pn, gn = float(p[a:b].norm()), float(gs.norm())
            den = gn + wd * pn
            r = eta * pn / den if (pn > 0.0 and den > 0.0) else 1.0
            gs = r * (gs + wd * p[a:b])
        v_new[a:b] = mu * v[a:b] + gs
        p_new[a:b] = p[a:b] - lr * v_new[a:b]
    if at != p.numel():
        raise ValueError("lars_mixed_update: the tensors end at %d, the buffer has %d elements"
                         % (at, p.numel()))
    return p_new, v_new


def refuse(flags, what):
    """ValueError for a path without a norm pass (it names the ones that have it)."""
    kind = getattr(flags, "optimizer", "sgd")
    if is_layerwise(kind):
        raise ValueError("--optimizer %s: %s has no layer-wise update (it would need every "
                         "tensor's norm); it is supported by --strategy mirrored --model mlp "
                         "(the gradient-buffer engine on any number of GPUs; --device cpu), and "
                         "lars also by --strategy mirrored --model resnet50 (not with --zero1)"
                         % (kind, what))
