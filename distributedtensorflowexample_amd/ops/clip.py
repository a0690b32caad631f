"""Clipping the gradient by its global norm in the fused MLP trainer (``--clip_norm``): the
definition.

``tf.clip_by_global_norm`` (clip 1.0 in the LAMB and BERT large-batch recipes)::

    norm = sqrt(sum_i g_i^2)                  over ALL 79,510 elements of the flat gradient
    f    = clip_norm / max(norm, clip_norm)
    g   <- g * f

* ``g`` is the gradient of the batch-mean loss averaged over the replicas: after the all-reduce
  and the ``1 / world`` scale.
* Clipping comes first, as in TF and torch: weight decay, momentum, the Adam moments and the
  LARS / LAMB trust ratios all see the clipped ``g``.
* ``clip_norm`` is finite and > 0; ``0`` resolves to ``None`` (off: today's kernels).
* ``norm <= clip_norm`` gives ``f = 1`` exactly: the gradient's bits do not change.
* A non-finite gradient gives a non-finite result, as in TF; there is no special case.

On the device (``csrc/kernels/optim.hip``) the average and the clip are ONE multiplier: with
``pre = 1 / world`` the norm of ``pre g`` is ``pre |g|``, so the sums of squares are taken from the
unscaled gradient -- one partial per workgroup of ``BLOCK`` = 1,024 elements, by ``gnorm_partials``
or, above 256 rows on one GPU, by the large-batch reduce launch that stores the gradient -- and
``clip_scale`` multiplies by ``pre * clip_norm / max(pre * sqrt(sum), clip_norm)`` in the launch
that used to multiply by ``pre``.  The pre-clip ``norm`` lands in a one-float device tensor.
"""
from __future__ import annotations

import math

BLOCK = 1024


def check(clip_norm):
    """``clip_norm`` as a finite float >= 0, else ValueError (0 = off)."""
    try:
        c = float(clip_norm)
    except (TypeError, ValueError):
        raise ValueError("clip_norm must be a number, got %r" % (clip_norm,))
    if not math.isfinite(c) or c < 0.0:
        raise ValueError("clip_norm must be finite and > 0, or 0 for no clipping, got %r"
                         % (clip_norm,))
    return c


def resolve(clip_norm):
    """``None`` for ``clip_norm == 0`` (today's code paths, untouched), else the validated float."""
    return check(clip_norm) or None


def num_partials(n):
    """Partial sums (workgroups of ``BLOCK`` elements) of a gradient of ``n`` elements."""
    return (int(n) + BLOCK - 1) // BLOCK


def clip(g, clip_norm, pre=1.0):
    """The definition in float64 -> ``(clipped pre * g, norm of pre * g)`` (a new tensor and a
    float; ``g`` untouched)."""
    import torch

    c = check(clip_norm)
    if c == 0.0:
        raise ValueError("clip: clip_norm 0 is no clipping at all")
    g = g.detach().to(torch.float64) * float(pre)
    norm = float(g.norm())
    return g * (c / max(norm, c)), norm


def from_flags(flags):
    """The validated ``--clip_norm``, or ``None`` when clipping is off.  A flags object without it
    (an embedding caller's namespace) trains unclipped."""
    try:
        return resolve(getattr(flags, "clip_norm", 0.0) or 0.0)
    except ValueError as e:
        raise ValueError("--clip_norm: %s" % e)


def refuse(flags, what):
    """ValueError for a path without a global norm (it names the one that has it)."""
    if from_flags(flags) is not None:
        raise ValueError("--clip_norm: %s does not clip the gradient (it would need the norm of "
                         "the whole gradient); it is supported by --strategy mirrored --model mlp "
                         "(the gradient-buffer engine on any number of GPUs; --device cpu)" % what)
