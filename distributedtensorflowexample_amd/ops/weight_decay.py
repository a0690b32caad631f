"""Weight decay (L2, AdamW) and Nesterov momentum of the fused MLP trainer: the definition.

One definition everywhere -- ``ops/optim.py`` / ``csrc/kernels/optim.hip``'s, which is
``torch.optim``'s.  ``wd`` = weight decay, ``lr_t`` = the rate of the step being applied (the
scheduled rate when a schedule is on), ``g`` = the batch-mean gradient, ``p`` any of the 79,510
parameters.  Decay is uniform over the flat buffer, biases included.

* sgd: ``p -= lr_t * (g + wd * p)``
* momentum: ``g' = g + wd * p; accum = mu * accum + g'; p -= lr_t * accum``
* momentum with ``nesterov``: the same ``g'`` and ``accum``, then ``p -= lr_t * (g' + mu * accum)``
* adam, ``adamw=False``: ``g' = g + wd * p`` goes into ``m`` and ``v``
* adam, ``adamw=True`` (the default, like ``ops.optim.adam_``): ``m`` and ``v`` take ``g`` and the
  parameter additionally loses ``lr_t * wd * p`` (decoupled)

The recorded loss stays the cross-entropy alone; a checkpoint carries nothing new (the Nesterov
accumulator is momentum's slot under momentum's name).

The fused step's first launch takes four wave-uniform words (``WeightDecay.words()``): ``l2`` and
``dec`` -- the coupled and the decoupled coefficient, one of them ``wd`` and the other 0 -- and
``(na, nb)`` of ``p -= lr_t * (na * g' + nb * accum)``: ``(0, 1)`` plain, ``(1, mu)`` Nesterov.
``weight_decay=0, nesterov=False`` resolves to ``None`` and launches exactly the kernels there were.
"""
from __future__ import annotations

import math

import numpy as np


def check(weight_decay):
    """``weight_decay`` as a finite float >= 0, else ValueError."""
    try:
        wd = float(weight_decay)
    except (TypeError, ValueError):
        raise ValueError("weight_decay must be a number, got %r" % (weight_decay,))
    if not math.isfinite(wd) or wd < 0.0:
        raise ValueError("weight_decay must be finite and >= 0, got %r" % (weight_decay,))
    return wd


class WeightDecay:
    """The terms of one (optimizer, weight_decay, adamw, nesterov): ``words()`` for the fused
    step's launchers, ``sgd_kw`` / ``momentum_kw`` / ``adam_kw`` for ``ops.optim``'s functions."""

    def __init__(self, kind, weight_decay=0.0, adamw=True, nesterov=False, momentum=0.9):
        self.kind = kind
        self.wd = check(weight_decay)
        self.nesterov = bool(nesterov)
        self.adamw = bool(adamw)
        if self.nesterov and kind != "momentum":
            raise ValueError("nesterov needs optimizer momentum, got %r" % (kind,))
        if self.wd == 0.0 and not self.nesterov:
            raise ValueError("WeightDecay: weight_decay 0 without nesterov is no term at all "
                             "(pass None to the step)")
        self.mu = float(np.float32(momentum))  # (what the kernel receives as h0)

    @property
    def decoupled(self):
        return self.kind == "adam" and self.adamw

    def words(self):
        """(l2, dec, na, nb) as the WD launchers take them."""
        l2, dec = (0.0, self.wd) if self.decoupled else (self.wd, 0.0)
        na, nb = (1.0, self.mu) if self.nesterov else (0.0, 1.0)
        return (l2, dec, na, nb)

    @property
    def sgd_kw(self):
        return dict(weight_decay=self.wd)

    @property
    def momentum_kw(self):
        return dict(weight_decay=self.wd, nesterov=self.nesterov)

    @property
    def adam_kw(self):
        return dict(weight_decay=self.wd, adamw=self.adamw)


def resolve(kind, weight_decay=0.0, adamw=True, nesterov=False, momentum=0.9):
    """``None`` for ``weight_decay == 0`` without Nesterov (today's code paths, untouched), else a
    ``WeightDecay``.  Validates either way: a negative or non-finite decay and Nesterov without
    momentum are refused."""
    wd = check(weight_decay)
    if nesterov and kind != "momentum":
        raise ValueError("nesterov needs optimizer momentum, got %r" % (kind,))
    if wd == 0.0 and not nesterov:
        return None
    return WeightDecay(kind, wd, adamw, nesterov, momentum)


def _flag_terms(flags):
    return (getattr(flags, "weight_decay", 0.0) or 0.0, bool(getattr(flags, "adamw", True)),
            bool(getattr(flags, "nesterov", False)))


def from_flags(flags):
    """The ``WeightDecay`` of ``--weight_decay`` / ``--adamw`` / ``--nesterov`` (validated), or
    ``None`` when they ask for nothing.  ``--adamw`` is read only with ``--optimizer adam``.  A
    flags object without them (an embedding caller's namespace) trains without the terms."""
    wd, adamw, nesterov = _flag_terms(flags)
    kind = getattr(flags, "optimizer", "sgd")
    if nesterov and kind != "momentum":
        raise ValueError("--nesterov needs --optimizer momentum, got --optimizer %s" % kind)
    try:
        return resolve(kind, wd, adamw, nesterov,
                       float(getattr(flags, "momentum", 0.9)))
    except ValueError as e:
        raise ValueError("--weight_decay: %s" % e)


def refuse(flags, what):
    """ValueError for a path without the terms (it names the one that has them)."""
    wd, _, nesterov = _flag_terms(flags)
    if check(wd) != 0.0 or nesterov:
        raise ValueError("--weight_decay / --nesterov: %s has no weight-decay or Nesterov variant; "
                         "they are supported by --strategy mirrored --model mlp (one GPU: the "
                         "fused two-launch step; several: the all-reduce engine; --device cpu)"
                         % what)
