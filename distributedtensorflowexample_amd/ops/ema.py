"""Moving average of the parameters of the fused MLP trainer (``--ema_decay``): the definition.

``tf.train.ExponentialMovingAverage``: every variable has a *shadow* that follows it, and a TF
user evaluates and exports the shadows instead of the raw variables.  After the update of step
``s`` (the 0-based ``global_step``; ``t = s + 1``) has produced the parameters ``p_t``::

    shadow_t = shadow_{t-1} - (1 - d_t) * (shadow_{t-1} - p_t)        # TF's assign_sub form
    d_t = decay                                   (num_updates off)
    d_t = min(decay, (1 + t) / (10 + t))          (num_updates on: TF's num_updates = global_step,
                                                   read after the train op incremented it)

* ``shadow_0`` is the initial parameters, as in TF; there is no zero-debias.
* ``0 < decay < 1``; ``decay == 0`` resolves to ``None`` (no shadow, today's kernels).
* The shadow covers the whole flat buffer, biases included, and never feeds back into training.
* Nothing pending (``apply == 0``) touches no shadow byte.

On the device ``1 - d_t`` is wave-uniform: ``1 - (1 + t) / (10 + t) = 9 / (10 + t)``, so it is
``max(omd, 9 / (10 + t))`` with ``omd = f32(1 - decay)``, computed once per wave from the step
word (``csrc/kernels/mlp_step_opt.h``: ``ema_omd``; ``optim.hip``'s ``ema_kernel`` the same);
``one_minus_decay_f32`` is that arithmetic operation for operation.  The fused step's first
launch takes three words (``EMA.words()``): the shadow plane's address comes from the caller,
then ``omd`` and the ``num_updates`` flag.
"""
from __future__ import annotations

import math

import numpy as np


def check(decay):
    """``decay`` as a float in [0, 1), else ValueError (0 = off)."""
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError("ema_decay must be a number, got %r" % (decay,))
    if not math.isfinite(d) or d < 0.0 or d >= 1.0:
        raise ValueError("ema_decay must lie in (0, 1), or be 0 for no moving average, got %r"
                         % (decay,))
    return d


class EMA:
    """One (decay, num_updates): the float64 definition, the device arithmetic and the words the
    launchers take."""

    def __init__(self, decay, num_updates=False):
        self.decay = check(decay)
        if self.decay == 0.0:
            raise ValueError("EMA: decay 0 is no moving average at all (pass None to the step)")
        self.num_updates = bool(num_updates)
        self.omd = float(np.float32(1.0 - self.decay))  # (what the kernel receives)
        if not 0.0 < self.omd < 1.0:
            raise ValueError("ema_decay %r: 1 - decay is not in (0, 1) as float32" % (decay,))

    def __repr__(self):
        return "EMA(decay=%r, num_updates=%r)" % (self.decay, self.num_updates)

    def decay_at(self, t):
        """d_t in float64; ``t`` = global_step + 1 of the step whose update is averaged."""
        t = int(t)
        return min(self.decay, (1.0 + t) / (10.0 + t)) if self.num_updates else self.decay

    def update(self, shadow, p_new, t):
        """The definition in float64: the new shadow (a new array / tensor; inputs untouched)."""
        omd = 1.0 - self.decay_at(t)
        if hasattr(shadow, "detach"):  # torch tensors
            import torch

            e, v = shadow.to(torch.float64), p_new.to(torch.float64)
        else:
            e, v = np.asarray(shadow, np.float64), np.asarray(p_new, np.float64)
        return e - omd * (e - v)

    def one_minus_decay_f32(self, t):
        """The device arithmetic in numpy float32 -> numpy.float32."""
        f = np.float32
        omd = f(self.omd)
        if not self.num_updates:
            return omd
        q = f(f(9.0) / f(f(10.0) + f(int(t))))  # (a correctly rounded f32 division)
        return np.maximum(omd, q)

    def words(self):
        """(omd, num_updates) as the moving-average launchers take them after the shadow
        plane's address."""
        return (self.omd, 1 if self.num_updates else 0)


def resolve(decay, num_updates=False):
    """``None`` for ``decay == 0`` (today's code paths, untouched), else an ``EMA``.  Validates
    either way."""
    d = check(decay)
    return None if d == 0.0 else EMA(d, num_updates)


def _flag_terms(flags):
    return (getattr(flags, "ema_decay", 0.0) or 0.0, bool(getattr(flags, "ema_num_updates", False)))


def from_flags(flags):
    """The ``EMA`` of ``--ema_decay`` / ``--ema_num_updates`` (validated), or ``None`` when the
    moving average is off.  ``--ema_num_updates`` and ``--eval_ema`` need ``--ema_decay`` (the
    eval job, which only reads a checkpoint, is exempt from the latter).  A flags object without
    them (an embedding caller's namespace) trains without a shadow."""
    decay, nu = _flag_terms(flags)
    try:
        ema = resolve(decay, nu)
    except ValueError as e:
        raise ValueError("--ema_decay: %s" % e)
    if ema is None and nu:
        raise ValueError("--ema_num_updates needs --ema_decay > 0")
    if (ema is None and getattr(flags, "eval_ema", False)
            and getattr(flags, "job_name", "") != "eval"):
        raise ValueError("--eval_ema needs --ema_decay > 0 (there are no averaged variables to "
                         "evaluate)")
    return ema


def refuse(flags, what):
    """ValueError for a path without a shadow (it names the one that has it)."""
    decay, nu = _flag_terms(flags)
    if check(decay) != 0.0 or nu:
        raise ValueError("--ema_decay / --ema_num_updates: %s keeps no moving average of the "
                         "parameters; it is supported by --strategy mirrored --model mlp (one "
                         "GPU: the fused two-launch step; several: the all-reduce engine; "
                         "--device cpu)" % what)


def tf_name(variable):
    """The checkpoint name of ``variable``'s shadow, as TF's ``variables_to_restore`` maps it."""
    return variable + "/ExponentialMovingAverage"
