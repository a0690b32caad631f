"""Learning-rate schedules of the fused MLP trainer, evaluated on the device.

``s`` is the 0-based ``global_step`` of the step whose update is applied (the word Adam reads as
``t - 1``)::

    q       = s // decay_steps              if staircase      (integer division)
            = s / decay_steps               otherwise
    decay   = decay_rate ** q               kind "exponential"   (tf.train.exponential_decay)
            = 1 / (1 + decay_rate * q)      kind "inverse_time"  (tf.train.inverse_time_decay)
            = 1                             kind "constant"
    warm    = min(1, (s + 1) / warmup_steps)   if warmup_steps > 0, else 1
    lr(s)   = learning_rate * decay * warm

The schedule is a pure function of ``global_step``: a checkpoint needs nothing new, and a run
resumed with ``seek`` continues on the same curve.

``LRSchedule.value`` is the float64 definition.  ``value_f32`` is the device arithmetic of
``csrc/kernels/mlp_step_opt.h`` (``sched_rate``) in numpy float32, operation for operation: the
staircase quotient by integer division, ``float(s) * f32(1 / decay_steps)`` otherwise,
``exp2(q * f32(log2 decay_rate))``, ``1 / fma(decay_rate, q, 1)``, ``min(1, float(s + 1) *
f32(1 / warmup_steps))``.  The device's exp2 and reciprocal come from the transcendental unit
(1 ulp); numpy's are correctly rounded to within the same ulp, so the two agree to that ulp and
exactly wherever the result is exact (integer ``q`` with a power-of-two rate, ``decay_rate`` 1).
"""
from __future__ import annotations

import math

import numpy as np

KINDS = ("constant", "exponential", "inverse_time")
BLOCK_WORDS = 8   # int32 words of the device block: [tp0, tp1, flags, decay_steps, a, inv, invw, 0]


class LRSchedule:
    def __init__(self, kind="constant", decay_steps=1, decay_rate=1.0, staircase=False,
                 warmup_steps=0):
        kind = str(kind)
        if kind not in KINDS:
            raise ValueError("--lr_schedule must be one of %s, got %r" % ("|".join(KINDS), kind))
        if int(decay_steps) != decay_steps or int(decay_steps) < 1 or int(decay_steps) >= 2 ** 31:
            raise ValueError("--lr_decay_steps must be an integer >= 1, got %r" % (decay_steps,))
        if not (float(decay_rate) > 0.0) or not math.isfinite(float(decay_rate)):
            raise ValueError("--lr_decay_rate must be > 0, got %r" % (decay_rate,))
        if int(warmup_steps) != warmup_steps or int(warmup_steps) < 0:
            raise ValueError("--lr_warmup_steps must be an integer >= 0, got %r" % (warmup_steps,))
        self.kind = kind
        self.decay_steps = int(decay_steps)
        self.decay_rate = float(decay_rate)
        self.staircase = bool(staircase)
        self.warmup_steps = int(warmup_steps)

    def __repr__(self):
        return ("LRSchedule(%r, decay_steps=%d, decay_rate=%r, staircase=%r, warmup_steps=%d)"
                % (self.kind, self.decay_steps, self.decay_rate, self.staircase,
                   self.warmup_steps))

    @property
    def is_constant(self):
        """Today's constant rate: no decay kind and no warm-up."""
        return self.kind == "constant" and self.warmup_steps == 0

    # -- the oracle -----------------------------------------------------------------------
    def value(self, lr0, s):
        """``lr(s)`` by the definitions above in float64."""
        s = int(s)
        q = float(s // self.decay_steps) if self.staircase else s / self.decay_steps
        if self.kind == "exponential":
            decay = self.decay_rate ** q
        elif self.kind == "inverse_time":
            decay = 1.0 / (1.0 + self.decay_rate * q)
        else:
            decay = 1.0
        warm = min(1.0, (s + 1) / self.warmup_steps) if self.warmup_steps > 0 else 1.0
        return float(lr0) * decay * warm

    # -- the device's words -----------------------------------------------------------------
    def args(self):
        """``(flags, decay_steps, a, inv_decay_steps, inv_warmup)`` as the launchers take them
        (words 2..6 of the device block): ``flags = kind | staircase << 2``; ``a`` =
        f32(log2 decay_rate) for the exponential kind, f32(decay_rate) for inverse time; the
        reciprocals are formed in float64 and rounded once; ``inv_warmup`` = 0: no warm-up."""
        if self.kind == "exponential":
            a = np.float32(math.log2(self.decay_rate))
        elif self.kind == "inverse_time":
            a = np.float32(self.decay_rate)
        else:
            a = np.float32(0.0)
        inv = np.float32(1.0 / self.decay_steps)
        invw = np.float32(1.0 / self.warmup_steps) if self.warmup_steps > 0 else np.float32(0.0)
        flags = KINDS.index(self.kind) | (1 << 2 if self.staircase else 0)
        return (int(flags), self.decay_steps, float(a), float(inv), float(invw))

    def block_words(self):
        """The int32 [8] device block with a zero step pair: the float words as their bits."""
        flags, ds, a, inv, invw = self.args()
        w = np.zeros(BLOCK_WORDS, dtype=np.int32)
        w[2], w[3] = flags, ds
        w[4:7] = np.array([a, inv, invw], dtype=np.float32).view(np.int32)
        return w

    def value_f32(self, lr0, s):
        """The device arithmetic in numpy float32 -> numpy.float32."""
        f = np.float32
        _, ds, a, inv, invw = (self.args())
        a, inv, invw = f(a), f(inv), f(invw)
        s = int(s)
        q = f(s // ds) if self.staircase else f(f(s) * inv)
        if self.kind == "exponential":
            decay = f(np.exp2(f(q * a)))
        elif self.kind == "inverse_time":
            # fma(a, q, 1): the f32 product is exact in float64; one rounding of the sum
            decay = f(f(1.0) / f(np.float64(a) * np.float64(q) + 1.0))
        else:
            decay = f(1.0)
        lr = f(f(lr0) * decay)
        if self.warmup_steps > 0:
            lr = f(lr * np.minimum(f(1.0), f(f(s + 1) * invw)))
        return lr


def resolve(schedule):
    """``None`` for no schedule or the constant one without warm-up (today's trainer), else the
    ``LRSchedule``."""
    if schedule is None:
        return None
    if not isinstance(schedule, LRSchedule):
        raise ValueError("lr_schedule must be an ops.lr_schedule.LRSchedule, got %r" % (schedule,))
    return None if schedule.is_constant else schedule


def from_flags(flags):
    """The ``LRSchedule`` of ``--lr_schedule`` and its ``--lr_*`` flags (validated), or ``None``
    when they describe the constant rate.  A flags object without them (an embedding caller's
    namespace) trains at the constant rate."""
    if not hasattr(flags, "lr_schedule"):
        return None
    return resolve(LRSchedule(flags.lr_schedule, getattr(flags, "lr_decay_steps", 1000),
                              getattr(flags, "lr_decay_rate", 0.96),
                              getattr(flags, "lr_staircase", False),
                              getattr(flags, "lr_warmup_steps", 0)))


def refuse(flags, what):
    """ValueError for a path that trains at one constant rate only."""
    sched = from_flags(flags)
    if sched is not None:
        raise ValueError("--lr_schedule %s (warm-up %d): %s trains at a constant "
                         "--learning_rate; schedules are supported by --strategy mirrored "
                         "--model mlp (one GPU: the fused step; several: the all-reduce engine; "
                         "--device cpu)" % (sched.kind, sched.warmup_steps, what))
