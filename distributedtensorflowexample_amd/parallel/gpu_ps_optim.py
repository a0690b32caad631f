"""Stateful optimizers on the GPU-resident parameter store: names, hyper-parameters, reference.

``--optimizer momentum | adam`` keeps the optimizer's slot variables in the store's allocation,
next to the variables, as TF keeps them on the ps; the store's apply kernels
(``csrc/kernels/gpu_ps.hip``: ``gps_apply_opt_kernel`` and the closer of
``gps_sync_push_kernel``) update them.  The formulas are ``ops/optim.py``'s ``momentum_`` and
``adam_`` with ``weight_decay = 0`` and no Nesterov:

* momentum: ``accum = mu * accum + g; p -= lr * accum``
* adam: ``m = b1 * m + (1 - b1) * g; v = b2 * v + (1 - b2) * g * g;
  p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)``

``t`` is not a variable: it is ``global_step + 1`` at apply time (in a sync round exactly
``round + 1``), so a restored ``global_step`` restores it and there are no ``beta*_power``
variables.

This module is pure Python / NumPy (no GPU, no native module), like ``gpu_ps_sync.py``.
"""
from __future__ import annotations

import numpy as np

KINDS = ("sgd", "momentum", "adam")
# TF's slot names (tf.train.MomentumOptimizer / AdamOptimizer): <variable>/<slot>, in the
# order of the store's planes
SLOT_NAMES = {"sgd": (), "momentum": ("Momentum",), "adam": ("Adam", "Adam_1")}
DEFAULTS = {"momentum": 0.9, "beta1": 0.9, "beta2": 0.999, "epsilon": 1e-8}


def check_kind(kind):
    kind = str(kind)
    if kind not in KINDS:
        raise ValueError("--optimizer must be one of %s, got %r" % ("|".join(KINDS), kind))
    return kind


def num_slots(kind):
    """Planes the store appends for ``kind`` (also the kind's number in the control block)."""
    return len(SLOT_NAMES[check_kind(kind)])


def slot_names(kind, var_names):
    """[[<var>/<slot> for each variable] for each plane of ``kind``]."""
    return [["%s/%s" % (v, s) for v in var_names] for s in SLOT_NAMES[check_kind(kind)]]


def hyper_args(kind, momentum=DEFAULTS["momentum"], beta1=DEFAULTS["beta1"],
               beta2=DEFAULTS["beta2"], epsilon=DEFAULTS["epsilon"]):
    """The kernels' three hyper-parameter words ``(h0, h1, h2)``: momentum ``(mu, 0, 0)``,
    adam ``(beta1, beta2, epsilon)``, sgd none."""
    kind = check_kind(kind)
    if kind == "momentum":
        return (float(momentum), 0.0, 0.0)
    if kind == "adam":
        return (float(beta1), float(beta2), float(epsilon))
    return ()


def validate(kind, ps_device, use_locking):
    """The combinations ``--optimizer`` supports; ValueError otherwise (before any device or
    server is touched)."""
    kind = check_kind(kind)
    if kind == "sgd":
        return kind
    if str(ps_device) != "gpu":
        raise ValueError("--optimizer %s needs --ps_device gpu: the TCP ps applies gradient "
                         "descent only" % kind)
    if use_locking:
        raise ValueError("--optimizer %s does not support --use_locking: a locked "
                         "read-modify-write of the parameters and their slots would need a "
                         "kernel that waits on another process, which the GPU store never "
                         "does" % kind)
    return kind


def _f32(x):
    return np.float32(x)


def _muladd(a, b, c, fma):
    """a * b + c in f32: product and sum rounded separately, or (``fma``) the product feeding
    the sum unrounded -- emulated in float64, where the product of two f32 values is exact."""
    if fma:
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64)
                + np.asarray(c, np.float64)).astype(np.float32)
    return (np.asarray(a * b, np.float32) + c).astype(np.float32)


def mean_gradient(grads):
    """A sync round's ``gbar`` as the closer forms it: ``s = ((g[0] + g[1]) + ...)`` in ticket
    order in f32, times ``1 / R`` rounded to f32 once."""
    gs = [np.asarray(g, dtype=np.float32) for g in grads]
    s = gs[0].copy()
    for g in gs[1:]:
        s = (s + g).astype(np.float32)
    return (s * (_f32(1.0) / _f32(len(gs)))).astype(np.float32)


def apply_reference(kind, p, g, slots, lr, t, hyper, fma=False):
    """One apply of ``kind`` in f32 the way the kernel evaluates it -> ``(p, [slots])``.

    ``p``, ``g`` and each of ``slots`` (momentum: ``[accum]``; adam: ``[m, v]``; sgd: ``[]``)
    are f32 arrays; ``hyper`` is :func:`hyper_args`' tuple; ``t`` the 1-based step
    (``global_step + 1``; only adam uses it).  ``g`` is the gradient the optimizer sees: in a
    sync round :func:`mean_gradient` of the tickets' gradients.  ``fma=True`` fuses every
    ``a * b + c`` of the update (see ``gpu_ps_sync.round_reference``); for data on which every
    product and sum is exact both give the same bits."""
    kind = check_kind(kind)
    p = np.asarray(p, dtype=np.float32)
    g = np.asarray(g, dtype=np.float32)
    slots = [np.asarray(s, dtype=np.float32) for s in slots]
    if len(slots) != num_slots(kind):
        raise ValueError("%s takes %d slot arrays, got %d" % (kind, num_slots(kind), len(slots)))
    lr = _f32(lr)
    if kind == "sgd":
        return _muladd(-lr, g, p, fma), []
    if kind == "momentum":
        mu = _f32(hyper[0])
        accum = _muladd(mu, slots[0], g, fma)
        return _muladd(-lr, accum, p, fma), [accum]
    b1, b2, eps = (_f32(h) for h in hyper)
    one, tf = _f32(1.0), _f32(t)
    step_size = lr / (one - np.power(b1, tf, dtype=np.float32))
    rbc2 = one / np.sqrt(one - np.power(b2, tf, dtype=np.float32))
    m = _muladd(b1, slots[0], ((one - b1) * g).astype(np.float32), fma)
    v = _muladd(b2, slots[1], (((one - b2) * g).astype(np.float32) * g).astype(np.float32), fma)
    denom = _muladd(np.sqrt(v), rbc2, eps, fma)
    upd = ((step_size * m).astype(np.float32) / denom).astype(np.float32)
    return (p - upd).astype(np.float32), [m, v]
