"""Shared inputs and the float64 reference of the moving-average tests (``test_ema_cpu.py``,
``test_fused_ema_gpu.py``).

The update is written out here in float64 -- TF's ``assign_sub`` form of
``tf.train.ExponentialMovingAverage`` -- and calls nothing of the code under test except, with
``num_updates``, ``EMA.one_minus_decay_f32`` (the wave-uniform f32 coefficient the kernel computes;
``test_ema_cpu.py`` checks it against float64 on its own).  Hyper-parameters are rounded to
float32 first, as ``optim_reference`` does: that is what a kernel receives.

Inputs: ``weight_decay_reference``'s (parameters ``0.1 * randn`` with non-zero biases, batch sizes
1, 17, 100, 113, 256, three batches).  ``DECAY = 0.99``: with ``num_updates`` the applies from
``global_step`` 0 (t = 1, 2, 3) take ``(1 + t) / (10 + t)`` and the ones from 1000 (t = 1001..:
``1010 / 1019 > 0.99``) take ``decay`` -- both sides of the min().  ``shadow0`` sits ~0.1 from the
parameters, so one update moves a shadow element by ``(1 - d_t) * 0.1`` >= 1e-3 against an allowed
error of ``optim_reference.bound(1, ref)`` = 2.4e-7.
"""
import torch

import optim_reference as oref
import weight_decay_reference as wr
from distributedtensorflowexample_amd.ops import ema as ema_mod
from distributedtensorflowexample_amd.ops import lr_schedule, mlp_step

SIZES, NB, REGIONS, LR, WD = wr.SIZES, wr.NB, wr.REGIONS, wr.LR, wr.WD
data = wr.data
DECAY = 0.99
STARTS = (0, 1000)  # global_step before the first apply
SCHED = lr_schedule.LRSchedule("exponential", 4, 0.5, False, 3)

# name -> (optimizer, FusedMLPTrainer keywords besides the moving average's)
CASES = {
    "sgd": ("sgd", {}),
    "momentum": ("momentum", {}),
    "adam": ("adam", {}),
    "adam_sched": ("adam", dict(lr_schedule=SCHED)),
    "sgd_l2": ("sgd", dict(weight_decay=WD)),
}
# the trainers whose parameters and slots must not notice the shadow
NO_FEEDBACK = dict(CASES, adamw=("adam", dict(weight_decay=WD, adamw=True)),
                   adamw_sched=("adam", dict(weight_decay=WD, adamw=True, lr_schedule=SCHED)))
del NO_FEEDBACK["sgd_l2"]


def one_minus_decay(t, decay=DECAY, num_updates=False):
    """1 - d_t as the kernel holds it, widened to a Python float."""
    if num_updates:
        return float(ema_mod.EMA(decay, True).one_minus_decay_f32(t))
    return oref.f32(1.0 - decay)


def ref_update(shadow, p_new, t, decay=DECAY, num_updates=False):
    """float64 ``shadow - (1 - d_t) * (shadow - p_new)``; ``t`` = global_step + 1 of the update
    that produced ``p_new``."""
    e, v = shadow.detach().cpu().double(), p_new.detach().cpu().double()
    return e - one_minus_decay(t, decay, num_updates) * (e - v)


def shadow0(B):
    """A starting shadow ~0.1 per element away from ``data(B)``'s parameters."""
    gen = torch.Generator().manual_seed(11 + B)
    return data(B)[0] + 0.1 * torch.randn(mlp_step.NPARAM, generator=gen)


def bound1(ref):
    return oref.bound(1, ref)


def assert_visible(name, updated, untouched, tol_of=bound1):
    """On the references alone: the shadow after the update and the untouched shadow differ by at
    least 100 times the comparison's tolerance in each of W1, b1, W2 and b2 -- a kernel that
    leaves the shadow alone, or a region of it, cannot pass."""
    updated, untouched = updated.detach().cpu().double(), untouched.detach().cpu().double()
    for rname, idx in REGIONS:
        d = float((updated[idx] - untouched[idx]).abs().max())
        tol = tol_of(updated[idx])
        assert d >= 100.0 * tol, "%s[%s]: the update moves the shadow by %.3e < 100 x %.3e" % (
            name, rname, d, tol)


def cpu_param_step(B, kind, lr):
    """Parameters after one plain float64 step of ``kind`` from zero slots on ``data(B)``'s first
    batch (f32-rounded): a stand-in for the kernel's ``p_new`` in the CPU-side visibility check
    (the GPU's differs by rounding, ~1e-7, against a required shadow motion of >= 2.4e-5)."""
    p, x, y = data(B)
    g, _, _ = mlp_step.reference_step(p.double(), x[:B].double(), y[:B])
    slots = [torch.zeros_like(g) for _ in range({"sgd": 0, "momentum": 1, "adam": 2}[kind])]
    q, _ = wr.ref_apply(kind, p.double(), g, slots, lr, 1)
    return q.float()


def check_f32_coefficient(decay, t):
    """|one_minus_decay_f32 - float64| / float64 for ``num_updates`` at ``t``."""
    want = 1.0 - min(decay, (1.0 + t) / (10.0 + t))
    got = float(ema_mod.EMA(decay, True).one_minus_decay_f32(t))
    return abs(got - want) / want, got, want

