"""Shared inputs and float64 references of the weight-decay / Nesterov tests
(``test_weight_decay_cpu.py``, ``test_fused_weight_decay_gpu.py``).

The update rules are ``optim_reference``'s -- ``torch.optim`` on float64 tensors -- and the model
is ``mlp_step.reference_step`` in float64; nothing here calls the code under test except the
f32 CPU yardstick of the trajectories (``ops.optim``'s CPU branches), which only sets how far
an f32 run may sit from the float64 one.

Inputs: parameters ``0.1 * randn`` over all 79,510 elements, biases included (with zero biases a
missing bias decay shows nothing on the first apply); ``weight_decay = 0.05``; sgd and momentum
at ``lr = 0.3``, adam at ``lr = 0.01``.  One apply then moves a parameter of magnitude 0.1 by
``lr * wd * |p|`` = 1.5e-3 (sgd, momentum) or 5e-5 (AdamW) against an allowed error of
``optim_reference.bound(1, ref)`` = 2.4e-7.
"""
import numpy as np
import torch

import optim_reference as oref
from distributedtensorflowexample_amd.ops import lr_schedule, mlp_step

SIZES = [1, 17, 100, 113, 256]
NB = 3
WD = 0.05
MU = 0.9
LR = {"sgd": 0.3, "momentum": 0.3, "adam": 0.01}
REGIONS = [("W1", torch.arange(mlp_step.OFF_W1, mlp_step.OFF_B1)),
           ("b1", torch.arange(mlp_step.OFF_B1, mlp_step.OFF_W2)),
           ("W2", torch.arange(mlp_step.OFF_W2, mlp_step.OFF_B2)),
           ("b2", torch.arange(mlp_step.OFF_B2, mlp_step.NPARAM))]
assert [int(r[0]) for _, r in REGIONS] == [0, 78400, 78500, 79500]

# name -> (optimizer, FusedMLPTrainer keywords of the term)
CASES = {
    "sgd_l2": ("sgd", dict(weight_decay=WD)),
    "momentum_l2": ("momentum", dict(weight_decay=WD)),
    "nesterov": ("momentum", dict(nesterov=True)),
    "nesterov_l2": ("momentum", dict(weight_decay=WD, nesterov=True)),
    "adam_l2": ("adam", dict(weight_decay=WD, adamw=False)),
    "adamw": ("adam", dict(weight_decay=WD, adamw=True)),
}


def data(B, nb=NB, seed=0, extra=0):
    """CPU f32 (p, x, y): the same values wherever they are generated."""
    g = torch.Generator().manual_seed(1000 * seed + B + 31)
    p = 0.1 * torch.randn(mlp_step.NPARAM, generator=g)
    x = torch.rand(nb * B + extra, 784, generator=g)
    y = torch.randint(0, 10, (nb * B + extra,), generator=g).int()
    return p, x, y


def slots0(kind, B):
    """Non-zero starting slots (momentum: [accum]; adam: [m, v]; sgd: [])."""
    gen = torch.Generator().manual_seed(7 + B)
    m0 = 0.1 * torch.randn(mlp_step.NPARAM, generator=gen)
    v0 = 0.01 + 0.1 * torch.rand(mlp_step.NPARAM, generator=gen)
    return {"sgd": [], "momentum": [m0], "adam": [m0, v0]}[kind]


def ref_apply(kind, p, g, slots, lr, t, weight_decay=0.0, adamw=True, nesterov=False, mu=MU,
              eps=1e-8):
    """One float64 ``torch.optim`` step number ``t`` (1-based) -> (p, slots)."""
    if kind == "adam":
        q, m, v = oref.adam_step(p, g, slots[0], slots[1], lr, t, eps=eps, wd=weight_decay,
                                 adamw=adamw)
        return q, [m, v]
    if kind == "momentum":
        q, buf = oref.sgd_step(p, g, lr, wd=weight_decay, mu=mu, nesterov=nesterov, buf=slots[0])
        return q, [buf]
    q, _ = oref.sgd_step(p, g, lr, wd=weight_decay)
    return q, []


def plain_terms(term):
    """The keywords of the same optimizer WITHOUT the term under test: no decay; a Nesterov
    case without decay falls back to plain momentum."""
    if term.get("weight_decay", 0.0):
        return dict(term, weight_decay=0.0)
    return dict(term, nesterov=False)


def assert_term_visible(name, with_term, without, tol_of):
    """The condition every comparison test asserts on the float64 references alone: the
    reference with the term and the one without differ by at least 100 times the comparison's
    tolerance in each of W1, b1, W2 and b2 -- a kernel that ignores the term cannot pass."""
    for rname, idx in REGIONS:
        d = float((with_term[idx] - without[idx]).abs().max())
        tol = tol_of(with_term[idx])
        assert d >= 100.0 * tol, "%s[%s]: the term moves the reference by %.3e < 100 x %.3e" % (
            name, rname, d, tol)


# ---- trajectories --------------------------------------------------------------------------------
TRAJ_STEPS = 12
TRAJ_EPS = 1e-3  # (as test_fused_optim_gpu.py: at 1e-8 a vanishing gradient moves +-lr either way)
TRAJ_MARGIN = 4.0
TRAJ = {
    "sgd_l2": ("sgd", dict(weight_decay=WD), None),
    "nesterov_l2": ("momentum", dict(weight_decay=WD, nesterov=True), None),
    "adamw_sched": ("adam", dict(weight_decay=WD, adamw=True),
                    lr_schedule.LRSchedule("exponential", 4, 0.5, False, 3)),
}


def trajectory(case, B, dtype, steps=TRAJ_STEPS):
    """``steps`` whole-model steps on the CPU.  float64: ``reference_step`` + ``torch.optim``
    (the oracle).  float32: ``reference_step`` in f32 + ``ops.optim``'s CPU branches (the
    yardstick of the f32 / f64 gap).  The scheduled rate of step s is ``value_f32`` for both."""
    from distributedtensorflowexample_amd.ops import optim

    kind, term, sched = TRAJ[case]
    p, x, y = data(B)
    p, x = p.to(dtype), x.to(dtype)
    slots = [torch.zeros_like(p) for _ in range({"sgd": 0, "momentum": 1, "adam": 2}[kind])]
    wd = term.get("weight_decay", 0.0)
    for s in range(steps):
        sl = slice((s % NB) * B, (s % NB + 1) * B)
        g, _, _ = mlp_step.reference_step(p, x[sl], y[sl])
        lr = LR[kind] if sched is None else float(sched.value_f32(LR[kind], s))
        if dtype == torch.float64:
            p, slots = ref_apply(kind, p, g, slots, lr, s + 1, eps=TRAJ_EPS, **term)
        elif kind == "sgd":
            optim.sgd_(p, g, float(np.float32(lr)), weight_decay=oref.f32(wd))
        elif kind == "momentum":
            optim.momentum_(p, g, slots[0], float(np.float32(lr)), momentum=oref.f32(MU),
                            weight_decay=oref.f32(wd), nesterov=term.get("nesterov", False))
        else:
            optim.adam_(p, g, slots[0], slots[1], float(np.float32(lr)), s + 1,
                        beta1=oref.f32(0.9), beta2=oref.f32(0.999), eps=oref.f32(TRAJ_EPS),
                        weight_decay=oref.f32(wd), adamw=term.get("adamw", True))
    return p, slots


_TRAJ = {}


def traj(case, B):
    """(float64 parameters, tolerance, measured CPU gap) of a trajectory case, computed once:
    tolerance = TRAJ_MARGIN x max |p_f32 - p_f64| of the two CPU runs, as test_fused_optim_gpu.py
    derives its traj_tol (the MFMA's summation order is not the CPU's)."""
    if (case, B) not in _TRAJ:
        p64, _ = trajectory(case, B, torch.float64)
        p32, _ = trajectory(case, B, torch.float32)
        gap = float((p32.double() - p64).abs().max())
        _TRAJ[(case, B)] = (p64, TRAJ_MARGIN * gap, gap)
    return _TRAJ[(case, B)]
