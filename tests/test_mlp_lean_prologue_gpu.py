"""The operand addressing of the two lean launches' prologues (head_row<.., SB> in
csrc/kernels/mlp_step_3launch.h, fwdapply_block in csrc/kernels/mlp_step_fwdapply.h;
profiles/lean_prologue/): the head's 28 slab loads go through one buffer descriptor (lane offset
in the vector offset, plane and row in the scalar one).  The same series measured the first
launch's dz1R / x_prev loads through descriptors with 32-bit offsets (the row clamp
``min(row, B - 1)`` as an add and a min per row quad) and did not keep them; the cases below were
chosen for both and hold for any form of the two launches.  Against the untouched generic pair
``mlp_fwdapply(ks=28)`` + ``mlp_head2(single=1)``, BIT for bit, with the comparison of
tests/test_mlp_wide_stores_gpu.py (both parameter buffers, stats ring, global_step, dz1R, dlR,
hbuf, rowstat, the whole slab), over 4 steps and the flush, at the batch sizes where such
addressing can go wrong and that file and tests/test_mlp_lean_step_gpu.py do not reach:

* 3: one partly live row quad (every other quad of every wave clamped);
* 99: the last live quad holds 3 rows;
* 112: ``NGT = 7`` with no clamped row;
* 113: the first size on the generic ``NGT = 0`` instantiation;
* 255.

Guard rows (3, 99, 113): the batches are the END of an x buffer that has 16 rows of NaN before
them and 16 behind them, and the labels have a guard value (a class out of range) on both sides.
A dropped or shifted row clamp reads a NaN row, which shows as NaN in the parameters and as a
difference from the generic pair.

The momentum and Adam instantiations and their flush after 3 and after 4 steps, at batch 99:
the float64 ``torch.optim`` references fed the kernel's own gradient and the bound of
tests/test_fused_optim_gpu.py (``optim_reference.assert_close``), as they stand there.
"""
import pytest
import torch

import optim_reference as oref
import test_fused_optim_gpu as tfo
import test_mlp_wide_stores_gpu as tws
from distributedtensorflowexample_amd.ops import mlp_step

pytestmark = pytest.mark.gpu

NB, KS, HP, GUARD = tws.NB, tws.KS, tws.HP, 16


def _guarded(gpu, B):
    """(p, x, y) of tws._setup with the NB batches at the end of a buffer between NaN rows."""
    p, x, y = tws._setup(gpu, B)
    xg = torch.full((GUARD + NB * B + GUARD, 784), float("nan"), device=gpu)
    xg[GUARD:GUARD + NB * B] = x
    yg = torch.full((GUARD + NB * B + GUARD,), 1 << 20, device=gpu, dtype=torch.int32)
    yg[GUARD:GUARD + NB * B] = y
    xv, yv = xg[GUARD:GUARD + NB * B], yg[GUARD:GUARD + NB * B]
    assert xv.data_ptr() == xg.data_ptr() + GUARD * 784 * 4 and xv.is_contiguous()
    return p, xv, yv, (xg, yg)


def _no_nan(state, what):
    for k, v in state.items():
        if v.is_floating_point():
            assert not bool(torch.isnan(v).any()), "%s: NaN in %s" % (what, k)


@pytest.mark.parametrize("B", [3, 99, 112, 113, 255])
def test_edge_batches_bit_identical_to_generic_pair(gpu, B):
    if B in (3, 99, 113):
        p, x, y, keep = _guarded(gpu, B)
    else:
        p, x, y = tws._setup(gpu, B)
    new = tws._steps_then_flush(gpu, p, x, y, B, True, 4)
    old = tws._steps_then_flush(gpu, p, x, y, B, False, 4)
    BP = (B + 15) // 16 * 16
    assert float(old[0]["slab"].view(KS, BP, HP)[:, :B, :100].abs().sum()) > 0
    assert float(old[1]["stats"].abs().sum()) > 0
    for half, when in ((0, "before"), (1, "after")):
        # (4 steps and the flush: every parameter buffer has been written by then)
        _no_nan(old[half], "generic pair, B=%d %s the flush" % (B, when))
        _no_nan(new[half], "lean pair, B=%d %s the flush" % (B, when))
        tws._assert_same(new[half], old[half], "B=%d %s the flush" % (B, when))


@pytest.mark.parametrize("steps", [3, 4])
@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_optimizer_instantiations_and_flush_at_99(gpu, kind, steps):
    """``steps`` applies from non-zero slots at lr = 1e-3, the last one by flush() (the apply-only
    instantiation), the others inside the following steps' first launches: parameters and slots
    against torch.optim in float64 fed the kernel's own gradient, within
    optim_reference.bound(k, ref) after k applies (test_fused_optim_gpu's second test at batch
    99 and over both step counts)."""
    B, lr = 99, 1e-3
    data = tfo._data(B)
    oracle = tfo._trainer(gpu, B, lr, data, optimizer="momentum", momentum=0.0)
    tr = tfo._trainer(gpu, B, lr, data, optimizer=kind)
    gen = torch.Generator().manual_seed(7 + B)
    m0 = 0.1 * torch.randn(mlp_step.NPARAM, generator=gen)
    v0 = 0.01 + 0.1 * torch.rand(mlp_step.NPARAM, generator=gen)
    slots0 = [m0] if kind == "momentum" else [m0, v0]
    tr.load_slots([s.to(gpu) for s in slots0])
    ref_p = data[0].double()
    ref_s = [s.double() for s in slots0]
    tr.step()
    for k in range(1, steps + 1):
        assert tr.pending
        g = tfo._kernel_gradient(oracle, tr.params.clone(), k - 1).cpu()
        if k < steps:
            tr.step()
        else:
            tr.flush()
        torch.cuda.synchronize()
        if kind == "momentum":
            ref_p, buf = oref.sgd_step(ref_p, g, lr, mu=0.9, buf=ref_s[0])
            ref_s = [buf]
        else:
            ref_p, m, v = oref.adam_step(ref_p, g, ref_s[0], ref_s[1], lr, k, eps=1e-8, wd=0.0,
                                         adamw=False)
            ref_s = [m, v]
        oref.assert_close("p after %d" % k, tr.params, ref_p, k, tfo.REGIONS)
        for i, (s, r) in enumerate(zip(tr.slots, ref_s)):
            oref.assert_close("slot %d after %d" % (i, k), s, r, k, tfo.REGIONS)
    assert tr.global_step() == steps
