"""Large-batch gradient of the reference MNIST MLP: the fused step above 256 rows.

Python side of ``csrc/kernels/mlp_large_batch.hip`` (that file opens with the kernel design).
``ops.mlp_step``'s launches are shaped for a batch of at most ``mlp_step.MAX_BATCH`` = 256 rows;
for ``MAX_BATCH < B <= MAX_LARGE_BATCH`` the step is::

    mlp_lb_fwdhead : 16 rows per workgroup, K = 784 over its 4 waves -> h, dz1, dlogits, row stats
    mlp_lb_wgrad   : the batch in S slices of R rows -> one partial gradient plane per slice
    mlp_lb_reduce  : the planes in slice order -> flat gradient, stats record, global_step += 1

It leaves the flat 79,510-element gradient of the batch mean loss in ``grad`` -- what
``mlp_step.step_grad`` leaves below 256 -- for ``FusedMLPTrainer``'s all-reduce engine, which
applies it through ``ops.optim``.  Fixed summation order: the same inputs give the same bits.
Any batch in the range works, not only multiples of 16.  No dropout variant yet.

Mixed precision (``csrc/kernels/mlp_large_batch_bf16.hip``): ``step_grad_bf16`` takes the batch as
bf16 rows and runs the two 784-wide GEMMs on the bf16 MFMA with f32 accumulation; the parameters,
the head, the small parameters and the gradient stay f32.  Its workspace is
``LargeBatchWorkspace(..., bf16=True)`` (a layout of its own).
"""
from __future__ import annotations

import torch

from . import hidden_act, mlp_step
from ._ext import hip, ptr, stream_handle

MIN_LARGE_BATCH = mlp_step.MAX_BATCH + 1
MAX_LARGE_BATCH = 65536


def slices(B):
    """(S, R): the weight-gradient launch cuts the batch into S slices of R rows (R a multiple of
    16 in [64, 256], chosen from B alone; S >= 2)."""
    S, R = hip().mlp_lb_slices(int(B))
    return int(S), int(R)


def slices_bf16(B):
    """(S, R) of the bf16 weight-gradient launch: R a multiple of 32 in [64, 256]; S >= 2."""
    S, R = hip().mlp_lbh_slices(int(B))
    return int(S), int(R)


class LargeBatchWorkspace:
    """Device scratch of the large-batch step for batch size ``B``, with the attributes
    ``FusedMLPTrainer`` uses on ``mlp_step.StepWorkspace``: ``buf`` (zeroed once; its last four
    words are the hand-off words ``check()`` reads), the device ``global_step`` counter ``ctr``
    and the stats ring.  ``bf16``: the workspace of ``step_grad_bf16`` (it also holds dz1 as a bf16
    plane, whose padding rows rely on the zeroing here)."""

    def __init__(self, B, device, stats_ring=4096, bf16=False):
        if not MIN_LARGE_BATCH <= B <= MAX_LARGE_BATCH:
            raise ValueError("the large-batch MLP step supports %d <= batch <= %d"
                             % (MIN_LARGE_BATCH, MAX_LARGE_BATCH))
        self.B = int(B)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("the large-batch MLP step runs on the GPU")
        self.bf16 = bool(bf16)
        floats = hip().mlp_lbh_workspace_floats if self.bf16 else hip().mlp_lb_workspace_floats
        self.buf = torch.zeros(int(floats(self.B)), device=device, dtype=torch.float32)
        self.ctr = torch.zeros(1, device=device, dtype=torch.int32)
        self.stats_ring = stats_ring
        self.stats = torch.zeros(stats_ring, 2, device=device, dtype=torch.float32)

    def global_step(self) -> int:
        return int(self.ctr[0].item())

    def set_global_step(self, s: int):
        self.ctr.fill_(int(s))

    def factors_bf16(self):
        """Views of a bf16 workspace's factor regions: ``h`` [BP, 112], ``dz1`` [BP, 112], ``dl``
        [BP, 16] (f32, BP = B rounded up to 16) and ``dz1h`` [BP32, 112] (bf16, BP32 = B rounded up
        to 32)."""
        if not self.bf16:
            raise ValueError("factors_bf16: not a bf16 workspace")
        h, dz1, dl, _, dz1h, planes, BP, BP32 = hip().mlp_lbh_offsets(self.B)
        return dict(h=self.buf[h:dz1].view(BP, 112), dz1=self.buf[dz1:dl].view(BP, 112),
                    dl=self.buf[dl:dl + BP * 16].view(BP, 16),
                    dz1h=self.buf[dz1h:planes].view(torch.bfloat16).view(BP32, 112))


def reduce_partials(B):
    """Workgroups of the reduce launch = floats of ``step_grad``'s ``partials`` (78 at every B)."""
    return int(hip().mlp_lb_reduce_partials(int(B)))


def _check_partials(partials, B):
    if partials is None:
        return 0
    if (not torch.is_tensor(partials) or not partials.is_cuda or partials.dtype != torch.float32
            or not partials.is_contiguous() or partials.numel() < reduce_partials(B)):
        raise ValueError("partials must be a contiguous f32 GPU tensor of at least %d floats"
                         % reduce_partials(B))
    return ptr(partials)


def step_grad(p, x, labels, ws: LargeBatchWorkspace, grad, stats=True, activation="sigmoid",
              partials=None):
    """Forward/backward of the batch (x [B,784], labels [B]) at the parameters ``p``, writing the
    flat gradient ``grad``, the step's (loss, accuracy) into ``ws.stats[global_step % ring]`` (with
    ``stats``) and advancing ``ws.ctr``.  ``activation``: ``ops/hidden_act.py``.  ``partials``
    (``reduce_partials(B)`` floats, for ``ops.optim.clip_by_global_norm_(have_partials=True)``):
    the reduce launch also leaves each workgroup's sum of squares of the gradient it stored, what
    ``gnorm_partials`` would compute from ``grad``; ``None`` launches today's reduce.  Returns
    ``p``."""
    if not isinstance(ws, LargeBatchWorkspace) or ws.bf16:
        raise ValueError("the large-batch step needs a LargeBatchWorkspace (bf16=False)")
    mlp_step._check(x, labels, ws.B)
    mlp_step._check_flat(p, grad)
    if labels is None or not labels.is_cuda:
        raise ValueError("labels must be a contiguous int32 GPU batch of B values")
    if grad.data_ptr() % 16:
        raise ValueError("the gradient buffer must be 16-byte aligned")
    act = hidden_act.act_id(activation)
    pp = _check_partials(partials, ws.B)
    h, s = hip(), stream_handle()
    h.mlp_lb_fwdhead(ptr(p), ptr(x), ptr(labels), ptr(ws.buf), ws.B, act, s)
    h.mlp_lb_wgrad(ptr(x), ptr(ws.buf), ws.B, s)
    h.mlp_lb_reduce(ptr(ws.buf), ptr(grad), ptr(ws.ctr), ptr(ws.stats) if stats else 0,
                    ws.stats_ring, ws.B, s, pp)
    return p


def step_grad_bf16(p, xh, labels, ws: LargeBatchWorkspace, grad, stats=True, activation="sigmoid",
                   partials=None):
    """``step_grad`` with the batch as bf16 rows ``xh`` [B,784] (contiguous, 16-byte aligned) and
    ``ws`` a ``LargeBatchWorkspace(bf16=True)``: bf16 operands and f32 accumulation in the two
    784-wide GEMMs, everything else -- the f32 parameters ``p`` and ``partials`` included -- as
    ``step_grad``."""
    if not isinstance(ws, LargeBatchWorkspace) or not ws.bf16:
        raise ValueError("the bf16 large-batch step needs a LargeBatchWorkspace(bf16=True)")
    if (not torch.is_tensor(xh) or xh.dtype != torch.bfloat16 or not xh.is_cuda
            or tuple(xh.shape) != (ws.B, mlp_step.D) or not xh.is_contiguous()
            or xh.data_ptr() % 16):
        raise ValueError("xh must be a contiguous, 16-byte aligned bf16 GPU batch [%d, %d]"
                         % (ws.B, mlp_step.D))
    if (labels is None or not labels.is_cuda or labels.dtype != torch.int32
            or tuple(labels.shape) != (ws.B,) or not labels.is_contiguous()):
        raise ValueError("labels must be a contiguous int32 GPU batch of B values")
    mlp_step._check_flat(p, grad)
    if grad.data_ptr() % 16:
        raise ValueError("the gradient buffer must be 16-byte aligned")
    act = hidden_act.act_id(activation)
    pp = _check_partials(partials, ws.B)
    h, s = hip(), stream_handle()
    h.mlp_lbh_fwdhead(ptr(p), ptr(xh), ptr(labels), ptr(ws.buf), ws.B, act, s)
    h.mlp_lbh_wgrad(ptr(xh), ptr(ws.buf), ws.B, s)
    h.mlp_lbh_reduce(ptr(ws.buf), ptr(grad), ptr(ws.ctr), ptr(ws.stats) if stats else 0,
                     ws.stats_ring, ws.B, s, pp)
    return p
