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


class LargeBatchWorkspace:
    """Device scratch of the large-batch step for batch size ``B``, with the attributes
    ``FusedMLPTrainer`` uses on ``mlp_step.StepWorkspace``: ``buf`` (zeroed once; its last four
    words are the hand-off words ``check()`` reads), the device ``global_step`` counter ``ctr``
    and the stats ring."""

    def __init__(self, B, device, stats_ring=4096):
        if not MIN_LARGE_BATCH <= B <= MAX_LARGE_BATCH:
            raise ValueError("the large-batch MLP step supports %d <= batch <= %d"
                             % (MIN_LARGE_BATCH, MAX_LARGE_BATCH))
        self.B = int(B)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("the large-batch MLP step runs on the GPU")
        self.buf = torch.zeros(int(hip().mlp_lb_workspace_floats(self.B)), device=device,
                               dtype=torch.float32)
        self.ctr = torch.zeros(1, device=device, dtype=torch.int32)
        self.stats_ring = stats_ring
        self.stats = torch.zeros(stats_ring, 2, device=device, dtype=torch.float32)

    def global_step(self) -> int:
        return int(self.ctr[0].item())

    def set_global_step(self, s: int):
        self.ctr.fill_(int(s))


def step_grad(p, x, labels, ws: LargeBatchWorkspace, grad, stats=True, activation="sigmoid"):
    """Forward/backward of the batch (x [B,784], labels [B]) at the parameters ``p``, writing the
    flat gradient ``grad``, the step's (loss, accuracy) into ``ws.stats[global_step % ring]`` (with
    ``stats``) and advancing ``ws.ctr``.  ``activation``: ``ops/hidden_act.py``.  Returns ``p``."""
    if not isinstance(ws, LargeBatchWorkspace):
        raise ValueError("the large-batch step needs a LargeBatchWorkspace")
    mlp_step._check(x, labels, ws.B)
    mlp_step._check_flat(p, grad)
    if labels is None or not labels.is_cuda:
        raise ValueError("labels must be a contiguous int32 GPU batch of B values")
    if grad.data_ptr() % 16:
        raise ValueError("the gradient buffer must be 16-byte aligned")
    act = hidden_act.act_id(activation)
    h, s = hip(), stream_handle()
    h.mlp_lb_fwdhead(ptr(p), ptr(x), ptr(labels), ptr(ws.buf), ws.B, act, s)
    h.mlp_lb_wgrad(ptr(x), ptr(ws.buf), ws.B, s)
    h.mlp_lb_reduce(ptr(ws.buf), ptr(grad), ptr(ws.ctr), ptr(ws.stats) if stats else 0,
                    ws.stats_ring, ws.B, s)
    return p
