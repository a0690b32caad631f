"""Fused evaluation of the reference MNIST MLP (784 -> 100 sigmoid -> 10).

Python side of ``csrc/kernels/mlp_eval.hip``: ONE launch runs ``n`` rows through the network
and leaves predictions, class probabilities (the reference's ``self.net``), the summed
softmax cross-entropy, the number of correct rows and a 10 x 10 confusion matrix -- the
reference's 10,000-image test evaluation (worker.py:87-90,150-154) plus the test loss it
never computed.  The hidden activations and the logits never reach global memory.

The device accumulator is integer throughout (the loss sum in 64-bit fixed point, 2^-32
units), so it is bitwise reproducible; the launcher zeroes it on the stream ahead of the
kernel.  ``EvalResult`` reads it back lazily, once: an evaluation can be queued between two
graph replays, or captured into a graph with a reused ``acc=``, and read later.

Rows whose label is outside ``[0, 10)`` still get a prediction and probabilities and are
counted in nothing (mask rows with ``-1``).  The arg-max is the lowest class whose logit
equals the maximum (``tf.argmax``).  CPU tensors take the same function through
``mlp_step.reference_forward``.

``activation=`` (``ops/hidden_act.py``: sigmoid, the reference's and the default, relu, tanh)
selects the hidden activation on both paths: one kernel instantiation each.  A checkpoint does not
record it, so the caller names the one the parameters were trained with.
"""
from __future__ import annotations

import torch

from . import hidden_act, mlp_step
from ._ext import hip, ptr, stream_handle

D, H, C = mlp_step.D, mlp_step.H, mlp_step.C
# accumulator block as int32 words: [0:2] loss sum (int64, 2^-32 units), [2] correct,
# [3] count, [4:104] confusion [label][predicted] -- csrc/kernels/mlp_eval.hip, EvalAcc
ACC_WORDS = 4 + C * C
LOSS_SCALE = 2.0 ** 32
# a row's loss enters the sum clamped to [0, LOSS_CAP] (a NaN loss as LOSS_CAP)
LOSS_CAP = 1024.0


def acc_words():
    """int32 words of the device accumulator block (the kernel module's own size)."""
    n = int(hip().mlp_eval_acc_bytes())
    if n != 4 * ACC_WORDS:
        raise RuntimeError("mlp_eval accumulator layout mismatch: %d bytes" % n)
    return ACC_WORDS


def new_acc(device):
    """A fresh accumulator block (every labelled ``evaluate`` zeroes it on the stream)."""
    if torch.device(device).type == "cuda":
        acc_words()
    return torch.zeros(ACC_WORDS, dtype=torch.int32, device=device)


class EvalResult:
    """Result of :func:`evaluate`: the accumulator block ``acc`` (int32 [104], on the
    input's device; ``None`` for a predict-only call) and the optional ``pred`` (int32 [n])
    / ``probs`` (f32 [n, 10]) tensors.  ``loss`` (mean over the counted rows), ``accuracy``,
    ``count``, ``correct`` and ``confusion`` ([label][predicted], int64 CPU tensor) are lazy:
    the first of them reads the accumulator back (one D2H copy, which waits for the
    evaluation), the others reuse that copy."""

    def __init__(self, acc, pred=None, probs=None):
        self.acc, self.pred, self.probs = acc, pred, probs
        self._host = None

    def _read(self):
        if self.acc is None:
            raise ValueError("a predict-only evaluation (labels=None) has no accumulator")
        if self._host is None:
            self._host = self.acc.detach().to("cpu").clone()
        return self._host

    @property
    def loss_sum(self) -> float:
        return int(self._read()[:2].view(torch.int64)[0]) / LOSS_SCALE

    @property
    def correct(self) -> int:
        return int(self._read()[2])

    @property
    def count(self) -> int:
        return int(self._read()[3])

    @property
    def loss(self) -> float:
        n = self.count
        return self.loss_sum / n if n else float("nan")

    @property
    def accuracy(self) -> float:
        n = self.count
        return self.correct / n if n else float("nan")

    @property
    def confusion(self):
        return self._read()[4:4 + C * C].view(C, C).to(torch.int64)


def _check(params, x, labels, acc):
    if x.dim() != 2 or x.shape[1] != D:
        raise ValueError("x must be [n, 784]")
    n = x.shape[0]
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("x must be a contiguous f32 [n, 784] matrix")
    if x.data_ptr() % 16:
        raise ValueError("x must be 16-byte aligned")
    if (params.numel() != mlp_step.NPARAM or params.dtype != torch.float32
            or not params.is_contiguous() or params.device != x.device):
        raise ValueError("params must be the contiguous f32 [79510] buffer on x's device")
    if params.data_ptr() % 16:
        raise ValueError("params must be 16-byte aligned")
    if labels is not None and (labels.dtype != torch.int32 or labels.numel() != n
                               or not labels.is_contiguous() or labels.device != x.device):
        raise ValueError("labels must be a contiguous int32 vector of n values on x's device")
    if acc is not None and (acc.dtype != torch.int32 or acc.numel() != ACC_WORDS
                            or not acc.is_contiguous() or acc.device != x.device
                            or acc.data_ptr() % 8):
        raise ValueError("acc must be a contiguous int32 [%d] block on x's device" % ACC_WORDS)
    return n


def _evaluate_cpu(params, x, labels, predictions, probs, acc, activation="sigmoid"):
    _, logits = mlp_step.reference_forward(params, x, activation)
    # lowest class whose logit equals the maximum (tf.argmax), whatever torch's tie rule
    m = logits.max(1, keepdim=True).values
    cls = torch.arange(C).expand_as(logits)
    pred = torch.where(logits == m, cls, torch.full_like(cls, C)).min(1).values
    pred = torch.where(pred < C, pred, torch.zeros_like(pred)).to(torch.int32)
    out_probs = torch.softmax(logits, 1) if probs else None
    if labels is None:
        return EvalResult(None, pred if predictions else None, out_probs)
    lab = labels.long()
    keep = (lab >= 0) & (lab < C)
    lk, pk = lab[keep], pred[keep].long()
    row = torch.logsumexp(logits[keep], 1) - logits[keep].gather(1, lk[:, None])[:, 0]
    row = torch.where(row >= 0, row, torch.where(row < 0, torch.zeros_like(row),
                                                 torch.full_like(row, LOSS_CAP)))
    row = row.clamp(max=LOSS_CAP)
    if acc is None:
        acc = new_acc("cpu")
    acc.zero_()
    acc[:2].view(torch.int64)[0] = int(torch.round(row.double().sum() * LOSS_SCALE))
    acc[2] = int((lk == pk).sum())
    acc[3] = int(keep.sum())
    acc[4:].copy_(torch.bincount(lk * C + pk, minlength=C * C).to(torch.int32))
    return EvalResult(acc, pred if predictions else None, out_probs)


def evaluate(params, x, labels=None, *, predictions=False, probs=False, acc=None,
             activation="sigmoid"):
    """Evaluate the flat parameter buffer ``params`` on ``x`` [n, 784] (f32).

    ``labels`` (int32 [n]): loss, accuracy, counts and the confusion matrix are accumulated
    over the rows whose label is in ``[0, 10)``; ``None``: predict only, no accumulator is
    written.  ``predictions`` / ``probs``: also return the predicted classes (int32 [n]) /
    the class probabilities (f32 [n, 10]).  ``acc``: reuse this accumulator block
    (:func:`new_acc`) instead of allocating one -- under graph capture, so that every replay
    zeroes and fills the same block.  ``activation``: the model's hidden activation
    (``sigmoid`` | ``relu`` | ``tanh``).

    GPU tensors: one memset node and one kernel on the current stream, no host
    synchronisation.  CPU tensors: the same result through ``mlp_step.reference_forward``.
    """
    act = hidden_act.act_id(activation)
    n = _check(params, x, labels, acc)
    if labels is None:  # predict only: the accumulator (a caller's included) is not touched
        acc = None
        predictions = predictions or not probs
    if not x.is_cuda:
        return _evaluate_cpu(params, x, labels, predictions, probs, acc, activation)
    h = hip()
    if n > h.mlp_eval_max_rows():
        raise ValueError("mlp_eval: at most %d rows per call" % h.mlp_eval_max_rows())
    dev = x.device
    if labels is not None and acc is None:
        acc = torch.empty(acc_words(), dtype=torch.int32, device=dev)
    pred = torch.empty(n, dtype=torch.int32, device=dev) if predictions else None
    pr = torch.empty(n, C, dtype=torch.float32, device=dev) if probs else None
    h.mlp_eval(ptr(params), ptr(x), ptr(labels), n, ptr(acc), ptr(pred), ptr(pr),
               stream_handle(dev), act)
    return EvalResult(acc, pred, pr)


def predict(params, x):
    """Predicted classes (int32 [n]) of ``x`` [n, 784]: the predict-only launch."""
    return evaluate(params, x, None, predictions=True).pred
