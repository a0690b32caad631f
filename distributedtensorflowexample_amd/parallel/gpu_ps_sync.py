"""Synchronous-replica rounds on the GPU-resident parameter store: the host side.

The device side (``csrc/kernels/gpu_ps.hip``: ``gps_sync_join_kernel`` /
``gps_sync_push_kernel``) never waits on another process.  A push takes a ticket of the open
round on the packed round word ``(round << 32) | tickets_taken``, stores the gradient into the
ticket's slot and returns; the R-th arrival of a chunk sums the slots in ticket order and
applies ``p -= (lr / R) * sum`` (or, with ``--optimizer momentum | adam``, runs that optimizer on
the mean and the chunk's slot planes: ``gpu_ps_optim.py``); the block that completes the last chunk advances
``global_step`` and publishes the next round word.  Every wait is here, on the host:
:class:`SyncRounds` polls the round word until the round it joined has closed.

This module is pure Python / NumPy (no GPU, no native module), so the protocol's host logic is
testable anywhere: :class:`SyncRounds` only needs an object with ``sync_begin`` and
``sync_poll`` (the native ``GpuParamStore``, or a stub).
"""
from __future__ import annotations

import time

import numpy as np

# outcomes of gps_sync_join_kernel (the decision word's status)
JOINED, STALE, AHEAD, LATE, CONTENDED = 0, 1, 2, 3, 4
STATUS_NAMES = {JOINED: "JOINED", STALE: "STALE", AHEAD: "AHEAD", LATE: "LATE",
                CONTENDED: "CONTENDED"}
CHUNK = 1024  # floats per arrival counter (one 256-thread block of float4 accesses)
ROUND_MASK = 0xFFFFFFFF


def pack_round(round_, tickets=0):
    """The 64-bit round word: the round (= global step, 32 bits) above the tickets taken."""
    round_, tickets = int(round_), int(tickets)
    if not 0 <= round_ <= ROUND_MASK:
        raise ValueError("gpu_ps: the sync round is a 32-bit counter, got %d" % round_)
    if not 0 <= tickets <= ROUND_MASK:
        raise ValueError("gpu_ps: bad ticket count %d" % tickets)
    return (round_ << 32) | tickets


def unpack_round(word):
    """-> (round, tickets_taken) of a packed round word."""
    word = int(word) & 0xFFFFFFFFFFFFFFFF
    return word >> 32, word & ROUND_MASK


def num_chunks(n):
    return (int(n) + CHUNK - 1) // CHUNK


def round_reference(p, grads, lr, fma=False):
    """What one closed round leaves in the store, in f32 exactly as the kernel evaluates it:
    ``s = ((g[0] + g[1]) + ...)`` in ticket order, ``p - (lr / R) * s`` with ``lr / R``
    rounded to f32 first.  ``fma=False``: product and difference rounded separately
    (``np.float32`` arithmetic); ``fma=True``: the product feeds the subtraction unrounded
    (a fused multiply-add), emulated in float64 -- exact there, since the product of two f32
    values has at most 48 significant bits -- and rounded once, up to float64's own rounding
    of the final difference (double rounding needs a 29-bit run of zeros or ones and does not
    occur for the test data)."""
    p = np.asarray(p, dtype=np.float32)
    gs = [np.asarray(g, dtype=np.float32) for g in grads]
    scale = np.float32(lr) / np.float32(len(gs))
    s = gs[0].copy()
    for g in gs[1:]:
        s = (s + g).astype(np.float32)
    if fma:
        return (p.astype(np.float64) - np.float64(scale) * s.astype(np.float64)).astype(
            np.float32)
    return (p - (scale * s).astype(np.float32)).astype(np.float32)


class SyncRounds:
    """Host protocol of one worker over a raw store ``st`` with

    * ``st.sync_begin(grad_ptr, lr, local_step, stream, extra_ptr, nextra)`` ->
      ``(status, round, ticket, [floats])`` -- join + push enqueued, one read-back, no wait on
      other workers;
    * ``st.sync_poll(stream)`` -> ``(round, tickets_taken)``.

    ``replicas`` is the store's R.  Unlike the TCP parameter server, a push that timed out is
    NOT withdrawn: its slot may already be counted, so the round can still close with it.
    The caller keeps waiting with :meth:`wait`; a second :meth:`push` for a round this worker
    already joined is refused here (on the device it would take a second ticket and count this
    worker twice)."""

    SPIN_POLLS = 64  # polls without yielding the core; later ones yield (sleep(0))

    def __init__(self, st, replicas, stream=lambda: 0, clock=time.monotonic, sleep=time.sleep,
                 hyper=()):
        self.st = st
        self.replicas = int(replicas)
        # a stateful optimizer's hyper-parameter words (gpu_ps_optim.hyper_args), appended to
        # every sync_begin: the round's closer runs the optimizer on the mean gradient
        self.hyper = tuple(float(h) for h in hyper)
        self._stream, self._clock, self._sleep = stream, clock, sleep
        self.joined_round = None  # the last round this worker holds (held) a ticket of
        self.polls = 0  # host polls so far (tools/probes/gpu_ps_sync_cost.py)

    def push(self, grad_ptr, lr, local_step, timeout_s=60.0, extra_ptr=0, nextra=0):
        """-> (step, applied, [floats]).  JOINED: waits until the round closed, (round + 1,
        True).  STALE: at once, (current round, False).  LATE (the round is open but its R
        tickets are taken: a backup replica): waits for the close, (new round, False).
        AHEAD / CONTENDED: RuntimeError.  TimeoutError names the round and ``k of R``."""
        local_step = int(local_step)
        if self.joined_round is not None and local_step == self.joined_round:
            raise RuntimeError("gpu_ps: this worker already pushed a gradient for round %d "
                               "(a timed-out push is not withdrawn: wait for it with "
                               "sync_push_wait)" % local_step)
        status, round_, ticket, vals = self.st.sync_begin(
            int(grad_ptr), float(lr), local_step, self._stream(), int(extra_ptr), int(nextra),
            *self.hyper)
        status, round_ = int(status), int(round_)
        vals = [float(v) for v in vals]
        if status == STALE:
            return round_, False, vals
        if status == AHEAD:
            raise RuntimeError("gpu_ps: local step %d is ahead of the store's round %d"
                               % (local_step, round_))
        if status == CONTENDED:
            raise RuntimeError("gpu_ps: no ticket for round %d after the join's retry bound"
                               % local_step)
        if status == JOINED:
            self.joined_round = local_step
        elif status != LATE:
            raise RuntimeError("gpu_ps: unknown join status %d" % status)
        step = self.wait(local_step, timeout_s)
        return step, status == JOINED, vals

    def wait(self, local_step, timeout_s=60.0):
        """Poll (on the host) until the round ``local_step`` has closed; -> the new global
        step.  TimeoutError after ``timeout_s``; the wait can be repeated."""
        local_step = int(local_step)
        t0 = self._clock()
        k, spins = 0, 0
        while True:
            round_, k = self.st.sync_poll(self._stream())
            self.polls += 1
            if round_ > local_step:
                return int(round_)
            if self._clock() - t0 > timeout_s:
                raise TimeoutError("gpu_ps: sync round %d still open after %.3g s (%d of %d "
                                   "gradients)" % (local_step, timeout_s, k, self.replicas))
            spins += 1
            if spins > self.SPIN_POLLS:
                self._sleep(0)
