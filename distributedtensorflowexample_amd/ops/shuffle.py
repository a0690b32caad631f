"""Per-epoch reshuffle of a resident dataset: a stateless permutation and its gather.

The reference's hot loop draws ``mnist.train.next_batch(100)`` (worker.py:133): TF's
``DataSet.next_batch`` reshuffles the training set at every epoch boundary, the first epoch
included.  ``shuffle_index(seed, epoch, n)[j]`` is the original row that lands at position
``j`` in that epoch -- a pure function of its arguments (no permutation array is kept, no sort
runs, no RNG state exists), so a run resumed at global step ``s`` reproduces the order
(``epoch = s // nbatches``), every data-parallel rank computes the same order without
communicating, and the factor engines can shuffle every rank's stream locally.

Construction: a balanced 4-round Feistel network over ``2k`` bits, ``k = ceil(max(bitlen(n -
1), 2) / 2)``; round function murmur3 ``fmix32`` of ``R ^ key_r`` masked to ``k`` bits; round
keys ``fmix32`` of (seed, epoch, r); cycle-walking into ``[0, n)`` (the network is re-applied
while the value is ``>= n``; the walk ends because the start value lies on the cycle).  Only
32-bit unsigned arithmetic, so this numpy form and the ``__device__`` form in
``csrc/kernels/shuffle.hip`` agree bit for bit.  The function is frozen: changing it changes
the batch order of every resumed run (tests/test_shuffle_cpu.py pins values).

``shuffle_rows_`` is the gather ``dst[w, j] = src[w, shuffle_index(...)[j]]`` over ``W`` planes
of ``[n, 784]`` f32 plus the int32 labels: one HIP launch on the GPU, the explicit index
expression on CPU tensors.
"""
from __future__ import annotations

import numpy as np
import torch

from ._ext import hip, ptr, stream_handle

D = 784
_M32 = 0xFFFFFFFF


def _fmix32(h):
    """murmur3's 32-bit finaliser on a uint32 array (wrapping arithmetic)."""
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def _round_keys(seed, epoch):
    s = np.array([(int(seed) & _M32) ^ 0x9E3779B9], dtype=np.uint32)
    base = _fmix32(_fmix32(s) + np.uint32(int(epoch) & _M32))
    return _fmix32(base + np.arange(1, 5, dtype=np.uint32))


def shuffle_index(seed, epoch, n):
    """int64 [n]: the original row at each position of epoch ``epoch`` (a bijection of [0, n))."""
    n = int(n)
    if not 1 <= n < 2 ** 31:
        raise ValueError("shuffle_index: 1 <= n < 2^31")
    k = np.uint32((max((n - 1).bit_length(), 2) + 1) // 2)
    mask = np.uint32((1 << int(k)) - 1)
    keys = _round_keys(seed, epoch)
    v = np.arange(n, dtype=np.uint32)
    todo = np.arange(n)  # positions still walking
    while todo.size:
        w = v[todo]
        L, R = w >> k, w & mask
        for r in range(4):
            L, R = R, L ^ (_fmix32(R ^ keys[r]) & mask)
        w = (L << k) | R
        v[todo] = w
        todo = todo[w >= n]
    return torch.from_numpy(v.astype(np.int64))


def _planes(t, name):
    """(planes, n, plane stride in floats) of a [n, 784] or [W, n, 784] f32 tensor whose rows
    are dense (a plane stride larger than n * 784 is fine: a slice of a bigger allocation)."""
    if t.dtype != torch.float32 or t.dim() not in (2, 3) or t.shape[-1] != D:
        raise ValueError("%s must be f32 [n, 784] or [W, n, 784]" % name)
    if t.stride(-1) != 1 or t.stride(-2) != D:
        raise ValueError("%s rows must be dense (row stride 784)" % name)
    if t.dim() == 2:
        return 1, t.shape[0], t.shape[0] * D
    return t.shape[0], t.shape[1], (t.stride(0) if t.shape[0] > 1 else t.shape[1] * D)


def _extent(t):
    """[first, last) byte addresses a dense-row tensor spans."""
    span = sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1
    return t.data_ptr(), t.data_ptr() + span * t.element_size()


def shuffle_rows_(dst_x, dst_y, src_x, src_y, seed, epoch):
    """``dst_x[..., j, :] = src_x[..., perm[j], :]`` and ``dst_y[j] = src_y[perm[j]]`` with
    ``perm = shuffle_index(seed, epoch, n)``.  ``dst_y`` / ``src_y`` (int32 [n]) may both be
    None.  ``dst`` and ``src`` must not overlap (raises)."""
    W, n, dstride = _planes(dst_x, "dst_x")
    Ws, ns, sstride = _planes(src_x, "src_x")
    if (W, n) != (Ws, ns) or dst_x.device != src_x.device:
        raise ValueError("dst_x and src_x must have the same shape and device")
    if (dst_y is None) != (src_y is None):
        raise ValueError("both label tensors or neither")
    for y in (dst_y, src_y):
        if y is not None and (y.dtype != torch.int32 or y.shape != (n,) or not y.is_contiguous()
                              or y.device != src_x.device):
            raise ValueError("labels must be contiguous int32 [n] on the data's device")
    if n < 1:
        raise ValueError("empty dataset")
    if not src_x.is_cuda:
        for d, s in ((dst_x, src_x), (dst_y, src_y)):
            if d is not None and _extent(d)[0] < _extent(s)[1] and _extent(s)[0] < _extent(d)[1]:
                raise RuntimeError("shuffle_rows: dst and src overlap")
        idx = shuffle_index(seed, epoch, n)
        with torch.no_grad():
            dst_x.copy_(src_x.index_select(src_x.dim() - 2, idx))
            if dst_y is not None:
                dst_y.copy_(src_y[idx])
        return dst_x
    hip().shuffle_rows(ptr(dst_x), ptr(src_x), ptr(dst_y), ptr(src_y), n, W, dstride, sstride,
                       int(seed) & _M32, int(epoch) & _M32, stream_handle())
    return dst_x
