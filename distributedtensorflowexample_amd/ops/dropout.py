"""Hidden-layer dropout of the fused MLP step: the definition, on the host.

Inverted dropout on the hidden activation ``h`` [B, 100], with integer decisions only.  This is
a framework extension (the ``tf.layers.dropout`` a user of the MLP path would reach for); the
reference model has no dropout.

* Threshold.  ``rate`` in [0, 1).  ``thr = int(round((1 - rate) * 2**24))``, computed in float64
  on the host; ``thr < 1`` is refused.
* Effective keep probability.  ``q = thr / 2**24``.
* Scale.  ``scale = float32(2**24 / thr)``, passed to the kernels by value.
* Linear index.  Element (row r of the batch, hidden unit j) has linear index ``n = r * 100 + j``.
* Philox word.  The word of that element is word ``n & 3`` of ``philox4x32_10(counter =
  {n >> 2, 0, s, stream}, key = {lo32 seed, hi32 seed})``: ``s`` is the 0-based global_step of the
  step the head belongs to, ``stream`` the replica's rank.  (With the fill kernels' counter
  layout this is ``words(B * 100, seed, (stream << 32) | s)`` flattened.)
* Keep rule.  Keep iff ``(word >> 8) < thr``.
* Forward.  ``hd = keep ? h * scale : 0`` and ``logits = hd . W2 + b2``.  The head's ``hbuf``
  holds ``hd``; its padding stays exactly 0.
* Backward.  ``dz1 = (dl . W2) * (keep ? scale : 0) * h * (1 - h)``, with the undropped ``h``.

The mask is a pure function of (seed, global_step, replica, row, unit), as the shuffle order is
one of (seed, epoch): nothing is baked into a captured graph, a checkpoint carries nothing new,
and ``seek()`` resumes the mask sequence.  The kernels read ``s`` from the device step counter,
which equals the step's own index at every head launch (its only writer is the stats lane of the
launch that records the step before).  The recorded per-step loss and accuracy are training-mode
values; ``evaluate()``, ``snapshot()``, ``ops.mlp_eval`` and the eval job never drop.

``keep_mask`` is that mask on the CPU, from a numpy Philox of this module's own.
"""
from __future__ import annotations

import numpy as np

H = 100  # hidden units: the row pitch of the linear index

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO, _32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def check_rate(rate):
    """``rate`` as a float in [0, 1), else ValueError."""
    r = float(rate)
    if not 0.0 <= r < 1.0:
        raise ValueError("dropout rate must be in [0, 1), got %r" % (rate,))
    return r


def threshold(rate):
    """(thr, scale): the 24-bit keep threshold and the float32 rescale of kept units."""
    r = check_rate(rate)
    thr = int(round((1.0 - np.float64(r)) * 2.0 ** 24))
    if thr < 1:
        raise ValueError("dropout rate %r keeps nothing (threshold below 1 / 2**24)" % (rate,))
    return thr, float(np.float32(2.0 ** 24 / thr))


def _philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over uint64 arrays holding 32-bit counters -> four uint64 arrays."""
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> _32, p0 & _LO, p1 >> _32, p1 & _LO
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def seed_words(seed):
    """(lo32, hi32) of the seed: the Philox key."""
    s = int(seed) & (2 ** 64 - 1)
    return s & 0xFFFFFFFF, s >> 32


def mask_words(seed, step, stream, B):
    """uint32 [B, 100]: the Philox word behind every element of one step's mask."""
    n4 = (int(B) * H + 3) // 4
    i = np.arange(n4, dtype=np.uint64)
    k0, k1 = seed_words(seed)
    z = np.zeros(n4, dtype=np.uint64)
    w = _philox(i, z, z + np.uint64(int(step) & 0xFFFFFFFF),
                z + np.uint64(int(stream) & 0xFFFFFFFF), k0, k1)
    return np.stack(w, axis=-1).reshape(-1)[:int(B) * H].astype(np.uint32).reshape(int(B), H)


def keep_mask(seed, step, stream, B, rate):
    """CPU bool tensor [B, 100]: True where the unit is kept at ``rate``."""
    import torch

    thr, _ = threshold(rate)
    return torch.from_numpy((mask_words(seed, step, stream, B) >> np.uint32(8)) < np.uint32(thr))


class Dropout:
    """The words the launchers take for one (rate, seed, replica): ``args()`` follows the device
    counter's address in ``mlp_head_drop`` / ``mlp_lean_head_drop`` / ``set_drop``."""

    def __init__(self, rate, seed=0, stream=0):
        self.rate = check_rate(rate)
        if self.rate == 0.0:
            raise ValueError("Dropout: rate 0 is no dropout (pass dropout=None to the step)")
        self.seed, self.stream = int(seed), int(stream)
        if not 0 <= self.stream < 2 ** 32:
            raise ValueError("dropout stream (the replica's rank) must fit 32 bits")
        self.thr, self.scale = threshold(self.rate)
        self.k0, self.k1 = seed_words(self.seed)

    def args(self):
        """(k0, k1, thr, stream, scale)"""
        return (self.k0, self.k1, self.thr, self.stream, self.scale)

    def keep_mask(self, step, B):
        return keep_mask(self.seed, step, self.stream, B, self.rate)


def resolve(rate, seed=0, stream=0):
    """``None`` for rate 0 (today's code paths, untouched), else a ``Dropout``."""
    return None if check_rate(rate) == 0.0 else Dropout(rate, seed, stream)


def refuse(flags, what):
    """A trainer without the fused MLP head refuses a non-zero ``--dropout``."""
    if float(getattr(flags, "dropout", 0.0) or 0.0) != 0.0:
        raise ValueError("--dropout: %s has no hidden-layer dropout (the mirrored MLP only)"
                         % what)
