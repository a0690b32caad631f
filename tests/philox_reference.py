"""Plain numpy Philox4x32-10 and the float64 form of what ops.init.fill_ promises on the GPU:

element 4i + e is word e of philox(counter = {lo32 i, hi32 i, lo32 offset + round, hi32 offset},
key = {lo32 seed, hi32 seed}); u01(x) = ((x >> 8) + 1) / 2^24; uniform = a + (b - a)(1 - u01);
normal = Box-Muller (r0 cos t0, r0 sin t0, r1 cos t1, r1 sin t1) of the four words; truncated
normal = the first of 16 rounds with |z| <= 2, else round 15 clamped to +-2.
"""
import numpy as np

# (n, seed, offset, mean, std) of the truncated-normal GPU cases; the CPU self-check verifies
# the share of elements they leave out
TRUNC_CASES = [(5, 3, 0, 0.5, 2.0), (4099, 3, 0, 0.5, 2.0), (4099, 1234, (2 << 40) + 0xFFFFFFF8,
                                                            0.0, 0.02)]

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: uint32 [..., 4], key: two Python ints (32 bits each) -> uint32 [..., 4]."""
    c0, c1, c2, c3 = (np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4))
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> _32, p0 & _LO, p1 >> _32, p1 & _LO
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def words(n, seed, offset, rnd=0):
    """uint32 [ceil(n / 4), 4]: the four words of every counter a fill of n elements uses."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    i = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.empty((i.size, 4), dtype=np.uint32)
    ctr[:, 0] = (i & _LO).astype(np.uint32)
    ctr[:, 1] = (i >> _32).astype(np.uint32)
    ctr[:, 2] = ((offset & 0xFFFFFFFF) + rnd) & 0xFFFFFFFF
    ctr[:, 3] = offset >> 32
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))


def top24(n, seed, offset):
    """x >> 8 of the word behind each of the n elements (int64 [n])."""
    return (words(n, seed, offset).reshape(-1)[:n] >> np.uint32(8)).astype(np.int64)


def u01(x):
    return ((x >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0


def top24_from_uniform(v):
    """Inverts fill_(t, "uniform", 0, 1): v = 1 - u01(x) is exact in float32, so
    2^24 (1 - v) - 1 is x >> 8."""
    return np.rint(16777216.0 * (1.0 - np.asarray(v, dtype=np.float64)) - 1.0).astype(np.int64)


def std_normal(n, seed, offset, rnd=0):
    """float64 [ceil(n / 4) * 4] standard normals (Box-Muller of the four words), untrimmed."""
    u = u01(words(n, seed, offset, rnd))
    r0, t0 = np.sqrt(-2.0 * np.log(u[:, 0])), 2.0 * np.pi * u[:, 1]
    r1, t1 = np.sqrt(-2.0 * np.log(u[:, 2])), 2.0 * np.pi * u[:, 3]
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)],
                    axis=-1).reshape(-1)


def normal(n, seed, offset, mean, std):
    return mean + std * std_normal(n, seed, offset)[:n]


def truncated_normal(n, seed, offset, mean, std, margin=1e-3):
    """(values float64 [n], near bool [n]).  ``near`` marks the elements with | |z| - 2 | < margin
    in some round up to the accepted one: there a float32 kernel may decide the other way."""
    n4 = (n + 3) // 4 * 4
    z = np.zeros(n4)
    done = np.zeros(n4, dtype=bool)
    near = np.zeros(n4, dtype=bool)
    for rnd in range(16):
        zr = std_normal(n, seed, offset, rnd)
        near |= ~done & (np.abs(np.abs(zr) - 2.0) < margin)
        take = ~done & ((np.abs(zr) <= 2.0) | (rnd == 15))
        z[take] = np.clip(zr[take], -2.0, 2.0)
        done |= take
        if done.all():
            break
    return mean + std * z[:n], near[:n]
