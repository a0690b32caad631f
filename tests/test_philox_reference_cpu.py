"""Self-checks of the numpy Philox4x32-10 reference the GPU initialiser is held to
(tests/philox_reference.py): the Random123 known answers and the helper identities."""
import numpy as np

import philox_reference as PH

# (counter, key, output) of the Random123 known-answer file, philox4x32 with 10 rounds
KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
     [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
]


def test_known_answers():
    for ctr, key, want in KAT:
        got = PH.philox4x32_10(np.array(ctr, dtype=np.uint32), key)
        assert [int(x) for x in got] == want
    # batched: the three counters under the third key, row by row
    ctrs = np.array([k[0] for k in KAT], dtype=np.uint32)
    got = PH.philox4x32_10(ctrs, KAT[2][1])
    assert [int(x) for x in got[2]] == KAT[2][2]
    assert [int(x) for x in got[0]] != KAT[0][2]


def test_counter_layout():
    """words(): counter {lo32 i, hi32 i, lo32 offset + round, hi32 offset}, key {lo32 seed,
    hi32 seed}."""
    assert [int(x) for x in PH.words(4, 0, 0)[0]] == KAT[0][2]
    seed, offset = (0x299F31D0 << 32) | 0xA4093822, (0x03707344 << 32) | (0x13198A2E - 3)
    got = PH.philox4x32_10(np.array([5, 0, (offset + 3) & 0xFFFFFFFF, offset >> 32],
                                    dtype=np.uint32), (seed & 0xFFFFFFFF, seed >> 32))
    assert np.array_equal(PH.words(24, seed, offset, rnd=3)[5], got)
    # the low offset word wraps on its own: no carry into the high word
    a = PH.words(4, 1, 0xFFFFFFFF, rnd=1)[0]
    b = PH.philox4x32_10(np.array([0, 0, 0, 0], dtype=np.uint32), (1, 0))
    assert np.array_equal(a, b)


def test_uniform_inverse_is_exact_in_float32():
    """1 - u01(x) computed in float32 (as the kernel does) gives back x >> 8 exactly."""
    rng = np.random.default_rng(0)
    x = rng.integers(0, 2 ** 32, size=100000, dtype=np.uint64).astype(np.uint32)
    x[:4] = [0, 0xFF, 0xFFFFFF00, 0xFFFFFFFF]
    u = ((x >> np.uint32(8)).astype(np.float32) + np.float32(1)) * np.float32(1.0 / 16777216.0)
    v = np.float32(0) + (np.float32(1) - np.float32(0)) * (np.float32(1) - u)
    assert v.dtype == np.float32 and v.min() >= 0 and v.max() < 1
    assert np.array_equal(PH.top24_from_uniform(v), (x >> np.uint32(8)).astype(np.int64))


def test_normal_reference_moments():
    z = PH.std_normal(1 << 18, 7, 0)
    assert np.isfinite(z).all()
    assert abs(z.mean()) < 1e-2 and abs(z.std() - 1) < 1e-2
    # sine and cosine halves of a pair are uncorrelated, and pairs differ
    q = z.reshape(-1, 4)
    assert abs(np.mean(q[:, 0] * q[:, 1])) < 1e-2
    assert not np.allclose(q[:, 0], q[:, 2])


def test_truncated_reference_and_exclusion_cap():
    """The truncated-normal cases of test_philox_gpu: inside +-2 std, and at most 1 % of the
    elements (expected ~1e-4 per round) are left out as too close to the cut."""
    for n, seed, offset, a, b in PH.TRUNC_CASES:
        val, near = PH.truncated_normal(n, seed, offset, a, b)
        assert val.shape == (n,) and np.all(np.abs(val - a) <= 2 * b)
        assert near.mean() <= 0.01
        if n >= 1000:  # std of a standard normal cut at +-2
            assert abs(((val - a) / b).std() - 0.88) < 0.05
