"""The Philox initialiser (ops.init.fill_ on the GPU) against a plain numpy Philox4x32-10
(tests/philox_reference.py, itself checked against the Random123 known answers on the CPU):
replicas skip the parameter broadcast and checkpoints assume the same values across builds, so
the counter layout, the word order, the tail and the offset streams are pinned bit for bit."""
import numpy as np
import pytest
import torch

import philox_reference as PH
from distributedtensorflowexample_amd.ops import init

pytestmark = pytest.mark.gpu

N_WRAP = 2048 * 256 * 4 + 7  # a full pass of the capped grid, one more float4, a 3-element tail
SIZES = [1, 2, 3, 4, 5, 1027, N_WRAP]
SEEDS = [0, 1234, (1 << 40) + 7]
OFFSETS = [0, 1, 1 << 40, (3 << 40) + 5]
GUARD, POISON = 64, -7.0


def _fill(gpu, n, kind, a, b, seed, offset):
    """fill_ of the first n elements of a poisoned buffer; checks the guard behind them."""
    buf = torch.full((n + GUARD,), POISON, device=gpu)
    init.fill_(buf[:n], kind, a, b, seed=seed, offset=offset)
    out = buf.cpu().numpy()
    assert np.all(out[n:] == POISON), "wrote past the n-th element"
    return out[:n]


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", SIZES)
def test_uniform_words_exact(gpu, n, seed, offset):
    v = _fill(gpu, n, "uniform", 0.0, 1.0, seed, offset)
    assert v.min() >= 0.0 and v.max() < 1.0
    assert np.array_equal(PH.top24_from_uniform(v), PH.top24(n, seed, offset))


def test_first_known_answer(gpu):
    """Seed 0, offset 0, elements 0..3: the all-zero counter and key of Random123."""
    v = _fill(gpu, 4, "uniform", 0.0, 1.0, 0, 0)
    want = [x >> 8 for x in (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)]
    assert PH.top24_from_uniform(v).tolist() == want


def test_uniform_range(gpu):
    """a + (b - a)(1 - u01) at a range that is not [0, 1): half a float32 ulp of the range."""
    n, a, b = 1027, -1.0, 2.0
    v = _fill(gpu, n, "uniform", a, b, 5, 9)
    want = a + (b - a) * (1.0 - (PH.top24(n, 5, 9) + 1.0) / 16777216.0)
    assert np.abs(v - want).max() <= 2.0 ** -23 * 2.0
    assert v.min() >= a and v.max() < b


@pytest.mark.parametrize("n", [5, 4099])
@pytest.mark.parametrize("seed,offset", [(7, 0), ((1 << 40) + 7, (3 << 40) + 5)])
def test_normal_matches_box_muller(gpu, n, seed, offset):
    """Bound 1e-4 * std: the fast log / sin / cos are at the 1e-6 level, every layout mistake
    (sine and cosine swapped, wrong word, wrong pair) is O(1)."""
    mean, std = 0.5, 2.0
    v = _fill(gpu, n, "normal", mean, std, seed, offset)
    assert np.isfinite(v).all()
    assert np.abs(v - PH.normal(n, seed, offset, mean, std)).max() <= 1e-4 * std


@pytest.mark.parametrize("n,seed,offset,a,b", PH.TRUNC_CASES)
def test_truncated_normal(gpu, n, seed, offset, a, b):
    v = _fill(gpu, n, "truncated_normal", a, b, seed, offset)
    assert np.isfinite(v).all()
    assert np.all(np.abs(v.astype(np.float64) - a) <= 2 * b)
    want, near = PH.truncated_normal(n, seed, offset, a, b)
    assert near.mean() <= 0.01
    assert np.abs(v - want)[~near].max() <= 1e-4 * b


def test_model_offset_streams(gpu):
    """models/*.py give tensor i the offset i << 40: four fills match the reference and share no
    value position for position."""
    n, seed = 1027, 11
    got = [PH.top24_from_uniform(_fill(gpu, n, "uniform", 0.0, 1.0, seed, i << 40))
           for i in range(4)]
    for i in range(4):
        assert np.array_equal(got[i], PH.top24(n, seed, i << 40)), i
        for j in range(i):
            assert not np.any(got[i] == got[j]), (i, j)


def test_fill_restarts_at_counter_zero(gpu):
    """Two fills into one buffer, split where the second starts off a float4 boundary: each
    matches the reference for its own (n, offset), whatever its address."""
    k, n = 1030, 2053
    buf = torch.full((n + GUARD,), POISON, device=gpu)
    init.fill_(buf[:k], "uniform", 0.0, 1.0, seed=3, offset=0)
    init.fill_(buf[k:n], "uniform", 0.0, 1.0, seed=3, offset=1 << 40)
    out = buf.cpu().numpy()
    assert np.all(out[n:] == POISON)
    assert np.array_equal(PH.top24_from_uniform(out[:k]), PH.top24(k, 3, 0))
    assert np.array_equal(PH.top24_from_uniform(out[k:n]), PH.top24(n - k, 3, 1 << 40))
