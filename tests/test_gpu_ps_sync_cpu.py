"""Host side of the synchronous-replica rounds on the GPU parameter store (no GPU needed):
the packed round word, the NumPy round reference the GPU tests compare against, the flags,
and the status-to-result mapping of ``sync_push_flat`` driven by a stub store."""
import numpy as np
import pytest

from distributedtensorflowexample_amd import flags as F
from distributedtensorflowexample_amd.parallel import gpu_ps_sync as S


def test_round_word_pack_unpack():
    assert S.pack_round(0) == 0
    assert S.pack_round(1) == 1 << 32
    assert S.pack_round(7, 3) == (7 << 32) | 3
    for r, k in ((0, 0), (1, 0), (1000, 2), (2 ** 32 - 1, 2 ** 32 - 1), (2 ** 31, 1)):
        assert S.unpack_round(S.pack_round(r, k)) == (r, k)
    # taking a ticket is word + 1; closing a round is ((round + 1) << 32)
    assert S.unpack_round(S.pack_round(5, 1) + 1) == (5, 2)
    # the word as a signed 64-bit read (round >= 2^31) unpacks the same
    w = S.pack_round(2 ** 31 + 5, 4)
    assert S.unpack_round(w - (1 << 64)) == (2 ** 31 + 5, 4)
    for bad in ((-1, 0), (2 ** 32, 0), (0, -1), (0, 2 ** 32)):
        with pytest.raises(ValueError):
            S.pack_round(*bad)
    assert [S.num_chunks(n) for n in (1, 1023, 1024, 1025, 79510)] == [1, 1, 1, 2, 78]


def test_round_reference_exact_and_order():
    # integer data, lr / R a power of two: exact, with and without a fused multiply-add
    p = np.arange(-8, 8, dtype=np.float32)
    gs = [np.full(16, k + 1, np.float32) for k in range(4)]
    want = p - 0.25 * 10
    for fma in (False, True):
        out = S.round_reference(p, gs, 1.0, fma=fma)
        assert out.dtype == np.float32 and np.array_equal(out, want)
    assert np.array_equal(S.round_reference(p, gs[:1], 0.5), p - 0.5)
    # the sum is taken in ticket order, in f32: (1e8 + 1) - 1e8 loses the 1, 1e8 - 1e8 + 1 keeps it
    a, b, c = (np.array([v], np.float32) for v in (1e8, 1.0, -1e8))
    z = np.zeros(1, np.float32)
    assert S.round_reference(z, [a, b, c], 3.0)[0] == 0.0
    assert S.round_reference(z, [a, c, b], 3.0)[0] == -1.0
    # lr / R is rounded to f32 before the product (0.1 / 3 is not representable)
    g = np.array([3.0], np.float32)
    s = np.float32(0.1) / np.float32(3)
    assert S.round_reference(z, [g, g, g], 0.1)[0] == np.float32(0) - s * np.float32(9)
    # a fused multiply-add rounds once: differs from the two-rounding result somewhere
    rng = np.random.default_rng(0)
    p = rng.standard_normal(4096).astype(np.float32)
    gs = [rng.standard_normal(4096).astype(np.float32) for _ in range(3)]
    # (lr / R = 0.1f, not a power of two: the product is inexact in f32)
    a, b = S.round_reference(p, gs, 0.3), S.round_reference(p, gs, 0.3, fma=True)
    scale = np.float64(np.float32(0.3) / np.float32(3))
    exact = p.astype(np.float64) - scale * ((gs[0] + gs[1]) + gs[2]).astype(np.float64)
    assert not np.array_equal(a, b)
    assert np.abs(b - exact).max() <= np.abs(a - exact).max()
    assert np.all(np.abs(b - exact) <= np.spacing(np.abs(b)) / 2 * (1 + 2.0 ** -20))


def test_flags_gpu_store_with_sync_replicas():
    fv = F.FlagValues()
    F.define_reference_flags(fv)
    fv(["main.py", "--job_name", "worker", "--ps_device", "gpu", "--sync_replicas",
        "--replicas_to_aggregate", "2"])
    assert fv.ps_device == "gpu" and fv.sync_replicas is True and fv.replicas_to_aggregate == 2
    fv.reset()
    fv(["main.py", "--ps_device=gpu", "--sync_replicas"])
    assert fv.sync_replicas is True and fv.replicas_to_aggregate == 0  # 0: --num_workers


class _StubStore:
    """sync_begin answers from a script; sync_poll walks through a list of (round, tickets)."""

    def __init__(self, begin, polls=()):
        self.begin, self.polls = begin, list(polls)
        self.begun, self.n_polls = [], 0

    def sync_begin(self, grad, lr, local_step, stream, extra, nextra):
        self.begun.append((grad, lr, local_step, stream, extra, nextra))
        return self.begin

    def sync_poll(self, stream):
        self.n_polls += 1
        return self.polls.pop(0) if len(self.polls) > 1 else self.polls[0]


class _Clock:
    def __init__(self, tick=0.01):
        self.t, self.tick, self.sleeps = 0.0, tick, []

    def __call__(self):
        self.t += self.tick
        return self.t

    def sleep(self, s):
        self.sleeps.append(s)


def _rounds(st, R=2, clock=None):
    clock = clock or _Clock()
    return S.SyncRounds(st, R, stream=lambda: 77, clock=clock, sleep=clock.sleep), clock


def test_sync_push_status_mapping():
    # JOINED: polls until the round word moved past local_step
    st = _StubStore((S.JOINED, 4, 1, [0.5, 0.25]), [(4, 2), (4, 2), (5, 0)])
    r, _ = _rounds(st)
    assert r.push(1234, 0.1, 4, 10.0, 99, 2) == (5, True, [0.5, 0.25])
    assert st.begun == [(1234, 0.1, 4, 77, 99, 2)] and st.n_polls == 3 and r.polls == 3
    assert r.joined_round == 4
    # a second begin for the round this worker joined is refused before touching the store
    with pytest.raises(RuntimeError, match="already pushed"):
        r.push(1234, 0.1, 4)
    assert len(st.begun) == 1
    # STALE: at once, no poll, the current round, not applied
    st = _StubStore((S.STALE, 9, 0, []), [(9, 0)])
    r, _ = _rounds(st)
    assert r.push(1, 0.1, 7) == (9, False, []) and st.n_polls == 0 and r.joined_round is None
    # LATE (a backup replica: the round is open, its tickets are taken): waits for the close
    st = _StubStore((S.LATE, 3, 2, [1.0]), [(3, 2), (4, 0)])
    r, _ = _rounds(st)
    assert r.push(1, 0.1, 3) == (4, False, [1.0]) and st.n_polls == 2
    assert r.joined_round is None
    # AHEAD and CONTENDED are errors
    for status in (S.AHEAD, S.CONTENDED):
        r, _ = _rounds(_StubStore((status, 2, 0, []), [(2, 0)]))
        with pytest.raises(RuntimeError):
            r.push(1, 0.1, 5)
    # the round may have advanced by more than one by the time the poll runs
    st = _StubStore((S.JOINED, 4, 0, []), [(7, 1)])
    assert _rounds(st)[0].push(1, 0.1, 4)[:2] == (7, True)


def test_sync_push_timeout_is_not_a_withdrawal():
    st = _StubStore((S.JOINED, 4, 0, []), [(4, 1)])
    r, clock = _rounds(st, R=2)
    with pytest.raises(TimeoutError, match=r"round 4 .*1 of 2"):
        r.push(1, 0.1, 4, timeout_s=0.3)
    assert r.joined_round == 4  # the slot may be counted: still joined
    with pytest.raises(RuntimeError, match="already pushed"):
        r.push(1, 0.1, 4)
    with pytest.raises(TimeoutError, match=r"1 of 2"):
        r.wait(4, timeout_s=0.1)
    st.polls = [(4, 2), (5, 0)]
    assert r.wait(4, timeout_s=1.0) == 5


def test_poll_spins_first_then_yields():
    n = S.SyncRounds.SPIN_POLLS
    st = _StubStore((S.JOINED, 0, 0, []), [(0, 1)] * (n + 10) + [(1, 0)])
    r, clock = _rounds(st, clock=_Clock(tick=1e-6))
    assert r.push(1, 0.1, 0)[0] == 1
    assert st.n_polls == n + 11
    assert clock.sleeps == [0] * 10  # none in the first SPIN_POLLS polls; later ones yield only
