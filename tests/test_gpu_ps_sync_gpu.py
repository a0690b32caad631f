"""Synchronous replicas on the GPU-resident parameter store (``--ps_device gpu
--sync_replicas``): the round protocol of csrc/kernels/gpu_ps.hip on the raw store (several
logical workers are sequential ``sync_begin`` calls on one owner store, so the ticket order
is known), ``GpuPSStore``'s host protocol, and two worker processes sharing GPU 0."""
import types
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEP = "global/global_step"
SIZES = [1, 3, 1023, 1024, 1025, 4099, 79510]  # lone tail, chunk edge, multi-chunk tail, real
PAIRS = [(1, 0.5), (2, 0.5), (3, 0.75), (4, 1.0)]  # lr / R is a power of two


def _S():
    from distributedtensorflowexample_amd.parallel import gpu_ps_sync

    return gpu_ps_sync


def _stream():
    from distributedtensorflowexample_amd.ops._ext import stream_handle

    return stream_handle("cuda:0")


def _raw(n, R):
    from distributedtensorflowexample_amd.ops import hip

    return hip().GpuParamStore(0, n, True, R)


def _write(st, off, a):
    a = np.ascontiguousarray(a)
    st.write(a.ctypes.data, off, a.nbytes)


def _read(st, off, count, dtype=np.float32):
    a = np.empty(count, dtype=dtype)
    st.read(a.ctypes.data, off, a.nbytes)
    return a


def _snapshot(st, R):
    """Every byte the store uses: parameters, control block, sync region, the R slots."""
    return _read(st, 0, st.slot_offset(R - 1) + st.ctrl_offset(), np.uint8)


def _counters(st, n):
    """(round, tickets_taken, chunks_done, R, arrivals[]) of the sync control region."""
    S = _S()
    w = _read(st, st.sync_offset(), 4 + S.num_chunks(n), np.uint32)
    return int(w[1]), int(w[0]), int(w[2]), int(w[3]), w[4:].tolist()


def _begin(st, g, lr, step):
    status, rnd, ticket, _ = st.sync_begin(g.data_ptr(), lr, step, _stream(), 0, 0)
    return status, rnd, ticket


def _int_grad(n, k, rnd):
    """Integers in [-8, 8], distinct per worker, per round and per element."""
    i = np.arange(n, dtype=np.int64)
    return ((i * 7 + k * 3 + rnd * 5) % 17 - 8).astype(np.float32)


def _int_params(n):
    return ((np.arange(n, dtype=np.int64) * 37) % 129 - 64).astype(np.float32)


@pytest.mark.parametrize("R,lr", PAIRS)
@pytest.mark.parametrize("n", SIZES)
def test_exact_rounds(gpu, n, R, lr):
    """Integer parameters and gradients, lr / R a power of two: every sum and product is
    exact in f32, so three consecutive rounds (counter resets, slot reuse) equal the NumPy
    reference bitwise whatever the FMA contraction."""
    import torch

    S = _S()
    st = _raw(n, R)
    try:
        assert st.sync_slots() == R and _counters(st, n) == (0, 0, 0, R, [0] * S.num_chunks(n))
        p = _int_params(n)
        _write(st, 0, p)
        for rnd in range(3):
            gs = [_int_grad(n, k, rnd) for k in range(R)]
            for k in range(R):
                assert st.sync_poll(_stream()) == (rnd, k)
                assert st.fetch_add(0, 0, _stream()) == rnd  # global_step moves with the close
                g = torch.from_numpy(gs[k]).to(gpu)
                assert _begin(st, g, lr, rnd) == (S.JOINED, rnd, k)
            want = S.round_reference(p, gs, lr)
            assert np.array_equal(want, S.round_reference(p, gs, lr, fma=True))  # exact data
            p = want
            assert np.array_equal(_read(st, 0, n), p)
            assert st.sync_poll(_stream()) == (rnd + 1, 0)
            assert st.fetch_add(0, 0, _stream()) == rnd + 1
            assert _counters(st, n) == (rnd + 1, 0, 0, R, [0] * S.num_chunks(n))
            for k in range(R):  # each slot holds its ticket's gradient
                assert np.array_equal(_read(st, st.slot_offset(k), n), gs[k])
        if st.ctrl_offset() > n * 4:  # the padding behind the parameters was never written
            pad = _read(st, n * 4, st.ctrl_offset() - n * 4, np.uint8)
            assert not pad.any()
    finally:
        st.close()


def test_ticket_order_sum(gpu):
    """Random f32 gradients of mixed magnitude: the result is the f32 evaluation
    p - 0.25 * ((g0 + g1) + g2) in ticket order, bitwise -- with the product rounded (NumPy
    f32 arithmetic) or fused into the subtraction (float64 emulation, rounded once); and
    within the three roundings' bound of the float64 value."""
    import torch

    S = _S()
    n, R, lr = 4099, 3, 0.75
    rng = np.random.default_rng(7)
    p = rng.standard_normal(n).astype(np.float32)
    gs = [(rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
          for _ in range(R)]
    st = _raw(n, R)
    try:
        _write(st, 0, p)
        for k in range(R):
            assert _begin(st, torch.from_numpy(gs[k]).to(gpu), lr, 0) == (S.JOINED, 0, k)
        out = _read(st, 0, n)
    finally:
        st.close()
    plain, fused = S.round_reference(p, gs, lr), S.round_reference(p, gs, lr, fma=True)
    assert np.all((out == plain) | (out == fused))
    # another summation order is a different f32 result somewhere: the order is tested
    assert not np.array_equal(S.round_reference(p, gs[::-1], lr), plain)
    g64 = [g.astype(np.float64) for g in gs]
    exact = p.astype(np.float64) - 0.25 * (g64[0] + g64[1] + g64[2])
    bound = 2.0 ** -23 * (0.25 * 3 * sum(np.abs(g) for g in g64) + np.abs(p) + np.abs(exact))
    err = np.abs(out.astype(np.float64) - exact)
    print("ticket-order sum: max err / bound = %.3g" % (err / bound).max())
    assert np.all(err <= bound)


def test_statuses(gpu):
    """STALE / AHEAD / LATE change nothing (parameters, slots, counters, global_step); with
    R = 2 a third push of a step is dropped and the parameters are the two-gradient mean."""
    import torch

    S = _S()
    n, R, lr = 1025, 2, 0.5
    st = _raw(n, R)
    try:
        p = _int_params(n)
        _write(st, 0, p)
        gs = [_int_grad(n, k, 0) for k in range(3)]
        dev = [torch.from_numpy(g).to(gpu) for g in gs]
        for k in range(R):
            assert _begin(st, dev[k], lr, 0) == (S.JOINED, 0, k)
        p = S.round_reference(p, gs[:2], lr)
        assert st.sync_poll(_stream()) == (1, 0)
        before = _snapshot(st, R)
        status, rnd, _ = _begin(st, dev[2], lr, 0)  # local_step = round - 1
        assert (status, rnd) == (S.STALE, 1)
        assert np.array_equal(_snapshot(st, R), before)
        status, rnd, _ = _begin(st, dev[2], lr, 2)  # local_step = round + 1
        assert (status, rnd) == (S.AHEAD, 1)
        assert np.array_equal(_snapshot(st, R), before)
        # three pushes of step 1: the third finds the round closed (or full) and is dropped
        for k in range(R):
            assert _begin(st, dev[k], lr, 1) == (S.JOINED, 1, k)
        status, rnd, _ = _begin(st, dev[2], lr, 1)
        assert status in (S.LATE, S.STALE) and rnd == 2
        p = S.round_reference(p, gs[:2], lr)
        assert np.array_equal(_read(st, 0, n), p)
        assert _counters(st, n) == (2, 0, 0, R, [0, 0])
        # a full, still open round (both tickets taken, as a backup replica meets it): LATE
        _write(st, st.sync_offset(), np.array([S.pack_round(2, R)], np.uint64))
        before = _snapshot(st, R)
        assert _begin(st, dev[2], lr, 2) == (S.LATE, 2, R)
        assert np.array_equal(_snapshot(st, R), before)
    finally:
        st.close()


def test_restore_sets_the_round(gpu):
    """global_step set through the store (init / restore / assign) also sets the round word:
    a round at the restored step joins and closes at step + 1; an old step is stale."""
    import torch

    S = _S()
    n = 1025
    st = _raw(n, 1)
    try:
        p = _int_params(n)
        _write(st, 0, p)
        g = _int_grad(n, 0, 0)
        dev = torch.from_numpy(g).to(gpu)
        assert _begin(st, dev, 0.5, 0) == (S.JOINED, 0, 0)
        st.set_step(1000)
        assert st.sync_poll(_stream()) == (1000, 0) and st.fetch_add(0, 0, _stream()) == 1000
        status, rnd, _ = _begin(st, dev, 0.5, 0)
        assert (status, rnd) == (S.STALE, 1000)
        assert _begin(st, dev, 0.5, 1000) == (S.JOINED, 1000, 0)
        assert st.sync_poll(_stream()) == (1001, 0) and st.fetch_add(0, 0, _stream()) == 1001
        assert np.array_equal(_read(st, 0, n), p - g)  # two applies of 0.5 * g
        with pytest.raises(RuntimeError):
            st.set_step(2 ** 32)
    finally:
        st.close()


def test_async_store_unchanged(gpu):
    """sync_slots = 0 (and the three-argument constructor): the same control offset and
    extent, pull / push_apply / fetch_add as before, and no sync entry points."""
    import torch

    from distributedtensorflowexample_amd.ops import hip

    n = 4099
    p = _int_params(n)
    g = torch.from_numpy(_int_grad(n, 0, 0)).to(gpu)
    for args in ((0, n, True), (0, n, True, 0)):
        st = hip().GpuParamStore(*args)
        try:
            assert st.sync_slots() == 0
            assert st.ctrl_offset() == (n * 4 + 255) // 256 * 256
            _write(st, 0, p)
            st.push_apply(g.data_ptr(), 0.5, False, _stream())
            dst = torch.empty(n, device=gpu)
            st.pull(dst.data_ptr(), _stream())
            assert st.fetch_add(0, 3, _stream()) == 0 and st.fetch_add(0, 0, _stream()) == 3
            assert np.array_equal(dst.cpu().numpy(), p - 0.5 * g.cpu().numpy())
            _read(st, st.ctrl_offset(), 32, np.uint64)  # the whole control block, no more
            with pytest.raises(RuntimeError, match="out of range"):
                _read(st, st.ctrl_offset() + 256, 1, np.uint8)
            with pytest.raises(RuntimeError, match="no sync slots"):
                st.sync_begin(g.data_ptr(), 0.5, 0, _stream(), 0, 0)
            with pytest.raises(RuntimeError, match="no sync slots"):
                st.sync_poll(_stream())
        finally:
            st.close()


def _free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tf_values(flat):
    import torch

    from distributedtensorflowexample_amd.parallel.gpu_ps import _tf_from_flat

    return _tf_from_flat(torch.from_numpy(np.ascontiguousarray(flat)))


def test_store_timeout_without_a_hang(gpu):
    """GpuPSStore on a one-process cluster with sync_replicas = 2: a lone push times out
    naming 1 of 2 and is NOT withdrawn; the second gradient closes the round; the waiter gets
    the next step and the parameters are the exact mean update."""
    import torch

    from distributedtensorflowexample_amd.cluster import Server
    from distributedtensorflowexample_amd.ops import mlp_step
    from distributedtensorflowexample_amd.optim import GradientDescentOptimizer
    from distributedtensorflowexample_amd.parallel.gpu_ps import GpuPSStore, _flat_from_tf
    from distributedtensorflowexample_amd.parallel.ps import SyncReplicasOptimizer

    S = _S()
    n = mlp_step.NPARAM
    spec = {"ps": ["127.0.0.1:%d" % _free_port()], "worker": ["127.0.0.1:1"]}
    ps = Server(spec, "ps", 0)
    try:
        store = GpuPSStore(spec["ps"], gpu, 1, sync_replicas=2).create()
        p = _int_params(n)
        vals = _tf_values(p)
        vals[STEP] = 5
        store.assign(vals)
        assert store.uninitialized() == [] and store.read_int(STEP) == 5
        gs = [_int_grad(n, k, 0) for k in range(2)]
        dev = [torch.from_numpy(g).to(gpu) for g in gs]
        with pytest.raises(TimeoutError, match=r"round 5 .*1 of 2"):
            store.sync_push_flat(dev[0], 0.5, 5, timeout_s=0.3)
        with pytest.raises(RuntimeError, match="already pushed"):  # joined: no second begin
            store.sync_push_flat(dev[0], 0.5, 5, timeout_s=0.3)
        assert store.read_int(STEP) == 5
        assert store._st.sync_begin(dev[1].data_ptr(), 0.5, 5, _stream(), 0, 0)[:3] == (
            S.JOINED, 5, 1)
        assert store.sync_push_wait(5, timeout_s=10.0) == 6
        assert store.read_int(STEP) == 6
        want = S.round_reference(p, gs, 0.5)
        got = _flat_from_tf(store.pull(), torch.empty(n)).numpy()
        assert np.array_equal(got, want)
        with pytest.raises(ValueError, match="aggregates 2"):
            store.sync_push(_tf_values(gs[0]), 0.5, 3, 6)
        with pytest.raises(RuntimeError, match="rounds own"):
            store.fetch_add(STEP, 1)
        assert store.fetch_add(STEP, 0) == 6
        store.close()

        # SyncReplicasOptimizer, unchanged, over a store with R = 1: one step applied
        one = GpuPSStore(spec["ps"], gpu, 1, sync_replicas=1).create()
        vals[STEP] = 0
        one.assign(vals)
        opt = SyncReplicasOptimizer(GradientDescentOptimizer(0.5), 1, store=one, timeout_s=10.0)
        step = opt.apply_gradients([(t, k) for k, t in _tf_values(gs[0]).items()])
        assert step == 1 and opt.dropped == 0 and one.read_int(STEP) == 1
        got = _flat_from_tf(one.pull(), torch.empty(n)).numpy()
        assert np.array_equal(got, S.round_reference(p, gs[:1], 0.5))
        one.close()
    finally:
        ps.stop()


# -- two worker processes ---------------------------------------------------------------------
TRAIN_STEPS, LR, BATCH = 150, 0.05, 100


def _worker_flags(logdir):
    return types.SimpleNamespace(
        batch_size=BATCH, learning_rate=LR, training_steps=TRAIN_STEPS, logdir=logdir,
        log_every=100, eval_every=10 ** 9, save_model_secs=1000.0, save_summaries_secs=1000.0,
        use_locking=False, seed=0, device="cuda", ps_device="gpu", num_workers=2,
        sync_replicas=True, replicas_to_aggregate=0)


def _sync_worker(task, port, logdir, q):
    import torch

    from distributedtensorflowexample_amd.cluster import Server
    from distributedtensorflowexample_amd.data.mnist import read_data_sets
    from distributedtensorflowexample_amd.train.worker import Worker

    try:
        torch.cuda.set_device(0)
        spec = {"ps": ["127.0.0.1:%d" % port], "worker": ["127.0.0.1:1", "127.0.0.1:2"]}
        w = Worker("worker", task, Server(spec, "worker", task), _worker_flags(logdir + "/m"),
                   device="cuda", log=lambda *_: None)
        crcs, final = [], []
        pull_into, close = w.store.pull_into, w.store.close

        def pull_and_crc(dst):  # what this worker trains on at each step
            pull_into(dst)
            crcs.append(zlib.crc32(dst.cpu().numpy().tobytes()))

        def read_step_and_close(*a, **k):
            final.append(w.store.read_int(STEP))
            close(*a, **k)

        w.store.pull_into, w.store.close = pull_and_crc, read_step_and_close
        h = w.learn(read_data_sets(seed=task))
        q.put((task, [s for s, _, _ in h], [c for _, c, _ in h], crcs, final[0], None))
    except Exception as e:  # noqa: BLE001 - reported to the parent
        q.put((task, [], [], [], -1, repr(e)))


def _replay(rounds):
    """The same rounds in float64 in this process: both workers' batch streams from the same
    init, each round one apply of the mean of the two gradients (R = 2: the sum of two is
    order-free).  -> (CRC of the f32 init, losses[task][round])."""
    import torch

    from distributedtensorflowexample_amd import variables as vs
    from distributedtensorflowexample_amd.data.mnist import read_data_sets
    from distributedtensorflowexample_amd.models.dense import make_ps_model
    from distributedtensorflowexample_amd.ops import mlp_step
    from distributedtensorflowexample_amd.parallel.gpu_ps import _flat_from_tf
    from distributedtensorflowexample_amd.train.worker import build_worker_variables

    gvars, _ = build_worker_variables(make_ps_model("mlp", "", None), vs.VariableRegistry())
    init = {v.name: v.initial_value(0, i) for i, v in enumerate(gvars) if v.dtype == "float32"}
    p32 = _flat_from_tf(init, torch.empty(mlp_step.NPARAM))
    p = p32.double()
    data = [read_data_sets(seed=t) for t in (0, 1)]
    losses = ([], [])
    for _ in range(rounds):
        g = torch.zeros_like(p)
        for t in (0, 1):
            x, y = data[t].train.next_batch(BATCH)
            y = np.asarray(y)
            lab = torch.from_numpy(np.ascontiguousarray(y.argmax(1) if y.ndim == 2 else y))
            gt, loss, _ = mlp_step.reference_step(
                p, torch.from_numpy(np.ascontiguousarray(x)).double(), lab)
            losses[t].append(float(loss))
            g += gt
        p -= LR * g / 2
    return zlib.crc32(p32.numpy().tobytes()), losses


def test_two_sync_worker_processes(gpu, tmp_path):
    """--ps_device gpu --sync_replicas, chief + one more worker process sharing GPU 0: every
    worker is in every round (steps 0..150 each), both pull identical parameters at every
    step (no torn or unfinished round is ever seen), and each worker's losses follow a
    float64 replay of the 151 averaged rounds."""
    import multiprocessing as mp

    from distributedtensorflowexample_amd.cluster import Server

    port = _free_port()
    ps = Server({"ps": ["127.0.0.1:%d" % port], "worker": ["127.0.0.1:1", "127.0.0.1:2"]},
                "ps", 0)
    try:
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        procs = [ctx.Process(target=_sync_worker, args=(t, port, str(tmp_path), q))
                 for t in (0, 1)]
        for pr in procs:
            pr.start()
        res = sorted(q.get(timeout=180) for _ in procs)
        for pr in procs:
            pr.join(timeout=60)
            assert pr.exitcode == 0
    finally:
        ps.stop()
    for task, steps, _, crcs, _, err in res:
        assert err is None, err
        assert steps == list(range(TRAIN_STEPS + 1)), (task, steps[:5], steps[-5:])
        assert len(crcs) == len(steps)
    assert res[0][3] == res[1][3]  # the same parameters pulled at every step
    # the final global_step is the count of training steps run: steps 0..150 are 151 rounds,
    # and each worker reads the counter after its last round closed
    assert res[0][4] == res[1][4] == len(res[0][1]) == TRAIN_STEPS + 1
    init_crc, ref = _replay(TRAIN_STEPS + 1)
    assert res[0][3][0] == init_crc  # the replay starts from the workers' init
    worst = 0.0
    for task, _, losses, _, _, _ in res:
        for got, want in zip(losses, ref[task]):
            worst = max(worst, abs(got - want) / max(1.0, abs(want)))
            assert abs(got - want) < 1e-3 * max(1.0, abs(want)), (task, got, want)
    print("two sync workers vs float64 replay: worst loss error %.3g (bound 1e-3)" % worst)
