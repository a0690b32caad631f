"""Stateful optimizers on the GPU-resident parameter store (``--ps_device gpu --optimizer
momentum | adam``): the apply kernels of csrc/kernels/gpu_ps.hip on the raw store (async
applies and sync rounds, against ``gpu_ps_optim.apply_reference`` bitwise on exact data and
against float64 torch.optim otherwise), ``GpuPSStore``'s slot variables and their checkpoints,
two ``--sync_replicas`` worker processes sharing GPU 0, and a Worker end to end."""
import types
import zlib

import numpy as np
import pytest

import optim_reference as R

pytestmark = pytest.mark.gpu

STEP = "global/global_step"
SIZES = [1, 3, 1023, 1024, 1025, 4099, 79510]  # lone tail, chunk edge, multi-chunk tail, real
KINDS = {"momentum": 1, "adam": 2}


def _O():
    from distributedtensorflowexample_amd.parallel import gpu_ps_optim

    return gpu_ps_optim


def _S():
    from distributedtensorflowexample_amd.parallel import gpu_ps_sync

    return gpu_ps_sync


def _stream():
    from distributedtensorflowexample_amd.ops._ext import stream_handle

    return stream_handle("cuda:0")


def _raw(n, R_, slots):
    from distributedtensorflowexample_amd.ops import hip

    return hip().GpuParamStore(0, n, True, R_, slots)


def _write(st, off, a):
    a = np.ascontiguousarray(a)
    st.write(a.ctypes.data, off, a.nbytes)


def _read(st, off, count, dtype=np.float32):
    a = np.empty(count, dtype=dtype)
    st.read(a.ctypes.data, off, a.nbytes)
    return a


def _extent(st):
    """Bytes the store uses: everything up to the end of the last optimizer plane."""
    return st.opt_offset(st.opt_slots() - 1) + st.ctrl_offset()


def _snapshot(st):
    return _read(st, 0, _extent(st), np.uint8)


def _counters(st, n):
    w = _read(st, st.sync_offset(), 4 + _S().num_chunks(n), np.uint32)
    return int(w[1]), int(w[0]), int(w[2]), int(w[3]), w[4:].tolist()


def _begin(st, g, lr, step, hyper):
    status, rnd, ticket, _ = st.sync_begin(g.data_ptr(), lr, step, _stream(), 0, 0, *hyper)
    return status, rnd, ticket


def _int_grad(n, k, rnd):
    """Integers in [-8, 8], distinct per worker, per round and per element."""
    i = np.arange(n, dtype=np.int64)
    return ((i * 7 + k * 3 + rnd * 5) % 17 - 8).astype(np.float32)


def _int_params(n):
    return ((np.arange(n, dtype=np.int64) * 37) % 129 - 64).astype(np.float32)


def _pads_are_zero(st, n, R_):
    """The padding behind the parameters, every gradient slot and every optimizer plane."""
    pad = st.ctrl_offset() - n * 4
    starts = ([0] + [st.slot_offset(k) for k in range(R_)]
              + [st.opt_offset(k) for k in range(st.opt_slots())])
    return pad == 0 or not any(_read(st, s + n * 4, pad, np.uint8).any() for s in starts)


@pytest.mark.parametrize("R_", [1, 2, 4])
@pytest.mark.parametrize("n", SIZES)
def test_momentum_exact(gpu, n, R_):
    """Integer parameters and gradients, mu = 0.5, lr and 1 / R powers of two: every product and
    sum is exact in f32, so three async applies and then three sync rounds equal
    ``apply_reference`` bitwise -- parameters and the accumulator plane -- whatever the FMA
    contraction."""
    import torch

    O, S = _O(), _S()
    lr, hyper = 0.5, (0.5, 0.0, 0.0)
    st = _raw(n, R_, 1)
    try:
        assert st.opt_slots() == 1 and st.opt_offset(0) == st.slot_offset(R_ - 1) + st.ctrl_offset()
        p, acc = _int_params(n), np.zeros(n, np.float32)
        assert not _read(st, st.opt_offset(0), n).any()  # a new store's planes are zero
        _write(st, 0, p)

        def check(g):
            nonlocal p, acc
            want = O.apply_reference("momentum", p, g, [acc], lr, 1, hyper)
            fused = O.apply_reference("momentum", p, g, [acc], lr, 1, hyper, fma=True)
            assert np.array_equal(want[0], fused[0]) and np.array_equal(want[1][0], fused[1][0])
            p, (acc,) = want
            assert np.array_equal(_read(st, 0, n), p)
            assert np.array_equal(_read(st, st.opt_offset(0), n), acc)

        for k in range(3):  # async: the Hogwild apply, slots included; no round is touched
            g = _int_grad(n, k, 7)
            dev = torch.from_numpy(g).to(gpu)
            st.push_apply_opt(dev.data_ptr(), lr, *hyper, _stream())
            check(g)
            assert _counters(st, n) == (0, 0, 0, R_, [0] * S.num_chunks(n))
        for rnd in range(3):
            gs = [_int_grad(n, k, rnd) for k in range(R_)]
            for k in range(R_):
                assert st.sync_poll(_stream()) == (rnd, k)
                assert st.fetch_add(0, 0, _stream()) == rnd  # global_step moves with the close
                g = torch.from_numpy(gs[k]).to(gpu)
                assert _begin(st, g, lr, rnd, hyper) == (S.JOINED, rnd, k)
            check(O.mean_gradient(gs))
            assert st.sync_poll(_stream()) == (rnd + 1, 0)
            assert st.fetch_add(0, 0, _stream()) == rnd + 1
            assert _counters(st, n) == (rnd + 1, 0, 0, R_, [0] * S.num_chunks(n))
            for k in range(R_):  # each slot holds its ticket's gradient
                assert np.array_equal(_read(st, st.slot_offset(k), n), gs[k])
        assert acc.any() and _pads_are_zero(st, n, R_)
    finally:
        st.close()


@pytest.mark.parametrize("start", [0, 1000])
@pytest.mark.parametrize("R_", [0, 2, 3], ids=["async", "sync2", "sync3"])
@pytest.mark.parametrize("n", [4099, 79510])
def test_adam_against_float64(gpu, n, R_, start):
    """Three Adam steps at the reference's learning rate from make_case data (non-zero moments,
    zero / tiny / huge gradients), from global_step 0 and from a restored 1000: p, m and v stay
    within optim_reference.bound of torch.optim.Adam in float64.  In the sync cases the
    reference's gradient is the f32 ticket-order mean, so the summation's rounding is not
    charged to the bound."""
    import torch

    O, S = _O(), _S()
    lr, hyper = 1e-3, O.hyper_args("adam")
    p0, g0, m0, v0, regions = R.make_case(n, seed=23)
    gs = [(g0 * (1.0 + 0.25 * k)).numpy() for k in range(max(R_, 1))]
    gbar = torch.from_numpy(O.mean_gradient(gs))
    dev = [torch.from_numpy(g).to(gpu) for g in gs]
    st = _raw(n, R_, 2)
    try:
        _write(st, 0, p0.numpy())
        _write(st, st.opt_offset(0), m0.numpy())
        _write(st, st.opt_offset(1), v0.numpy())
        if start:
            st.set_step(start)
        p, m, v = p0.double(), m0.double(), v0.double()
        for k in range(3):
            step = start + k
            if R_:
                for t in range(R_):
                    assert _begin(st, dev[t], lr, step, hyper) == (S.JOINED, step, t)
            else:
                st.push_apply_opt(dev[0].data_ptr(), lr, *hyper, _stream())
                assert st.fetch_add(0, 1, _stream()) == step  # the worker's counter_op
            assert st.fetch_add(0, 0, _stream()) == step + 1
            p, m, v = R.adam_step(p, gbar, m, v, lr, step + 1, adamw=False, wd=0.0)
            for name, off, ref in (("p", 0, p), ("m", st.opt_offset(0), m),
                                   ("v", st.opt_offset(1), v)):
                R.assert_close("adam %s step %d" % (name, step + 1),
                               torch.from_numpy(_read(st, off, n)), ref, k + 1, regions)
    finally:
        st.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_statuses_leave_every_byte(gpu, kind):
    """STALE, AHEAD and LATE pushes change nothing: parameters, control block, sync region,
    gradient slots and the optimizer's planes, byte for byte."""
    import torch

    O, S = _O(), _S()
    n, R_, lr = 1025, 2, 0.5
    hyper = O.hyper_args(kind, momentum=0.5)
    st = _raw(n, R_, KINDS[kind])
    try:
        _write(st, 0, _int_params(n))
        dev = [torch.from_numpy(_int_grad(n, k, 0)).to(gpu) for k in range(3)]
        for k in range(R_):
            assert _begin(st, dev[k], lr, 0, hyper) == (S.JOINED, 0, k)
        assert st.sync_poll(_stream()) == (1, 0)
        before = _snapshot(st)
        assert before.size == st.opt_offset(KINDS[kind] - 1) + st.ctrl_offset()
        assert _read(st, st.opt_offset(KINDS[kind] - 1), n).any()  # the round wrote the planes
        status, rnd, _ = _begin(st, dev[2], lr, 0, hyper)  # local_step = round - 1
        assert (status, rnd) == (S.STALE, 1)
        assert np.array_equal(_snapshot(st), before)
        status, rnd, _ = _begin(st, dev[2], lr, 2, hyper)  # local_step = round + 1
        assert (status, rnd) == (S.AHEAD, 1)
        assert np.array_equal(_snapshot(st), before)
        # a full, still open round (both tickets taken, as a backup replica meets it): LATE
        _write(st, st.sync_offset(), np.array([S.pack_round(1, R_)], np.uint64))
        before = _snapshot(st)
        assert _begin(st, dev[2], lr, 1, hyper) == (S.LATE, 1, R_)
        assert np.array_equal(_snapshot(st), before)
        with pytest.raises(RuntimeError, match="out of range"):
            _read(st, _extent(st), 1, np.uint8)
    finally:
        st.close()


def test_layout_without_and_with_planes(gpu):
    """opt_slots = 0 (five-argument constructor): today's control offset, extent and "out of
    range" edge, and no optimizer entry points; opt_slots = k appends k planes of the padded
    parameter size behind everything, with or without a sync region."""
    import torch

    from distributedtensorflowexample_amd.ops import hip

    n = 4099
    pb = (n * 4 + 255) // 256 * 256
    g = torch.zeros(n, device=gpu)
    st = hip().GpuParamStore(0, n, True, 0, 0)
    try:
        assert st.opt_slots() == 0 and st.sync_slots() == 0 and st.ctrl_offset() == pb
        _read(st, st.ctrl_offset(), 32, np.uint64)  # the whole control block, no more
        with pytest.raises(RuntimeError, match="out of range"):
            _read(st, st.ctrl_offset() + 256, 1, np.uint8)
        with pytest.raises(RuntimeError, match="no optimizer slots"):
            st.push_apply_opt(g.data_ptr(), 0.5, 0.5, 0.0, 0.0, _stream())
        with pytest.raises(RuntimeError, match="no optimizer slots"):
            st.opt_offset(0)
    finally:
        st.close()
    st = hip().GpuParamStore(0, n, True, 2, 0)
    try:
        sync_extent = st.slot_offset(1) + pb
        with pytest.raises(RuntimeError, match="out of range"):
            _read(st, sync_extent, 1, np.uint8)
    finally:
        st.close()
    for R_, base in ((0, pb + 256), (2, sync_extent)):
        st = hip().GpuParamStore(0, n, True, R_, 2)
        try:
            assert st.ctrl_offset() == pb
            assert [st.opt_offset(k) for k in range(2)] == [base, base + pb]
            assert _read(st, st.ctrl_offset(), 3, np.uint64).tolist() == [0, 0, 2]  # the kind
            _read(st, base + pb, pb, np.uint8)
            with pytest.raises(RuntimeError, match="out of range"):
                _read(st, base + 2 * pb, 1, np.uint8)
            with pytest.raises(RuntimeError, match="bad optimizer slot"):
                st.opt_offset(2)
        finally:
            st.close()
    with pytest.raises(RuntimeError, match="opt_slots"):
        hip().GpuParamStore(0, n, True, 0, 3)


def _free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("sync_r", [0, 1], ids=["async", "sync"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_store_slots_and_checkpoint(gpu, tmp_path, kind, sync_r):
    """GpuPSStore on a one-process cluster: the slot variables are uninitialized until init,
    come back from read_all() in TF layout, and a run saved after three steps and restored into
    a new store continues bitwise like five uninterrupted steps (one worker: deterministic;
    Adam's t comes from the restored global_step)."""
    import torch

    from distributedtensorflowexample_amd.cluster import Server
    from distributedtensorflowexample_amd.ops import mlp_step
    from distributedtensorflowexample_amd.parallel.gpu_ps import (VAR_NAMES, GpuPSStore,
                                                                  _tf_from_flat)
    from distributedtensorflowexample_amd.train.saver import FastSaver, latest_checkpoint
    from distributedtensorflowexample_amd.train.worker import restricted_assign

    O = _O()
    n, lr = mlp_step.NPARAM, 1e-3
    hyper = O.hyper_args(kind)
    gen = torch.Generator().manual_seed(31)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(5)]
    dev = [g.to(gpu) for g in grads]
    slot_names = [k for plane in O.slot_names(kind, VAR_NAMES) for k in plane]
    spec = {"ps": ["127.0.0.1:%d" % _free_port()], "worker": ["127.0.0.1:1"]}
    ps = Server(spec, "ps", 0)

    def new_store():
        return GpuPSStore(spec["ps"], gpu, 1, sync_replicas=sync_r, optimizer=kind).create()

    def run(store, steps):
        for k in steps:
            if sync_r:
                assert store.sync_push_flat(dev[k], lr, k, timeout_s=10.0)[:2] == (k + 1, True)
            else:
                store.push_apply_flat(dev[k], lr)
                assert store.fetch_add(STEP, 1) == k

    try:
        store = new_store()
        assert store.uninitialized() == list(VAR_NAMES) + [STEP] + slot_names
        init = _tf_from_flat(p0)
        init[STEP] = 0
        with pytest.raises(ValueError, match="slot variables together"):
            store.assign({slot_names[0]: torch.zeros(784, 100)})
        store.assign(dict(init, **{k: torch.zeros(init[k.rsplit("/", 1)[0]].shape)
                                   for k in slot_names}))
        assert store.uninitialized() == []
        run(store, range(5))
        whole = store.read_all()
        store.close()

        # five steps of the f32 reference: the same values up to the kernel's own rounding
        # choices (FMA contraction, rsqrt), in the layout the store reports them
        p, slots = p0.numpy(), [np.zeros(n, np.float32) for _ in slot_names[::4]]
        for k in range(5):
            p, slots = O.apply_reference(kind, p, grads[k].numpy(), slots, lr, k + 1, hyper)
        assert sorted(whole) == sorted(list(VAR_NAMES) + [STEP] + slot_names)
        assert int(whole[STEP]) == 5
        for plane, flat in zip(O.slot_names(kind, VAR_NAMES), slots):
            want = _tf_from_flat(torch.from_numpy(flat), plane)
            for name in plane:
                assert whole[name].shape == want[name].shape
                R.assert_close(name, whole[name].flatten(), want[name].flatten().double(), 5,
                               [("all", torch.arange(want[name].numel()))])
        assert tuple(whole[slot_names[0]].shape) == (784, 100) and whole[slot_names[0]].any()

        store = new_store()
        store.assign(dict(init, **{k: torch.zeros(init[k.rsplit("/", 1)[0]].shape)
                                   for k in slot_names}))
        run(store, range(3))
        names = list(VAR_NAMES) + [STEP] + slot_names
        prefix = FastSaver({k: None for k in names}).save(
            None, str(tmp_path / "model.ckpt"), global_step=store.read_int(STEP),
            variables=store.read_all())
        store.close()
        assert latest_checkpoint(str(tmp_path)) == prefix and prefix.endswith("-3")

        store = new_store()
        assert store.uninitialized() == names
        FastSaver({k: None for k in names},
                  assign=restricted_assign(store.assign, names)).restore(None, prefix)
        assert store.uninitialized() == [] and store.read_int(STEP) == 3
        run(store, range(3, 5))
        resumed = store.read_all()
        store.close()
        for k in names:
            assert torch.equal(torch.as_tensor(resumed[k]), torch.as_tensor(whole[k])), k
    finally:
        ps.stop()


# -- worker processes ---------------------------------------------------------------------------
BATCH = 100
ROUNDS = 60
# (learning rate, hyper-parameter flags) of the two-worker runs
TWO_WORKER = {"momentum": (0.05, {"momentum": 0.5}), "adam": (1e-3, {})}


def _worker_flags(logdir, kind, lr, steps, num_workers, sync, extra):
    return types.SimpleNamespace(
        batch_size=BATCH, learning_rate=lr, training_steps=steps, logdir=logdir,
        log_every=100, eval_every=10 ** 9, save_model_secs=1000.0, save_summaries_secs=1000.0,
        use_locking=False, seed=0, device="cuda", ps_device="gpu", num_workers=num_workers,
        sync_replicas=sync, replicas_to_aggregate=0, optimizer=kind, **extra)


def replay(kind, rounds, tasks, lr, extra, dtype):
    """The same rounds on the CPU in ``dtype``: the workers' batch streams from the same init,
    each round one apply of the optimizer (slots carried) on the mean of the tasks' gradients.
    -> (CRC of the f32 init, losses[task][round])."""
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
    p = p32.to(dtype)
    mu = R.f32(extra.get("momentum", 0.9))
    b1, b2, eps = (R.f32(x) for x in _O().hyper_args("adam"))
    lr = R.f32(lr)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    data = [read_data_sets(seed=t) for t in tasks]
    losses = [[] for _ in tasks]
    for rnd in range(rounds):
        g = torch.zeros_like(p)
        for i, _ in enumerate(tasks):
            x, y = data[i].train.next_batch(BATCH)
            y = np.asarray(y)
            lab = torch.from_numpy(np.ascontiguousarray(y.argmax(1) if y.ndim == 2 else y))
            gt, loss, _ = mlp_step.reference_step(
                p, torch.from_numpy(np.ascontiguousarray(x)).to(dtype), lab)
            losses[i].append(float(loss))
            g += gt
        g /= len(tasks)
        if kind == "momentum":
            m = mu * m + g
            p = p - lr * m
        else:
            t = rnd + 1
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * g * g
            p = p - (lr / (1 - b1 ** t)) * m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
    return zlib.crc32(p32.numpy().tobytes()), losses


def worst_error(got, want):
    """max |got - want| / max(1, |want|) over the tasks' loss curves."""
    return max(abs(a - b) / max(1.0, abs(b)) for gs, ws in zip(got, want) for a, b in zip(gs, ws))


def _sync_worker(task, port, logdir, kind, q):
    import torch

    from distributedtensorflowexample_amd.cluster import Server
    from distributedtensorflowexample_amd.data.mnist import read_data_sets
    from distributedtensorflowexample_amd.train.worker import Worker

    try:
        torch.cuda.set_device(0)
        lr, extra = TWO_WORKER[kind]
        spec = {"ps": ["127.0.0.1:%d" % port], "worker": ["127.0.0.1:1", "127.0.0.1:2"]}
        w = Worker("worker", task, Server(spec, "worker", task),
                   _worker_flags(logdir + "/m", kind, lr, ROUNDS - 1, 2, True, extra),
                   device="cuda", log=lambda *_: None)
        crcs = []
        pull_into = w.store.pull_into

        def pull_and_crc(dst):  # what this worker trains on at each step
            pull_into(dst)
            crcs.append(zlib.crc32(dst.cpu().numpy().tobytes()))

        w.store.pull_into = pull_and_crc
        h = w.learn(read_data_sets(seed=task))
        q.put((task, [s for s, _, _ in h], [c for _, c, _ in h], crcs, None))
    except Exception as e:  # noqa: BLE001 - reported to the parent
        q.put((task, [], [], [], repr(e)))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_two_sync_worker_processes(gpu, tmp_path, kind):
    """--ps_device gpu --sync_replicas --optimizer momentum | adam, chief + one more worker
    process sharing GPU 0, 60 rounds: both pull identical parameters at every step, and each
    worker's losses follow a float64 replay that carries the slots, within the sync test's own
    1e-3 * max(1, |loss|).

    The bound tests the kernel, not chaos: a float32 CPU replay (``replay`` with
    torch.float32) of the same 60 rounds stays far within a third of that bound of the float64
    replay.  Measured worst error / bound: momentum (lr 0.05, mu 0.5) 0.0002, adam (lr 1e-3)
    0.0003."""
    import multiprocessing as mp

    import torch

    from distributedtensorflowexample_amd.cluster import Server

    port = _free_port()
    ps = Server({"ps": ["127.0.0.1:%d" % port], "worker": ["127.0.0.1:1", "127.0.0.1:2"]},
                "ps", 0)
    try:
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        procs = [ctx.Process(target=_sync_worker, args=(t, port, str(tmp_path), kind, q))
                 for t in (0, 1)]
        for pr in procs:
            pr.start()
        res = sorted(q.get(timeout=180) for _ in procs)
        for pr in procs:
            pr.join(timeout=60)
            assert pr.exitcode == 0
    finally:
        ps.stop()
    for task, steps, _, crcs, err in res:
        assert err is None, err
        assert steps == list(range(ROUNDS)), (task, steps[:5], steps[-5:])
        assert len(crcs) == len(steps)
    assert res[0][3] == res[1][3]  # the same parameters pulled at every step
    lr, extra = TWO_WORKER[kind]
    init_crc, ref = replay(kind, ROUNDS, (0, 1), lr, extra, torch.float64)
    assert res[0][3][0] == init_crc  # the replay starts from the workers' init
    worst = worst_error([r[2] for r in res], ref)
    print("two sync %s workers vs float64 replay: worst loss error %.3g (bound 1e-3)"
          % (kind, worst))
    assert worst < 1e-3


def test_worker_adam_async_end_to_end(gpu, tmp_path):
    """A single-process Worker with --ps_device gpu --optimizer adam in async mode, 150 steps on
    the MNIST assets: the slot variables are initialised with the others, and the losses stay
    within 1e-3 * max(1, |loss|) of a float64 replay (a float32 CPU replay of the same steps
    stays within 0.0004 of that bound)."""
    import torch

    from distributedtensorflowexample_amd.cluster import Server
    from distributedtensorflowexample_amd.data.mnist import read_data_sets
    from distributedtensorflowexample_amd.train.worker import Worker

    steps = 150
    spec = {"ps": ["127.0.0.1:%d" % _free_port()], "worker": ["127.0.0.1:1"]}
    ps = Server(spec, "ps", 0)
    try:
        w = Worker("worker", 0, Server(spec, "worker", 0),
                   _worker_flags(str(tmp_path / "m"), "adam", 1e-3, steps, 1, False, {}),
                   device="cuda", log=lambda *_: None)
        assert [v.name for v in w.global_vars][5:] == [
            k for plane in w.store.slot_names for k in plane]
        seen = []
        assign = w.store.assign
        w.store.assign = lambda values: (seen.append(sorted(values)), assign(values))[1]
        h = w.learn(read_data_sets(seed=0))
    finally:
        ps.stop()
    assert seen == [sorted(v.name for v in w.global_vars)]  # one init, slots included
    assert [s for s, _, _ in h] == list(range(steps + 1))
    _, ref = replay("adam", steps + 1, (0,), 1e-3, {}, torch.float64)
    worst = worst_error([[c for _, c, _ in h]], ref)
    print("adam worker vs float64 replay: worst loss error %.3g (bound 1e-3)" % worst)
    assert worst < 1e-3
