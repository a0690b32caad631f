"""Per-epoch reshuffle of the device-resident pipeline: the gather kernel
(csrc/kernels/shuffle.hip) against ``shuffle_index`` and ``FusedMLPTrainer(shuffle=True)``
across epoch boundaries (eager steps, graph replays, the C++ host loop, resume, the factor
engine's x_all planes).

Datasets are 5 * B + 7 rows (a tail that no fixed walk would ever feed) and runs are 13 steps:
two boundaries, so both shuffled buffers are written and read, and the update pending across a
boundary reads the previous epoch's last batch from the other buffer.
"""
import functools
import types

import pytest
import torch

from distributedtensorflowexample_amd.ops import init, mlp_step
from distributedtensorflowexample_amd.ops.shuffle import shuffle_index, shuffle_rows_

pytestmark = pytest.mark.gpu

LR, STEPS, SEED = 0.3, 13, 5


# ---------------------------------------------------------------------------------------
# the gather kernel
# ---------------------------------------------------------------------------------------
def _source(W, n, pad, dev):
    """[W, n, 784] with src[w, i, c] = w * 1e6 + i * 1000 + c (exact in f32 up to n = 1000: a
    misplaced 16-byte chunk of any row or plane shows), plane stride (n + pad) * 784."""
    big = torch.empty(W, n + pad, 784, device=dev)
    src = big[:, :n]
    w = torch.arange(W, device=dev, dtype=torch.float32).view(W, 1, 1)
    i = torch.arange(n, device=dev, dtype=torch.float32).view(1, n, 1)
    c = torch.arange(784, device=dev, dtype=torch.float32).view(1, 1, 784)
    src.copy_(w * 1e6 + i * 1000 + c)
    return big, src


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 100, 257, 1000])
def test_shuffle_rows_matches_reference(gpu, n, W):
    """Bit-equal to ``src[:, shuffle_index(seed, epoch, n)]``, labels too; for W = 3 both
    tensors are slices of bigger allocations (plane strides > n * 784, different for dst and
    src) whose padding rows stay untouched.  n = 1000 at 4 rows per block is more than one
    block; 257 = 4 * 64 + 1 leaves a block with one row."""
    pad = 0 if W == 1 else 3
    _, src = _source(W, n, pad, gpu)
    dbig = torch.full((W, n + 2 * pad, 784), float("nan"), device=gpu)
    dst = dbig[:, :n]
    y = (torch.arange(n, device=gpu, dtype=torch.int32) * 7 + 1)
    dy = torch.full_like(y, -1)
    for seed, epoch in ((0, 0), (9, 4)):
        idx = shuffle_index(seed, epoch, n).to(gpu)
        if W == 1:  # the [n, 784] form
            shuffle_rows_(dst[0], dy, src[0], y, seed, epoch)
        else:
            shuffle_rows_(dst, dy, src, y, seed, epoch)
        torch.cuda.synchronize()
        assert torch.equal(dst, src[:, idx])
        assert torch.equal(dy, y[idx])
        assert bool(torch.isnan(dbig[:, n:]).all())
    shuffle_rows_(dst, None, src, None, 1, 1)  # (labels are optional)
    torch.cuda.synchronize()
    assert torch.equal(dst, src[:, shuffle_index(1, 1, n).to(gpu)])


def test_shuffle_rows_rejects_overlap_and_misalignment(gpu):
    n = 8
    buf = torch.zeros((n + 1) * 784 + 4, device=gpu)
    rows = buf[:(n + 1) * 784].view(n + 1, 784)
    y = torch.zeros(n, device=gpu, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="overlap"):
        shuffle_rows_(rows[1:], None, rows[:-1], None, 0, 0)
    with pytest.raises(RuntimeError, match="overlap"):
        shuffle_rows_(rows[:n], None, rows[:n], None, 0, 0)
    with pytest.raises(RuntimeError, match="overlap"):
        shuffle_rows_(torch.empty(n, 784, device=gpu), y, rows[:n], y, 0, 0)
    off = buf[1:1 + n * 784].view(n, 784)  # base 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="aligned"):
        shuffle_rows_(torch.empty(n, 784, device=gpu), None, off, None, 0, 0)
    with pytest.raises(RuntimeError, match="aligned"):
        shuffle_rows_(off, None, torch.empty(n, 784, device=gpu), None, 0, 0)


# ---------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------
def _data(gpu, B, seed=4):
    """0.1-scaled N(0, 1) weights and 5 * B + 7 rows, as tests/test_mlp_rowmajor_gpu.py."""
    n = 5 * B + 7
    p = torch.empty(mlp_step.NPARAM, device=gpu)
    init.fill_(p, "normal", 0.0, 1.0, seed=seed)
    p[mlp_step.OFF_B1:mlp_step.OFF_W2].zero_()
    p[mlp_step.OFF_B2:].zero_()
    p.mul_(0.1)
    g = torch.Generator().manual_seed(seed + B)
    x = torch.rand(n, 784, generator=g).to(gpu)
    y = torch.randint(0, 10, (n,), generator=g).to(gpu).int()
    return p, x, y


@functools.lru_cache(maxsize=None)
def _reference(B):
    """float64 SGD over ``reference_step`` fed in ``shuffle_index`` order: (parameters after
    every step, losses); computed once per batch size and shared."""
    p, x, y = _data(torch.device("cuda:0"), B)
    ref, xr, yr = p.double().cpu(), x.double().cpu(), y.cpu()
    n, nb = x.shape[0], x.shape[0] // B
    params, losses = [], []
    for s in range(STEPS):
        idx = shuffle_index(SEED, s // nb, n)[(s % nb) * B:(s % nb + 1) * B]
        g, loss, _ = mlp_step.reference_step(ref, xr[idx], yr[idx])
        ref = ref - LR * g
        params.append(ref)
        losses.append(float(loss))
    return params, torch.tensor(losses)


def _trainer(gpu, B, **kw):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = _data(gpu, B)
    kw.setdefault("shuffle", True)
    return FusedMLPTrainer(p, x, y, B, LR, shuffle_seed=SEED, **kw)


def _err(tr, ref):
    torch.cuda.synchronize()
    return (tr.params.double().cpu() - ref).abs().max().item()


DRIVES = ["eager", "eager_flush_at_boundary", "graph", "launched", "launched_flush_at_boundary",
          "three_launch"]


@pytest.mark.parametrize("drive", DRIVES)
@pytest.mark.parametrize("B", [16, 100])
def test_shuffled_trajectory(gpu, B, drive):
    """13 steps over 5 batches per epoch against the float64 reference in shuffle_index order
    (< 1e-4, the bound of test_rowmajor_trajectory); global_step and the per-step losses line up
    (atol 1e-4).  ``*_flush_at_boundary``: a flush after step 5, where pos == 0 with the update
    pending (its input is the finished epoch's last batch, in the other buffer)."""
    refs, losses = _reference(B)
    tr = _trainer(gpu, B, pipeline=drive != "three_launch")
    assert tr.nbatches == 5 and tr.pipelined == (drive != "three_launch")
    e5 = None
    if drive in ("eager", "three_launch"):
        for _ in range(STEPS):
            tr.step()
    elif drive == "eager_flush_at_boundary":
        for _ in range(5):
            tr.step()
        assert tr.pos == 0 and tr.pending and tr.epoch == 1
        tr.flush()
        e5 = _err(tr, refs[4])
        tr.run(STEPS - 5, use_graph=False)
    elif drive == "graph":
        tr.run(STEPS)  # one eager step, then replays of 4, 5 and 3 steps
        assert len(tr._graphs) == 3
    elif drive == "launched":
        tr.run_launched(STEPS, flush=True)
        assert not tr.pending
    else:
        tr.run_launched(5, flush=True)  # (the flush runs inside the C++ call of epoch 0)
        assert tr.pos == 0 and not tr.pending and tr.epoch == 1
        e5 = _err(tr, refs[4])
        tr.run_launched(3)
        tr.run_launched(STEPS - 8, flush=True)  # (starts mid-epoch, crosses the second boundary)
    tr.flush()
    e13 = _err(tr, refs[-1])
    got = tr.stats_range(0, STEPS)[:, 0]
    print("B=%d %s: vs f64 after 5 / 13 steps %s / %.3e, max loss diff %.3e"
          % (B, drive, e5, e13, float((got.double() - losses.double()).abs().max())))
    assert e5 is None or e5 < 1e-4
    assert e13 < 1e-4
    assert tr.global_step() == STEPS and tr.epoch == 2 and tr.pos == STEPS % 5
    assert torch.allclose(got, losses, atol=1e-4)


def test_prepared_graphs_cross_boundaries(gpu):
    """prepare() captures the graphs of both buffer parities without running anything; the run
    that follows replays them and matches the reference."""
    B = 16
    refs, _ = _reference(B)
    tr = _trainer(gpu, B)
    tr.step()
    before = (tr.pos, tr.cur, tr.epoch, tr.x.data_ptr())
    tr.prepare(STEPS - 1)
    assert (tr.pos, tr.cur, tr.epoch, tr.x.data_ptr()) == before
    n = len(tr._graphs)
    tr.run(STEPS - 1)
    assert len(tr._graphs) == n == 3
    tr.flush()
    assert _err(tr, refs[-1]) < 1e-4


@pytest.mark.parametrize("B", [16, 100])
def test_tail_rows_are_fed(gpu, B):
    """Labels = arange(n): the trainer's current label buffer IS the epoch's order.  Each epoch
    it equals shuffle_index, and over 3 epochs the rows fed (the first nbatches * B positions)
    cover all 5 * B + 7 rows -- without the reshuffle the last 7 are never seen."""
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, _ = _data(gpu, B)
    n = x.shape[0]
    tr = FusedMLPTrainer(p, x, torch.arange(n, dtype=torch.int32), B, LR, shuffle=True,
                         shuffle_seed=SEED)
    fed = set()
    for e in range(3):
        assert tr.epoch == e
        torch.cuda.synchronize()
        order = tr.labels.cpu().long()
        assert torch.equal(order, shuffle_index(SEED, e, n))
        assert torch.equal(tr.x, x[order.to(gpu)])
        fed |= set(order[:tr.nbatches * B].tolist())
        tr.run(tr.nbatches)
    assert fed == set(range(n))
    plain = FusedMLPTrainer(p, x, torch.arange(n, dtype=torch.int32), B, LR)
    assert set(plain.labels[:plain.nbatches * B].tolist()) == set(range(n - 7))


@pytest.mark.parametrize("B", [16, 100])
def test_resume_reproduces_the_order(gpu, B):
    """7 steps, snapshot, a NEW trainer with load_params + seek(7), 6 more steps: equal to the
    uninterrupted 13 steps within 1e-5 (what the suite accepts between two launch forms of the
    same step)."""
    whole = _trainer(gpu, B)
    whole.run(STEPS, use_graph=False)
    whole.flush()
    first = _trainer(gpu, B)
    first.run(7, use_graph=False)
    snap = first.snapshot()
    second = _trainer(gpu, B)
    second.load_params(snap)
    second.seek(7)
    assert (second.pos, second.epoch, second.pending) == (2, 1, False)
    assert second.global_step() == 7
    second.run(STEPS - 7, use_graph=False)
    second.flush()
    torch.cuda.synchronize()
    err = (second.params - whole.params).abs().max().item()
    print("B=%d resume vs uninterrupted: %.3e" % (B, err))
    assert err < 1e-5
    assert second.global_step() == whole.global_step() == STEPS
    a, b = second.stats_range(7, STEPS), whole.stats_range(7, STEPS)
    assert torch.allclose(a, b, atol=1e-4)


def test_shuffle_off_is_the_default_path(gpu):
    """shuffle=False is bit-identical to a trainer constructed without the argument, and keeps
    no extra buffers."""
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    B = 16
    p, x, y = _data(gpu, B)
    a = FusedMLPTrainer(p, x, y, B, LR)
    b = FusedMLPTrainer(p, x, y, B, LR, shuffle=False, shuffle_seed=3)
    for t in (a, b):
        t.run(4)
        t.run_launched(5)
        t.run(4, use_graph=False)
        t.seek(t.global_step())
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params)
    assert torch.equal(a.stats_range(0, STEPS), b.stats_range(0, STEPS))
    assert not hasattr(b, "xs") and b.x.data_ptr() == a.x.data_ptr() and b.epoch == 0


def test_persistent_engine_refuses_shuffle(gpu):
    tr = _trainer(gpu, 16)
    assert not tr.persistent_ok and _trainer(gpu, 16, shuffle=False).persistent_ok
    with pytest.raises(RuntimeError, match="shuffle"):
        tr.run_persistent(3)


def test_mirrored_gpu_run_with_shuffle_flag(gpu, tmp_path, monkeypatch):
    """--shuffle reaches the GPU trainer: the mirrored loop's per-step losses follow the
    float64 reference in shuffle_index order (atol 1e-4 relative to the loss, as the CPU
    path's test) and differ from the unshuffled run."""
    import numpy as np

    from distributedtensorflowexample_amd.data.mnist import DataSet, DataSets
    from distributedtensorflowexample_amd.models import mlp as mlp_model
    from distributedtensorflowexample_amd.train.mirrored_mlp import train_mirrored

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    B, steps, lr = 16, 12, 0.05
    n = 5 * B + 7
    g = torch.Generator().manual_seed(3)
    x = torch.rand(n, 784, generator=g).numpy()
    y = torch.randint(0, 10, (n,), generator=g).numpy().astype(np.uint8)
    test = DataSet(x[:8], y[:8], one_hot=False)
    ds = DataSets(train=DataSet(x, y, one_hot=False), validation=test, test=test,
                  synthetic_train=True)

    def run(tag, **kw):
        fl = types.SimpleNamespace(batch_size=B, learning_rate=lr, training_steps=steps,
                                   logdir=str(tmp_path / tag), log_every=1, eval_every=10 ** 9,
                                   save_model_secs=1000.0, save_summaries_secs=1000.0,
                                   use_locking=False, seed=0, device="cuda", **kw)
        hist, _ = train_mirrored(fl, ds, log=lambda *_: None)
        assert [h[0] for h in hist] == list(range(1, steps + 1))
        return [h[1] for h in hist]

    p = mlp_model.init_params(gpu, seed=0).double().cpu()  # (what the loop initialises on the GPU)
    xr, yr = torch.from_numpy(x).double(), torch.from_numpy(y).int()
    ref = []
    for s in range(steps):
        idx = shuffle_index(4, s // 5, n)[(s % 5) * B:(s % 5 + 1) * B]
        gr, loss, _ = mlp_step.reference_step(p, xr[idx], yr[idx])
        p = p - lr * gr
        ref.append(float(loss))
    got, off = run("on", shuffle=True, shuffle_seed=4), run("off")
    print("shuffled", got, "\nreference", ref, "\nunshuffled", off)
    for a, b in zip(got, ref):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (got, ref)
    assert max(abs(a - b) for a, b in zip(got, off)) > 1e-2


# ---------------------------------------------------------------------------------------
# the factor engine: every rank's stream (x_all) is shuffled locally
# ---------------------------------------------------------------------------------------
def test_factor_engine_shuffles_every_plane(gpu):
    """World 2, B = 16, simulated peers (``XgmiComm.with_local_peers``, as
    tests/test_xgmi_sim_gpu.py::test_factor2_fwdapply_simulated_peers): after one boundary both
    planes of the trainer's current x_all buffer equal the reference gather, the pending
    update's input at pos == 0 is the finished epoch's last batch in the OTHER buffer (every
    rank's, at the shared plane stride), and the first launch of the step after the boundary,
    issued with the trainer's pointers, applies the expected global update.

    The simulated peers never run: their words are staged per launch, so the boundary is
    crossed on the host mirrors and the launch under test is issued as that test issues it."""
    from distributedtensorflowexample_amd.data.synthetic import mnist_like_device
    from distributedtensorflowexample_amd.models.mlp import init_params
    from distributedtensorflowexample_amd.ops._ext import hip, ptr, stream_handle
    from distributedtensorflowexample_amd.parallel.xgmi import XgmiComm
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    import test_xgmi_sim_gpu as sim

    world, rank, B, lr = 2, 1, 16, 0.5
    n = 2 * B + 5
    x_all = torch.stack([mnist_like_device(n, seed=70 + q, device=gpu)[0]
                         for q in range(world)]).contiguous()
    y = mnist_like_device(n, seed=70 + rank, device=gpu)[1].int()
    p = init_params(gpu, seed=9, stddev=0.3)
    comm, regs = XgmiComm.with_local_peers(rank, world, mlp_step.NPARAM, device=gpu)
    tr = FusedMLPTrainer(p, x_all[rank], y, B, lr * world, world_size=world, factor_comm=comm,
                         x_all=x_all, rank=rank, shuffle=True, shuffle_seed=SEED)
    assert tr.pipelined and tr.nbatches == 2
    idx0 = shuffle_index(SEED, 0, n).to(gpu)
    torch.cuda.synchronize()
    assert torch.equal(tr._dst[0], x_all[:, idx0]) and torch.equal(tr.labels, y[idx0])
    assert tr.x.data_ptr() == tr._dst[0][rank].data_ptr() and tr.xstride == x_all.stride(0)
    # the last step of epoch 0 as the simulated harness can run it: the factors of the last
    # batch in the workspace, every rank's dz1 in dz1A, the host mirrors at the boundary
    x_prev, y_prev = tr.batch(1)
    sim._pipelined_fwd_head(tr.bufs[tr.cur], x_prev, y_prev, tr.ws)
    g = torch.Generator().manual_seed(3)
    dz1A = torch.zeros(world, B, mlp_step.HP)
    dz1A[:, :, :100] = torch.randn(world, B, 100, generator=g) * 0.01
    tr.dz1A.copy_(dz1A.reshape(-1).to(gpu))
    tr.pos, tr.pending = 0, True
    tr._wrapped()
    assert tr.epoch == 1 and tr.x.data_ptr() == tr._dst[1][rank].data_ptr()
    idx1 = shuffle_index(SEED, 1, n).to(gpu)
    torch.cuda.synchronize()
    assert torch.equal(tr._dst[1], x_all[:, idx1]) and torch.equal(tr.labels, y[idx1])
    assert torch.equal(tr._dst[0], x_all[:, idx0])  # (the other buffer is intact)
    xp = tr._xprev(0)
    assert xp.data_ptr() == tr._dst[0][rank][B:2 * B].data_ptr()
    xb, yb = tr.batch(0)
    assert torch.equal(xb, x_all[rank][idx1[:B]])
    # the step after the boundary: expected-update check of the existing test
    p_old, p_new = tr.bufs[tr.cur], tr.bufs[tr.cur ^ 1]
    own = sim._ref_grad(p_old, x_prev, y_prev)
    gW1 = sim._global_w1_grad(dz1A.to(gpu), x_all[:, idx0[B:2 * B]], B)
    peers = sim._peer_grads(world, rank, 17 + world, 0.05)
    lo = mlp_step.OFF_B1
    sim._stage_param_words(comm, regs, peers, 1, lo, mlp_step.NPARAM)
    torch.cuda.synchronize()
    comm.mlp_fwdapply_factor(p_old, p_new, lr, xp, xb, tr.xstride, tr.dz1A, tr.ws, True)
    hip().mlp_head2(ptr(p_new), ptr(yb), ptr(tr.ws.buf), B, stream_handle(),
                    mlp_step.FACTOR_SLABS)
    comm.check()
    upd = sim._expected_update(own, peers, rank)
    upd[:lo] = gW1
    exp = p_old.double().cpu() - lr * upd
    err = float((p_new.double().cpu() - exp).abs().max())
    print("factor2 step after the boundary: %.3e" % err)
    assert err <= 2e-5, err
    hbuf, _, _ = sim._ws_views(tr.ws)
    h_ref, _ = mlp_step.reference_forward(p_new.double().cpu(), xb.double().cpu())
    assert float((hbuf[:B, :100].double().cpu() - h_ref).abs().max()) <= 1e-4
    comm.destroy()
