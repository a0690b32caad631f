"""Hidden-layer dropout (``ops/dropout.py``) on the CPU: the mask against ``philox_reference``,
the threshold / scale arithmetic, ``MnistMLP.loss(keep=...)`` against ``dropout_reference`` in
float64, the mirrored CPU loop (deterministic, resumes from a checkpoint in the same mask
sequence), the flags and the refusals, and the float64 figures the GPU tests rely on."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import dropout_reference as dr
import philox_reference as pr
from distributedtensorflowexample_amd import flags as F
from distributedtensorflowexample_amd.ops import dropout, mlp_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the mask ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, step, stream, B", [
    (5, 0, 0, 1), (5, 3, 0, 17), (5, 6, 1, 100), (0, 2 ** 31 - 2, 0, 113),
    ((1 << 63) + (7 << 32) + 9, 2 ** 31 - 1, 7, 256), ((3 << 40) + 1, 1 << 30, (1 << 32) - 1, 17),
])
@pytest.mark.parametrize("rate", [0.5, 0.1])
def test_keep_mask_is_the_reference_philox(seed, step, stream, B, rate):
    w = pr.words(B * 100, seed, (stream << 32) | step).reshape(-1)[:B * 100].reshape(B, 100)
    assert np.array_equal(dropout.mask_words(seed, step, stream, B), w)
    thr = int(round((1.0 - rate) * 2.0 ** 24))
    want = torch.from_numpy((w >> np.uint32(8)).astype(np.int64) < thr)
    got = dropout.keep_mask(seed, step, stream, B, rate)
    assert got.dtype == torch.bool and tuple(got.shape) == (B, 100)
    assert torch.equal(got, want) and torch.equal(got, dr.keep_mask(seed, step, stream, B, rate))
    d = dropout.Dropout(rate, seed, stream)
    assert torch.equal(d.keep_mask(step, B), want)
    assert d.args() == (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, thr, stream, d.scale)


def test_masks_differ_by_step_and_stream_and_keep_about_q():
    a = dropout.keep_mask(5, 0, 0, 256, 0.5)
    assert not torch.equal(a, dropout.keep_mask(5, 1, 0, 256, 0.5))
    assert not torch.equal(a, dropout.keep_mask(5, 0, 1, 256, 0.5))
    assert not torch.equal(a, dropout.keep_mask(6, 0, 0, 256, 0.5))
    for rate in (0.5, 0.1):  # 25,600 draws: 6 sigma of a binomial share
        q = 1.0 - rate
        share = float(dropout.keep_mask(5, 0, 0, 256, rate).float().mean())
        assert abs(share - q) < 6.0 * (q * (1 - q) / 25600) ** 0.5


def test_threshold_and_scale():
    assert dropout.threshold(0.0) == (1 << 24, 1.0)
    assert dropout.threshold(0.5) == (1 << 23, 2.0)
    thr, scale = dropout.threshold(0.1)
    assert thr == 15099494 and scale == float(np.float32(2.0 ** 24 / 15099494))
    assert dropout.threshold(1.0 - 2.0 ** -24) == (1, 16777216.0)
    assert dropout.resolve(0.0) is None and dropout.resolve(0.25, 3, 2).stream == 2
    for bad in (1.0, 1.5, -0.01, float("nan")):
        with pytest.raises(ValueError, match="dropout rate must be in"):
            dropout.threshold(bad)
    with pytest.raises(ValueError, match="keeps nothing"):
        dropout.threshold(1.0 - 2.0 ** -26)


# ---- the autograd path ---------------------------------------------------------------------------
@pytest.mark.parametrize("B, rate", [(1, 0.5), (17, 0.1), (100, 0.5)])
def test_mlp_loss_with_keep_matches_float64_reference(B, rate):
    from distributedtensorflowexample_amd.models.mlp import MnistMLP

    p, x, y = dr.data(B)
    keep = dr.keep_mask(dr.SEED, 4, 0, B, rate)
    _, scale = dr.threshold(rate)
    ref = dr.step(p, x[:B], y[:B], keep, scale)
    model = MnistMLP(flat=p.double().clone())
    loss, acc = model.loss(x[:B].double(), y[:B], keep=keep, scale=scale)
    loss.backward()
    assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-12
    # (the op returns the accuracy as an f32 mean)
    assert float(acc.detach()) == float(ref["correct"].float().mean())
    assert float((model.flat.grad - ref["grad"]).abs().max()) <= 1e-12
    plain = MnistMLP(flat=p.double().clone())
    l0, _ = plain.loss(x[:B].double(), y[:B])
    g0, l0_ref, _ = mlp_step.reference_step(p.double(), x[:B].double(), y[:B])
    l0, loss = float(l0.detach()), float(loss.detach())
    assert abs(l0 - float(l0_ref)) <= 1e-12 and abs(l0 - loss) > 1e-6


# ---- flags and refusals --------------------------------------------------------------------------
def test_flags_defaults_and_values():
    fv = F.FlagValues()
    F.define_reference_flags(fv)
    fv(["main.py"])
    assert fv.dropout == 0.0 and fv.dropout_seed == 0
    fv.reset()
    fv(["main.py", "--dropout", "0.5", "--dropout_seed=5"])
    assert fv.dropout == 0.5 and fv.dropout_seed == 5


def _wflags(**kw):
    d = dict(batch_size=100, learning_rate=0.05, training_steps=10, logdir="unused",
             use_locking=False, seed=0, ps_device="cpu", num_workers=1, sync_replicas=False,
             optimizer="sgd", dropout=0.5, dropout_seed=5)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_ps_async_worker_refuses(tmp_path, monkeypatch):
    from distributedtensorflowexample_amd.train.worker import Worker

    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="--dropout: --strategy ps_async"):
        Worker("worker", 0, None, _wflags(), device="cpu")
    assert os.listdir(str(tmp_path)) == []


def test_bert_and_resnet_refuse(tmp_path, monkeypatch):
    from distributedtensorflowexample_amd.train.mirrored_models import train_model_mirrored

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    for model in ("bert", "resnet50"):
        with pytest.raises(ValueError, match="--dropout: --model %s" % model):
            train_model_mirrored(_wflags(model=model, device="cpu", logdir=str(tmp_path / "m")))
    assert os.listdir(str(tmp_path)) == []


def test_cli_refuses_and_eval_ignores(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}

    def main(args):
        return subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, env=env,
                              cwd=ROOT, capture_output=True, text=True, timeout=240)

    r = main(["--strategy", "ps_async", "--job_name", "worker", "--dropout", "0.5", "--logdir",
              str(tmp_path / "no")])
    assert r.returncode != 0 and "--dropout: --strategy ps_async" in r.stderr, r.stderr
    r = main(["--strategy", "mirrored", "--dropout", "1.0", "--device", "cpu", "--logdir",
              str(tmp_path / "no")])
    assert r.returncode != 0 and "dropout rate must be in [0, 1)" in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "no"))
    # the eval job never drops and does not look at the flag: it fails on the missing checkpoint,
    # not on --dropout
    r = main(["--job_name", "eval", "--dropout", "0.5", "--device", "cpu", "--logdir",
              str(tmp_path / "empty")])
    assert "--dropout" not in r.stderr, r.stderr


def test_trainer_refuses_before_touching_anything():
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = torch.zeros(mlp_step.NPARAM), torch.zeros(300, 784), torch.zeros(300).int()
    with pytest.raises(ValueError, match="dropout: the exchange engines"):
        FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, fused_comm=object(), dropout=0.5)
    with pytest.raises(ValueError, match="dropout: the exchange engines"):
        FusedMLPTrainer(p, x, y, 100, 0.1, world_size=2, factor_comm=object(), dropout=0.5)
    with pytest.raises(ValueError, match="dropout rate must be in"):
        FusedMLPTrainer(p, x, y, 100, 0.1, dropout=1.0)
    with pytest.raises(ValueError, match="runs on the GPU"):  # rate 0: the usual CPU refusal
        FusedMLPTrainer(p, x, y, 100, 0.1, dropout=0.0)


# ---- the mirrored CPU loop -----------------------------------------------------------------------
B, STEPS, LR = 16, 12, 0.3
N = 5 * B + 7


def _dataset():
    from distributedtensorflowexample_amd.data.mnist import DataSet, DataSets

    g = torch.Generator().manual_seed(3)
    x = torch.rand(N, 784, generator=g).numpy()
    y = torch.randint(0, 10, (N,), generator=g).numpy().astype(np.uint8)
    test = DataSet(x[:8], y[:8], one_hot=False)
    return DataSets(train=DataSet(x, y, one_hot=False), validation=test, test=test,
                    synthetic_train=True)


def _run(tmp_path, tag, steps=STEPS, **kw):
    from distributedtensorflowexample_amd.train.mirrored_mlp import train_mirrored

    fl = types.SimpleNamespace(batch_size=B, learning_rate=LR, training_steps=steps,
                               logdir=str(tmp_path / tag), log_every=1, eval_every=10 ** 9,
                               save_model_secs=1000.0, save_summaries_secs=1000.0,
                               use_locking=False, seed=0, device="cpu", **kw)
    return train_mirrored(fl, _dataset(), log=lambda *_: None)


def test_mirrored_cpu_loop_is_deterministic_and_is_the_reference(tmp_path, monkeypatch):
    """12 sgd steps with --dropout 0.5 twice: the same bits; another seed or no dropout: another
    run; and the float64 loop of ``dropout_reference.step`` with the mask of (seed, step, rank 0)
    within 4.2e-5 on the parameters.  The bound is the f32 run's own rounding: the parameters are
    N(0, 1) draws below 8, so each of the 12 updates rounds by up to half an ulp of 8 (4.8e-7) and
    carries lr = 0.3 times the f32 error of a gradient element -- a sum over 16 rows of 784
    products, 1e-5 at these magnitudes with the scale of 2 -- so 12 x (4.8e-7 + 3e-6).  A wrong
    mask moves the parameters by more than 1e-3 (asserted on the other seed)."""
    from distributedtensorflowexample_amd.models import mlp as mlp_model

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    hist, a = _run(tmp_path, "a", dropout=0.5, dropout_seed=5)
    _, b = _run(tmp_path, "b", dropout=0.5, dropout_seed=5)
    _, other = _run(tmp_path, "c", dropout=0.5, dropout_seed=6)
    _, plain = _run(tmp_path, "d")
    assert [h[0] for h in hist] == list(range(1, STEPS + 1))
    assert torch.equal(a, b)
    assert float((a - other).abs().max()) > 1e-3 and float((a - plain).abs().max()) > 1e-3
    ds = _dataset()
    x = torch.from_numpy(ds.train.images).double()
    y = torch.from_numpy(ds.train.labels).int()
    p = mlp_model.init_params("cpu", seed=0).double()
    nb = N // B
    for s in range(STEPS):
        sl = slice((s % nb) * B, (s % nb + 1) * B)
        r = dr.step(p, x[sl], y[sl], dr.keep_mask(5, s, 0, B, 0.5), 2.0)
        p = p - float(np.float32(LR)) * r["grad"]
    err = float((a.double() - p).abs().max())
    print("max |p - p64| after %d dropout steps: %.3e" % (STEPS, err))
    assert err <= 4.2e-5


def test_resume_continues_the_mask_sequence(tmp_path, monkeypatch):
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    kw = dict(dropout=0.5, dropout_seed=5)
    _, full = _run(tmp_path, "full", 10, **kw)
    _run(tmp_path, "part", 5, **kw)
    hist, cont = _run(tmp_path, "part", 10, **kw)
    assert [h[0] for h in hist] == [6, 7, 8, 9, 10]
    assert torch.equal(full, cont)
    assert not torch.equal(dropout.keep_mask(5, 5, 0, B, 0.5), dropout.keep_mask(5, 0, 0, B, 0.5))


# ---- the figures the GPU tests rely on -----------------------------------------------------------
@pytest.mark.parametrize("rate", dr.RATES)
@pytest.mark.parametrize("size", dr.SIZES)
def test_float64_preconditions_of_the_gpu_tests(size, rate):
    """Steps 0..6 at learning rate 0.01 on dropout_reference.data: every h >= 1e-3 (the smallest is
    0.0019 at batch 17; a zero in hbuf can then only be a dropped unit), every softmax probability in [0.0037, 0.70], a top-2 logit
    gap of 1e-3 or less on at most 1 % of the rows (at most 4 of the 1,792 at batch 256), and
    gradients below 2."""
    tr, _ = dr.trajectory(size, rate, 7, 0.01)
    hmin = min(float(r["h"].min()) for _, r in tr)
    pmin = min(float(r["prob"].min()) for _, r in tr)
    pmax = max(float(r["prob"].max()) for _, r in tr)
    near = sum(int((r["gap"] <= 1e-3).sum()) for _, r in tr)
    gmax = max(float(r["grad"].abs().max()) for _, r in tr)
    print("B=%d rate=%g: min h %.5f prob [%.4f, %.4f] near %d/%d max |g| %.3f"
          % (size, rate, hmin, pmin, pmax, near, 7 * size, gmax))
    assert hmin >= 1e-3 and 0.0037 <= pmin and pmax <= 0.70
    assert near <= 0.01 * 7 * size and (size != 256 or near <= 4)
    assert gmax < 2.0
