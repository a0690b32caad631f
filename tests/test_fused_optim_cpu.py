"""``--optimizer momentum | adam`` under ``--strategy mirrored`` for the MLP, CPU tier: the CLI no
longer refuses it, the autograd path applies ``ops.optim``'s CPU branches with ``t = step + 1``,
the checkpoints carry the slot variables under TF's names in TF layout, and the combinations
that stay unsupported are still refused with a message."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from distributedtensorflowexample_amd.ops import mlp_step, optim
from distributedtensorflowexample_amd.train.saver import latest_checkpoint, load_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARS = ("global/dense/kernel", "global/dense/bias", "global/dense_1/kernel",
        "global/dense_1/bias")
TF_SHAPES = ((784, 100), (100,), (100, 10), (10,))


def _main(args, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + args, env=env,
                          cwd=ROOT, capture_output=True, text=True, timeout=timeout)


def test_cli_mirrored_cpu_momentum_checkpoint_holds_slots(tmp_path):
    logdir = str(tmp_path / "mom")
    r = _main(["--strategy", "mirrored", "--device", "cpu", "--optimizer", "momentum",
               "--training_steps", "20", "--log_every", "10", "--eval_every", "1000",
               "--logdir", logdir, "--save_model_secs", "1000"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "step: 20" in r.stdout
    v = load_checkpoint(latest_checkpoint(logdir))
    assert int(v["global/global_step"]) == 20
    assert sorted(v) == sorted(list(VARS) + [k + "/Momentum" for k in VARS]
                               + ["global/global_step"])
    for k, shape in zip(VARS, TF_SHAPES):
        assert tuple(v[k].shape) == shape
        assert tuple(v[k + "/Momentum"].shape) == shape
        assert float(np.abs(np.asarray(v[k + "/Momentum"])).max()) > 0  # a used accumulator


B, STEPS, LR = 16, 12, 0.05
N = 5 * B + 7


def _dataset():
    from distributedtensorflowexample_amd.data.mnist import DataSet, DataSets

    g = torch.Generator().manual_seed(3)
    x = torch.rand(N, 784, generator=g).numpy()
    y = torch.randint(0, 10, (N,), generator=g).numpy().astype(np.uint8)
    test = DataSet(x[:8], y[:8], one_hot=False)
    return DataSets(train=DataSet(x, y, one_hot=False), validation=test, test=test,
                    synthetic_train=True)


def _run(tmp_path, tag, **kw):
    from distributedtensorflowexample_amd.train.mirrored_mlp import train_mirrored

    fl = types.SimpleNamespace(batch_size=B, learning_rate=LR, training_steps=STEPS,
                               logdir=str(tmp_path / tag), log_every=1, eval_every=10 ** 9,
                               save_model_secs=1000.0, save_summaries_secs=1000.0,
                               use_locking=False, seed=0, device="cpu", **kw)
    hist, p = train_mirrored(fl, _dataset(), log=lambda *_: None)
    assert [h[0] for h in hist] == list(range(1, STEPS + 1))
    return [h[1] for h in hist], p


@pytest.mark.parametrize("kind", ["adam", "momentum"])
def test_mirrored_cpu_trajectory_is_reference_step_plus_optim(tmp_path, monkeypatch, kind):
    """World 1, 12 steps (two epoch wraps of the 5-batch set): losses, parameters and the
    checkpointed slots equal a direct f32 loop of ``reference_step`` + ``optim.adam_`` (``t =
    step + 1``) / ``optim.momentum_``.  The two are different f32 operation sequences (autograd
    modules / explicit formulas), so the gradients agree to f32 rounding (~1e-7 relative), not
    bitwise: losses within 1e-4 relative (the suite's bound between two forward passes).  Adam
    runs with epsilon 1e-3 so that rounding of a near-zero gradient cannot flip a +-lr update:
    then d(update)/dg <= lr (1 - b1) / eps = 5, a gradient error of ~1e-8 moves a parameter by
    <= 5e-8 per step, and 12 steps stay far below the 1e-5 allowed here (a wrong t, a missing
    bias correction or a skipped slot update is >= 1e-3)."""
    from distributedtensorflowexample_amd.models import mlp as mlp_model

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    ds = _dataset()
    x = torch.from_numpy(ds.train.images).float()
    y = torch.from_numpy(ds.train.labels).int()
    p = mlp_model.init_params("cpu", seed=0).clone()
    slots = [torch.zeros_like(p) for _ in range(2 if kind == "adam" else 1)]
    nb, ref = N // B, []
    for s in range(STEPS):
        sl = slice((s % nb) * B, (s % nb + 1) * B)
        g, loss, _ = mlp_step.reference_step(p, x[sl], y[sl])
        ref.append(float(loss))
        if kind == "adam":
            optim.adam_(p, g, slots[0], slots[1], LR, s + 1, beta1=0.9, beta2=0.999, eps=1e-3,
                        weight_decay=0.0, adamw=False)
        else:
            optim.momentum_(p, g, slots[0], LR, momentum=0.9)
    kw = dict(optimizer=kind, adam_epsilon=1e-3) if kind == "adam" else dict(optimizer=kind)
    got, pg = _run(tmp_path, kind, **kw)
    sgd, ps = _run(tmp_path, "sgd")
    print(kind, "losses", got, "\nreference", ref, "\nmax |dp|", float((pg - p).abs().max()))
    for a, b in zip(got, ref):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (got, ref)
    assert float((pg - p).abs().max()) <= 1e-5
    assert float((pg - ps).abs().max()) > 1e-2  # (and it is not the sgd run)
    # the final checkpoint: slots in TF layout under TF's names
    v = load_checkpoint(latest_checkpoint(str(tmp_path / kind)))
    names = ("Adam", "Adam_1") if kind == "adam" else ("Momentum",)
    for name, plane in zip(names, slots):
        W1t, b1, W2t, b2 = mlp_step.unflatten(plane)
        for k, want in zip(VARS, (W1t.t(), b1, W2t.t(), b2)):
            have = torch.as_tensor(np.asarray(v["%s/%s" % (k, name)]))
            assert tuple(have.shape) == tuple(want.shape)
            assert float((have - want).abs().max()) <= 1e-5, (k, name)


def test_cpu_restore_rules(tmp_path, monkeypatch):
    """An Adam checkpoint restores into an Adam run (slots and t resume: the continued run
    equals the uninterrupted one bit for bit) and into an sgd run (slots ignored); an Adam run
    restoring an sgd checkpoint raises over its var list, as TF's restore and the GPU parameter
    store's path do."""
    from distributedtensorflowexample_amd.train.mirrored_mlp import train_mirrored

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)

    def run(tag, steps, **kw):
        fl = types.SimpleNamespace(batch_size=B, learning_rate=LR, training_steps=steps,
                                   logdir=str(tmp_path / tag), log_every=1, eval_every=10 ** 9,
                                   save_model_secs=1000.0, save_summaries_secs=1000.0,
                                   use_locking=False, seed=0, device="cpu", **kw)
        return train_mirrored(fl, _dataset(), log=lambda *_: None)

    _, full = run("full", 10, optimizer="adam")
    run("part", 5, optimizer="adam")
    hist, cont = run("part", 10, optimizer="adam")  # restores step 5 from its logdir
    assert [h[0] for h in hist] == [6, 7, 8, 9, 10]
    assert torch.equal(full, cont)
    hist, _ = run("part", 12, optimizer="sgd")  # the slots in the checkpoint are ignored
    assert [h[0] for h in hist] == [11, 12]
    run("plain", 3)
    with pytest.raises(KeyError, match="global/dense/kernel/Adam"):
        run("plain", 5, optimizer="adam")


@pytest.mark.parametrize("args, needle", [
    (["--model", "bert", "--optimizer", "adam"], "--model mlp"),
    (["--zero1", "--optimizer", "adam"], "--zero1"),
])
def test_cli_still_refuses(tmp_path, args, needle):
    r = _main(["--strategy", "mirrored", "--device", "cpu", "--training_steps", "2",
               "--logdir", str(tmp_path / "no")] + args)
    assert r.returncode != 0
    assert "--optimizer adam" in r.stderr and needle in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "no"))


@pytest.mark.slow
def test_mirrored_two_ranks_gloo_momentum_replicas_identical(tmp_path):
    from distributedtensorflowexample_amd.launch import launch_mirrored

    logdir = str(tmp_path / "mir")
    rc = launch_mirrored(nproc=2, log_dir=str(tmp_path / "logs"), quiet=True, timeout=240,
                         extra=["--training_steps", "40", "--log_every", "10",
                                "--eval_every", "1000", "--logdir", logdir, "--device", "cpu",
                                "--learning_rate", "0.05", "--save_model_secs", "100",
                                "--optimizer", "momentum", "--check_replicas_every", "10"])
    assert rc == {"rank0": 0, "rank1": 0}, rc
    v = load_checkpoint(latest_checkpoint(logdir))
    assert int(v["global/global_step"]) == 40
    assert float(np.abs(np.asarray(v["global/dense_1/bias/Momentum"])).max()) > 0
