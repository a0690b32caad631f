"""``--clip_norm`` without a GPU: ``ops/clip.py``'s definition and flag handling,
``ops.optim.clip_by_global_norm_``'s CPU branch against float64, and the refusals."""
import types

import pytest
import torch

import optim_reference as R
from distributedtensorflowexample_amd.ops import clip, optim


def _cli(args):
    import main as main_mod

    main_mod.FLAGS.reset()
    try:
        return main_mod.main(["main.py"] + args)
    finally:
        main_mod.FLAGS.reset()


@pytest.mark.parametrize("pre", [1.0, 0.5])
@pytest.mark.parametrize("ratio", [0.5, 2.0])
@pytest.mark.parametrize("n", [1, 3, 1025])
def test_definition_and_cpu_branch(n, ratio, pre):
    """Bound: the f32 norm and two roundings per element -- ``bound(2, ref)``."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(n))
    norm = pre * float(g.double().norm())
    c = ratio * norm
    ref, ref_norm = clip.clip(g, c, pre)
    want = g.double() * pre * min(1.0, ratio)  # clipped: the norm becomes c; else untouched
    assert float((ref - want).abs().max()) <= 1e-15 * float(want.abs().max())
    got, gn = g.clone(), torch.zeros(1)
    optim.clip_by_global_norm_(got, c, None, pre=pre, gnorm=gn)
    assert float((got.double() - ref).abs().max()) <= R.bound(2, ref)
    assert abs(float(gn) - norm) <= R.bound(2, torch.tensor([norm]))
    if ratio > 1.0 and pre == 1.0:
        assert torch.equal(got, g)


def test_flag_validation():
    ns = types.SimpleNamespace
    assert clip.from_flags(ns()) is None and clip.from_flags(ns(clip_norm=0.0)) is None
    assert clip.from_flags(ns(clip_norm=1.5)) == 1.5 and clip.num_partials(79510) == 78
    for bad in (-1.0, float("inf"), float("nan"), "x"):
        with pytest.raises(ValueError, match="--clip_norm"):
            clip.from_flags(ns(clip_norm=bad))


@pytest.mark.parametrize("args, msg", [
    (["--strategy", "ps_async", "--job_name", "worker"], "--strategy ps_async"),
    (["--strategy", "mirrored", "--model", "bert"], "--model bert"),
    (["--strategy", "mirrored", "--model", "resnet50"], "--model resnet50"),
    (["--strategy", "mirrored", "--zero1"], "--zero1"),
])
def test_main_refuses_as_system_exit(tmp_path, monkeypatch, args, msg):
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit) as e:
        _cli(args + ["--clip_norm", "1.0", "--device", "cpu", "--logdir", str(tmp_path / "no")])
    assert msg in str(e.value) and "--clip_norm" in str(e.value), str(e.value)


@pytest.mark.parametrize("kw, msg", [
    (dict(world_size=2, fused_comm=object()), "exchange engines"),
    (dict(world_size=2, factor_comm=object()), "exchange engines"),
    (dict(pipeline=False), "pipeline=False"),
    (dict(clip_norm=-1.0), "finite and > 0"),
])
def test_trainer_refuses_before_it_touches_a_device(kw, msg):
    from distributedtensorflowexample_amd.train.fused_mlp import FusedMLPTrainer

    p, x, y = torch.zeros(79510), torch.zeros(100, 784), torch.zeros(100, dtype=torch.int32)
    with pytest.raises(ValueError, match=msg):
        FusedMLPTrainer(p, x, y, 100, 0.1, **dict(dict(clip_norm=1.0), **kw))
