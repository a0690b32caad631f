"""``--job_name eval``: evaluate the latest checkpoint of a log directory on the test set.

    python main.py --job_name eval --logdir DIR [--data_dir ...] [--device auto|cuda|cpu]
                   [--eval_output FILE.npy] [--activation sigmoid|relu|tanh] [--eval_ema]

No server and no process group is started.  The checkpoint (TF V2 bundle with the
reference's variable names, train/saver.py) is restored into the flat parameter buffer and
run through ``ops.mlp_eval.evaluate``: the fused one-launch kernel on a GPU, the CPU path of
the same op with ``--device cpu`` (or on a machine without a GPU).  Prints the checkpoint's
global step, the test accuracy, the test loss and the 10 x 10 confusion matrix
([label][predicted]); ``--eval_output`` saves the int32 predictions.

``--activation`` is the model's hidden activation and must match the training run: a checkpoint
keeps the reference's variable names and does not record it.

``--eval_ema`` evaluates the averaged variables of a ``--ema_decay`` run
(``<variable>/ExponentialMovingAverage``, ops/ema.py) instead of the raw ones, and fails with a
message when the checkpoint has none.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from ..data.mnist import read_test_set
from ..ops import ema as ema_mod
from ..ops import hidden_act, mlp_eval, mlp_step
from .saver import latest_checkpoint, load_checkpoint
from .worker import FUSED_TF_SHAPES, REFERENCE_MLP_NAMES, tf_vars_to_flat

STEP_NAME = "global/global_step"


def restore_flat(logdir, ema=False):
    """(flat parameters on the CPU, global step, checkpoint prefix) of ``logdir``'s latest
    checkpoint; ``SystemExit`` with a message when there is none or it is not the reference
    784-100-10 model.  ``ema``: the averaged variables instead (``--eval_ema``); a checkpoint
    without them -- a run without ``--ema_decay`` -- is refused."""
    prefix = latest_checkpoint(logdir)
    if prefix is None:
        raise SystemExit("eval: no checkpoint in %r" % logdir)
    values = load_checkpoint(prefix)
    if ema:
        names = [ema_mod.tf_name(n) for n in REFERENCE_MLP_NAMES]
        missing = [n for n in names if n not in values]
        if missing:
            raise SystemExit("eval: --eval_ema: checkpoint %s has no averaged variables (%s is "
                             "missing); train with --ema_decay, or evaluate without --eval_ema"
                             % (prefix, missing[0]))
        values = dict(values, **{n: values[a] for n, a in zip(REFERENCE_MLP_NAMES, names)})
    for name, shape in zip(REFERENCE_MLP_NAMES, FUSED_TF_SHAPES):
        if name not in values:
            raise SystemExit("eval: checkpoint %s lacks variable %r" % (prefix, name))
        if tuple(values[name].shape) != tuple(shape):
            raise SystemExit("eval: checkpoint %s holds %s shaped %s, the reference 784-100-10 "
                             "model needs %s" % (prefix, name, tuple(values[name].shape),
                                                 tuple(shape)))
    flat = tf_vars_to_flat({k: values[k].float() for k in REFERENCE_MLP_NAMES},
                           torch.zeros(mlp_step.NPARAM))
    step = int(values[STEP_NAME]) if STEP_NAME in values else 0
    return flat, step, prefix


def eval_job(flags, log=print):
    try:
        act = hidden_act.from_flags(flags)
    except ValueError as e:
        raise SystemExit(str(e))
    use_ema = bool(getattr(flags, "eval_ema", False))
    flat, step, _ = restore_flat(flags.logdir, ema=use_ema)
    want = str(getattr(flags, "device", "auto") or "auto")
    if want == "auto":
        want = "cuda" if torch.cuda.is_available() else "cpu"
    dev = torch.device(want)
    test = read_test_set(flags.data_dir or None)
    x = torch.from_numpy(np.ascontiguousarray(test.images, np.float32)).to(dev)
    y = torch.from_numpy(np.asarray(test.labels).astype(np.int32)).to(dev)
    out = str(getattr(flags, "eval_output", "") or "")
    res = mlp_eval.evaluate(flat.to(dev), x, y, predictions=bool(out), activation=act)
    log("global_step: {}".format(step))
    if use_ema:
        log("variables: moving averages (ExponentialMovingAverage)")
    if act != hidden_act.DEFAULT:
        log("activation: {}".format(act))
    log("test accuracy: {}".format(res.accuracy))
    log("test loss: {}".format(res.loss))
    log("confusion matrix (rows: label, columns: predicted):")
    for row in res.confusion.tolist():
        log(" ".join("%5d" % v for v in row))
    if out:
        np.save(out, res.pred.cpu().numpy().astype(np.int32))
    sys.stdout.flush()
    return 0
