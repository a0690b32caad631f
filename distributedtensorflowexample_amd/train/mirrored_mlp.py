"""Sync data-parallel training loop of the reference MLP (``--strategy mirrored``).

One process per GPU (env RANK / WORLD_SIZE / LOCAL_RANK from the launcher
or torch.distributed.run).  GPU: the fused two-launch step + the native RCCL
all-reduce, hipGraph-replayed per epoch (train/fused_mlp.py).  CPU (gloo):
the autograd MnistMLP wrapped in DistributedDataParallel.

Observability mirrors the reference: ``step / cost / speed`` prints every
``log_every`` steps (speed in global steps/sec; samples/sec = speed *
batch_size * replicas), test accuracy every ``eval_every`` steps, loss and
accuracy summaries (bulk-written from the device stats ring), and chief
checkpoints in TF V2 format with the reference's variable names.
"""
from __future__ import annotations

import os
import time

import torch
import torch.distributed as dist

from ..models import mlp as mlp_model
from ..ops import dropout as dropout_mod
from ..ops import ema as ema_mod
from ..ops import hidden_act
from ..ops import lr_schedule, mlp_step, nn, optim
from ..ops import weight_decay as weight_decay_mod
from ..ops.shuffle import shuffle_index
from ..parallel import gpu_ps_optim
from ..parallel.comm import NativeComm, TorchComm
from ..parallel.watchdog import init_process_group_with_timeout, maybe_inject_fault, watch_peers
from ..optim import GradientDescentOptimizer
from ..parallel.mirrored import DistributedDataParallel
from ..parallel.sharded import ShardedOptimizer
from ..utils.summary import FileWriter
from .fused_mlp import FusedMLPTrainer
from .saver import FastSaver
from .supervisor import Supervisor
from .worker import REFERENCE_MLP_NAMES, flat_to_tf_vars, restricted_assign, tf_vars_to_flat


def _dist_env():
    return (int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")),
            int(os.environ.get("LOCAL_RANK", "0")))


def _mlp_graph(batch, lr):
    """The reference MLP's graph for the chief's Supervisor (names from a variable registry
    built like the async worker's, utils/graph.py)."""
    from .. import variables as vs
    from ..models.dense import make_ps_model
    from ..utils.graph import reference_mlp_graph
    from .worker import build_worker_variables

    gv, tv = build_worker_variables(make_ps_model("mlp", "", None), vs.VariableRegistry())
    return reference_mlp_graph(gv, tv, 0, batch_size=batch, learning_rate=lr)


def train_mirrored(flags, dataset, log=print, max_steps=None):
    rank, world, local = _dist_env()
    use_gpu = torch.cuda.is_available() and flags.device != "cpu"
    # --optimizer momentum | adam: inside the fused step on the GPU (train/fused_mlp.py), ops/
    # optim.py's CPU branches on the autograd path; the slot variables join the checkpoints
    # under TF's names (global/dense/kernel/Momentum, .../Adam, .../Adam_1, ...)
    opt_kind = gpu_ps_optim.check_kind(getattr(flags, "optimizer", "sgd"))
    opt_kw = dict(momentum=float(getattr(flags, "momentum", gpu_ps_optim.DEFAULTS["momentum"])),
                  beta1=float(getattr(flags, "adam_beta1", gpu_ps_optim.DEFAULTS["beta1"])),
                  beta2=float(getattr(flags, "adam_beta2", gpu_ps_optim.DEFAULTS["beta2"])),
                  epsilon=float(getattr(flags, "adam_epsilon", gpu_ps_optim.DEFAULTS["epsilon"])))
    if opt_kind != "sgd" and getattr(flags, "zero1", False):
        raise ValueError("--optimizer %s does not support --zero1: the sharded update applies "
                         "gradient descent only" % opt_kind)
    # --lr_schedule: on the device in the fused step / the all-reduce engine (train/fused_mlp.py),
    # LRSchedule.value_f32 per step on the autograd path; a pure function of global_step, so a
    # restored run continues on the curve and checkpoints hold nothing new
    sched = lr_schedule.from_flags(flags)
    if sched is not None and getattr(flags, "zero1", False):
        lr_schedule.refuse(flags, "--zero1 (the sharded update)")
    # --dropout: in the fused step's head / the all-reduce engine's (train/fused_mlp.py), the
    # same mask on the autograd path; a pure function of (seed, global_step, rank, row, unit)
    drop_rate = dropout_mod.check_rate(getattr(flags, "dropout", 0.0) or 0.0)
    drop_seed = int(getattr(flags, "dropout_seed", 0) or 0)
    if drop_rate and getattr(flags, "zero1", False):
        raise ValueError("--dropout does not support --zero1 (the sharded update)")
    drop = dropout_mod.resolve(drop_rate, drop_seed, rank)
    # --weight_decay / --adamw / --nesterov: in the fused step's first launch / the all-reduce
    # engine's ops.optim call (train/fused_mlp.py), the same ops.optim arguments on the autograd
    # path; no new state, so checkpoints hold nothing new
    decay = weight_decay_mod.from_flags(flags)
    if decay is not None and getattr(flags, "zero1", False):
        weight_decay_mod.refuse(flags, "--zero1 (the sharded update)")
    # --activation: the hidden activation of the fused step's head, the evaluation kernel and the
    # autograd path (ops/hidden_act.py); a checkpoint does not record it
    act = hidden_act.from_flags(flags)
    # --ema_decay / --ema_num_updates: the shadow plane inside the fused step's first launch / the
    # all-reduce engine's ops.optim.ema_ call (train/fused_mlp.py), the same op on the autograd
    # path; checkpoints carry the shadows as <variable>/ExponentialMovingAverage.  --eval_ema: the
    # periodic test evaluation reads them
    avg = ema_mod.from_flags(flags)
    # (main.py validates the flags once for the CLI; this guard is for callers that embed
    # train_mirrored with their own namespace, as the sibling guards above: the sharded update
    # below would otherwise train without ever touching the shadow)
    if avg is not None and getattr(flags, "zero1", False):
        ema_mod.refuse(flags, "--zero1 (the sharded update)")
    eval_ema = bool(getattr(flags, "eval_ema", False))
    if world > 1 and not dist.is_initialized():
        init_process_group_with_timeout(  # control plane; tensors over RCCL on GPU
            "gloo", getattr(flags, "dist_timeout_secs", None))
    shared_gpu = os.environ.get("DTFX_SHARED_GPU") == "1"
    if use_gpu:
        # DTFX_SHARED_GPU=1 (rehearsal on a one-GPU box only): every rank on device 0 and an
        # xGMI-IPC communicator in place of RCCL, which refuses two ranks on one GPU
        local = 0 if shared_gpu else local
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
        comm = None
        if world > 1 and shared_gpu:
            from ..parallel.xgmi import XgmiComm

            comm = XgmiComm(rank, world, mlp_step.NPARAM, device=dev, key="dtfx/mirrored/shared",
                            protocol="push", timeout_s=120.0)
        elif world > 1:
            comm = NativeComm.from_process_group()
        if getattr(flags, "zero1", False) and world > 1:
            # the fused GPU engines exchange gradients inside their kernels; a 1/N-sharded
            # update of a 318 KB model would only add two collectives per step
            raise ValueError("--zero1 is implemented on the autograd (CPU) mirrored path; the "
                             "fused GPU MLP engines replicate the update")
        if (comm is not None and not shared_gpu
                and os.environ.get("DTFX_MLP_COMM", "auto") != "rccl"):
            # the 318 KB gradient is latency bound: xGMI one-shot when verified and faster
            from ..parallel.select import pick_small_allreduce

            comm, _ = pick_small_allreduce(comm, "auto", world, rank, dev)
    else:
        dev = torch.device("cpu")
        comm = TorchComm() if world > 1 else None
    is_chief = rank == 0
    steps_total = int(flags.training_steps if max_steps is None else max_steps)
    B = int(flags.batch_size)
    # --shuffle: every replica's shard in a new order each epoch (ops/shuffle.py: a pure
    # function of seed and epoch, the same on the GPU engines and the autograd path)
    shuffle = bool(getattr(flags, "shuffle", False))
    shuffle_seed = int(getattr(flags, "shuffle_seed", 0) or 0)

    params = mlp_model.init_params(dev, seed=int(flags.seed))  # identical on every rank
    # each replica trains on its own shard of the (shuffled) training set
    tr_x = torch.from_numpy(dataset.train.images[rank::world]).float()
    tr_y = torch.from_numpy(dataset.train.labels[rank::world])
    tr_y = (tr_y.argmax(1) if tr_y.ndim == 2 else tr_y).to(torch.int32)

    writer = FileWriter(flags.logdir + "_%d" % rank) if is_chief else None
    # host mirror of global_step, advanced by the training loop only: the Supervisor's
    # service threads read it instead of touching trainer/device state
    state = {"step": 0}

    if use_gpu:
        fused = factor = x_all = None
        pipe = True
        if (comm is not None and os.environ.get("DTFX_MLP_COMM", "auto") != "rccl"
                and opt_kind == "sgd" and sched is None and drop is None and decay is None
                and act == "sigmoid" and avg is None):
            # exchange engine (fused into the backward kernel / factor all-gather) when
            # verified and faster than the all-reduce engine (sgd at a constant rate without
            # dropout or weight decay and the sigmoid head only: with an optimizer, a schedule,
            # --dropout, --weight_decay, --activation relu | tanh or --ema_decay the all-reduce
            # engine it is)
            from ..parallel.select import pick_mlp_engine

            if world <= 8:
                # every process holds the whole training set (like every reference
                # process, main.py:43-44): equal-length shards of all ranks, resident
                n = min(len(dataset.train.images[q::world]) for q in range(world))
                x_all = torch.stack([torch.from_numpy(dataset.train.images[q::world][:n]).float()
                                     for q in range(world)]).to(dev).contiguous()
                tr_x, tr_y = x_all[rank], tr_y[:n]
            kind, c, _ = pick_mlp_engine(params, tr_x.to(dev), tr_y.to(dev), B,
                                         flags.learning_rate, comm, world, rank, dev, x_all=x_all,
                                         mode=os.environ.get("DTFX_MLP_ENGINE", "auto"))
            fused = c if kind in ("fused", "fused2", "fused2x") else None
            factor = c if kind in ("factor", "factor2") else None
            pipe = kind not in ("fused", "factor")  # fused2 / factor2: two-launch variants
        tr = FusedMLPTrainer(params, tr_x, tr_y, B, flags.learning_rate,
                             allreduce=comm.allreduce_sum_ if (comm and not (fused or factor))
                             else None, world_size=world, fused_comm=fused, factor_comm=factor,
                             x_all=x_all if factor is not None else None, rank=rank,
                             pipeline=pipe if comm is not None else True,
                             shuffle=shuffle, shuffle_seed=shuffle_seed, optimizer=opt_kind,
                             lr_schedule=sched, dropout=drop_rate, dropout_seed=drop_seed,
                             weight_decay=decay.wd if decay else 0.0,
                             adamw=decay.adamw if decay else True,
                             nesterov=decay.nesterov if decay else False, activation=act,
                             ema_decay=avg.decay if avg else 0.0,
                             ema_num_updates=avg.num_updates if avg else False, **opt_kw)
        # tr.snapshot() never starts a peer exchange on ONE rank and never changes the
        # replicas' update sequence (the all-reduce engine's pending gradient is applied to a
        # copy); the pipelined exchange engines have nothing pending at the checkpoint /
        # eval / replica-check points, because the loop below reads each chunk's stats on
        # EVERY rank (stats_range flushes there, collectively)
        get_params = tr.snapshot
        # (parameters, [slot planes], shadow plane or None)
        get_state = lambda: (tr.snapshot(with_slots=True, with_ema=True) if avg is not None  # noqa: E731
                             else tr.snapshot(with_slots=True) + (None,))
        step_fn = None
    else:
        model = mlp_model.MnistMLP(flat=params, activation=act)
        zero1 = bool(getattr(flags, "zero1", False)) and comm is not None
        ddp = DistributedDataParallel(model, comm, shard=zero1) if comm else None
        zopt = (ShardedOptimizer(GradientDescentOptimizer(flags.learning_rate), ddp)
                if zero1 else None)
        state["pos"] = 0
        get_params = lambda: model.flat.detach().clone()  # noqa: E731
        cpu_slots = [torch.zeros(mlp_step.NPARAM)
                     for _ in range(gpu_ps_optim.num_slots(opt_kind))]
        cpu_shadow = model.flat.detach().clone() if avg is not None else None  # shadow_0 = p_0
        get_state = lambda: (get_params(), [t.clone() for t in cpu_slots],  # noqa: E731
                             None if cpu_shadow is None else cpu_shadow.clone())

        def step_fn():
            i = state["pos"]
            n = tr_x.shape[0] // B
            if shuffle:  # position j of epoch e holds original row shuffle_index(seed, e, rows)[j]
                e = i // n
                if state.get("epoch") != e:
                    state["epoch"], state["perm"] = e, shuffle_index(shuffle_seed, e,
                                                                     tr_x.shape[0])
                idx = state["perm"][(i % n) * B:(i % n + 1) * B]
                xb, yb = tr_x[idx], tr_y[idx]
            else:
                xb, yb = tr_x[(i % n) * B:(i % n + 1) * B], tr_y[(i % n) * B:(i % n + 1) * B]
            state["pos"] = i + 1
            if ddp:
                ddp.reset()
            else:
                model.flat.grad = None
            if drop is None:
                loss, acc = model.loss(xb, yb)
            else:  # the mask of step i = global_step, this replica's stream
                loss, acc = model.loss(xb, yb, keep=drop.keep_mask(i, xb.shape[0]),
                                       scale=drop.scale)
            loss.backward()
            if zopt is not None:  # reduce-scatter -> owner SGD on 1/world -> all-gather
                zopt.step()
                return float(loss), float(acc)
            if ddp:
                ddp.finish()
                g = ddp.flat_grad[:model.flat.numel()]
            else:
                g = model.flat.grad
            # the rate of step i = global_step (the device arithmetic, emulated in f32)
            lr = (flags.learning_rate if sched is None
                  else float(sched.value_f32(flags.learning_rate, i)))
            state["rates"].append(lr)
            with torch.no_grad():
                if opt_kind == "momentum":
                    optim.momentum_(model.flat.data, g, cpu_slots[0], lr,
                                    momentum=opt_kw["momentum"],
                                    **(decay.momentum_kw if decay else {}))
                elif opt_kind == "adam":  # t = global_step + 1 of this step
                    optim.adam_(model.flat.data, g, cpu_slots[0], cpu_slots[1],
                                lr, i + 1, beta1=opt_kw["beta1"],
                                beta2=opt_kw["beta2"], eps=opt_kw["epsilon"],
                                **(decay.adam_kw if decay
                                   else dict(weight_decay=0.0, adamw=False)))
                else:
                    optim.sgd_(model.flat.data, g, lr, **(decay.sgd_kw if decay else {}))
                if avg is not None:  # after the update; t = global_step + 1 of this step
                    optim.ema_(cpu_shadow, model.flat.data, avg, step=i + 1)
            return float(loss), float(acc)

    # one name tuple per slot plane, kernels in TF layout like the variables themselves
    slot_names = [tuple(n) for n in gpu_ps_optim.slot_names(opt_kind, REFERENCE_MLP_NAMES)]
    var_names = (list(REFERENCE_MLP_NAMES) + [n for names in slot_names for n in names]
                 + ["global/global_step"])
    saver = FastSaver({n: None for n in var_names})
    # the averaged variables under TF's names (kernels in TF layout like the variables); not in
    # the saver's var list, which is what a restore REQUIRES: a checkpoint without them (a run
    # without --ema_decay) restores, and the shadow then starts at the restored parameters
    ema_names = tuple(ema_mod.tf_name(n) for n in REFERENCE_MLP_NAMES) if avg is not None else ()

    def save_vars():
        p, slots, shadow = get_state()
        v = {k: t.contiguous() for k, t in flat_to_tf_vars(p.cpu()).items()}
        for names, plane in zip(slot_names, slots):
            v.update({k: t.contiguous() for k, t in flat_to_tf_vars(plane.cpu(), names).items()})
        if shadow is not None:
            v.update({k: t.contiguous()
                      for k, t in flat_to_tf_vars(shadow.cpu(), ema_names).items()})
        v["global/global_step"] = torch.tensor(global_step(), dtype=torch.int32)
        return v

    def global_step():
        return tr.global_step() if use_gpu else state.get("pos", 0)

    def published_step():
        return state["step"]

    def restore(values):
        p = torch.zeros(mlp_step.NPARAM)
        tf_vars_to_flat(values, p)
        # (a checkpoint that lacks this optimizer's slot variables -- an sgd run's, another
        # optimizer's -- never gets here: FastSaver.restore raises KeyError over its var list,
        # as TF's restore and the GPU parameter store's path do)
        planes = [tf_vars_to_flat(values, torch.zeros(mlp_step.NPARAM), names)
                  for names in slot_names]
        shadow = None
        if avg is not None:  # the checkpoint's shadows, or the restored parameters
            shadow = (tf_vars_to_flat(values, torch.zeros(mlp_step.NPARAM), ema_names)
                      if all(n in values for n in ema_names) else p.clone())
        if use_gpu:
            tr.load_params(p.to(dev))
            tr.load_slots([t.to(dev) for t in planes])
            if shadow is not None:
                tr.load_ema(shadow.to(dev))
            tr.seek(int(values["global/global_step"]))
        else:
            model.flat.data.copy_(p)
            for d, t in zip(cpu_slots, planes):
                d.copy_(t)
            if shadow is not None:
                cpu_shadow.copy_(shadow)
            state["pos"] = int(values["global/global_step"])
        state["step"] = int(values["global/global_step"])

    # (the var list only: an sgd run restoring a momentum / Adam checkpoint ignores the slots)
    saver.assign = restricted_assign(restore, var_names + list(ema_names))
    # checkpoints are taken by the training loop between chunks (Supervisor.service): the
    # fused trainer's deferred update may only be flushed where every rank flushes it
    sv = Supervisor(is_chief=is_chief, logdir=flags.logdir if is_chief else None,
                    saver=saver if is_chief else None, summary_writer=writer,
                    global_step=published_step, save_model_secs=flags.save_model_secs,
                    save_summaries_secs=flags.save_summaries_secs, save_variables=save_vars,
                    checkpoint_on_main_thread=True, graph=_mlp_graph(B, flags.learning_rate))

    test_x = torch.from_numpy(dataset.test.images).float().to(dev)
    test_y = dataset.test.labels.argmax(1) if dataset.test.labels.ndim == 2 else dataset.test.labels

    test_y_dev = torch.from_numpy(test_y.astype("int32")).to(dev) if use_gpu else None
    eval_summaries = bool(getattr(flags, "eval_summaries", False))

    def test_eval():
        """(test accuracy, test loss or None): on the GPU the one-launch evaluation kernel
        (ops/mlp_eval.py) through the trainer; the CPU autograd path keeps the generic
        forward (and computes the loss only where --eval_summaries asks for it)."""
        if use_gpu:
            res = tr.evaluate(test_x, test_y_dev, ema=eval_ema)
            return float(res.accuracy), float(res.loss)
        p = cpu_shadow.clone() if eval_ema else get_params()
        W1t, b1, W2t, b2 = mlp_step.unflatten(p)
        if act == "tanh":  # (not an epilogue of the generic GEMM)
            h = torch.tanh(nn.gemm(test_x, W1t, trans_b=True, bias=b1))
        else:
            h = nn.gemm(test_x, W1t, trans_b=True, bias=b1, act=act)
        logits = nn.gemm(h, W2t, trans_b=True, bias=b2)
        acc = float((logits.argmax(1).cpu().numpy() == test_y).mean())
        if not eval_summaries:
            return acc, None
        lab = torch.from_numpy(test_y.astype("int64"))
        loss = (torch.logsumexp(logits, 1) - logits.gather(1, lab[:, None])[:, 0]).mean()
        return acc, float(loss)

    history = []
    # fail-fast: a rank whose peer died aborts its communicator and exits (non-zero)
    with watch_peers(comm, float(getattr(flags, "peer_timeout_secs", 60.0) or 0.0)), \
            sv.managed_session():
        if world > 1 and sv.restored_from is not None:
            pass  # chief-only restore: other ranks broadcast below
        if world > 1:  # replicas start identical (restored or initialised on the chief)
            p = get_params()
            if comm is not None:
                comm.broadcast_(p, 0)
            # ... at the chief's global step (a restored chief resumes mid-run; the other
            # ranks must run exactly as many steps, or they wait in a collective forever)
            s = torch.tensor([global_step()], dtype=torch.int64)
            dist.broadcast(s, 0)
            s = int(s.item())
            planes = [t.clone() for t in (tr.slots if use_gpu else cpu_slots)]
            if avg is not None:  # (... and its shadow plane, with the slots)
                planes.append((tr.ema if use_gpu else cpu_shadow).clone())
            if comm is not None:  # (a restored chief's slot planes)
                for t in planes:
                    comm.broadcast_(t, 0)
            shadow = planes.pop() if avg is not None else None
            if use_gpu:
                tr.load_params(p)
                tr.load_slots(planes)
                if shadow is not None:
                    tr.load_ema(shadow)
                tr.seek(s)
            else:
                model.flat.data.copy_(p)
                for d, t in zip(cpu_slots, planes):
                    d.copy_(t)
                if shadow is not None:
                    cpu_shadow.copy_(shadow)
                state["pos"] = s
        chunk = int(flags.log_every)
        state["step"] = global_step()
        start_time, start_step = time.time(), state["step"]
        while not sv.should_stop():
            s0 = global_step()
            n = min(chunk - (s0 % chunk) if s0 % chunk else chunk, steps_total - s0)
            if n <= 0:
                break
            if use_gpu:
                tr.run(n)
                stats = tr.stats_range(s0, s0 + n)
                rates = tr.learning_rates(s0, s0 + n).tolist() if sched is not None else None
            else:
                state["rates"] = []
                stats = torch.tensor([step_fn() for _ in range(n)])
                rates = state["rates"] if sched is not None else None
            step = global_step()
            state["step"] = step
            maybe_inject_fault(rank, step)
            if writer is not None:
                writer.add_scalar_series(["loss", "accuracy"], range(s0, s0 + n), stats.tolist())
                if rates is not None:  # the rate each step applied
                    writer.add_scalar_series(["learning_rate"], range(s0, s0 + n),
                                             [[r] for r in rates])
            cost = float(stats[-1, 0])
            history.append((step, cost, float(stats[-1, 1])))
            if is_chief and step % chunk == 0:
                if use_gpu:
                    torch.cuda.synchronize()
                elapsed = time.time() - start_time
                log("step: {}\t| cost: {}\t| speed: {}step/sec".format(
                    step, cost, float((step - start_step) / max(elapsed, 1e-9))))
                start_time, start_step = time.time(), step
            if is_chief and step % int(flags.eval_every) == 0:
                t_acc, t_loss = test_eval()
                log("test accuracy: {}".format(t_acc))
                if eval_summaries and writer is not None:
                    writer.add_scalars({"test_loss": t_loss, "test_accuracy": t_acc}, step)
            k = int(getattr(flags, "check_replicas_every", 0) or 0)
            if k > 0 and world > 1 and step % k == 0:
                from ..parallel.mirrored import assert_replicas_identical

                assert_replicas_identical(comm, get_params(), world, step)
            sv.service()  # a requested checkpoint, on this thread, between chunks
            if step >= steps_total:
                break
        if is_chief:
            sv.save_checkpoint()
    return history, get_params()


def shutdown_mirrored():
    """Orderly end of a mirrored run (the CLI's, main.py): every rank -- the chief's final
    checkpoint included -- reaches a barrier before any process group goes away.  A rank that
    exited while the store-hosting chief was still tearing its gloo group down died in
    std::terminate at interpreter exit now and then (tests/test_cluster_e2e.py, frequent
    checkpoints)."""
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
