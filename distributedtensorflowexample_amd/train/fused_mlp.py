"""Fused MNIST-MLP training engine: three HIP launches per step, hipGraph-replayed.

This is the MI355X-native replacement of the reference's per-step session
loop (worker.py:129-159).  Per step the reference makes three gRPC round
trips (pull 318 KB, push 318 KB + remote ApplyGradientDescent, AssignAdd),
a host->GPU feed of 317 KB and ~14 tiny TF kernels.  Here:

* the dataset is resident in HBM; each launch gets its batch's pointer, and
  one hipGraph is captured per epoch (``nbatches`` steps), so replaying it
  walks the dataset like ``next_batch`` with no host work per step;
* on one GPU the step is TWO launches (``pipeline=True``, default):
  ``mlp_fwdapply`` applies step t-1's update -- formed tile by tile from the
  factors the previous head left behind, never stored as a gradient -- and runs
  step t's forward; ``mlp_head`` finishes step t.  The last update stays pending
  until ``flush()`` (ping-pong parameter buffers, like the DP path below).
  ``pipeline=False``: the three-launch step ``mlp_fwd`` / ``mlp_head`` /
  ``mlp_wgrad`` with the SGD apply fused into ``mlp_wgrad``'s epilogue;
* in sync data-parallel mode the flat 318 KB gradient is all-reduced after
  ``mlp_wgrad`` by a pluggable ``allreduce(grad)`` callable (RCCL through
  ``torch.distributed`` or the native communicator) and applied, averaged
  through ``lr / world_size``, inside the next step's ``mlp_fwd``/``mlp_head``;
* or, with ``fused_comm`` (an ``XgmiComm`` with protocol "push"), the gradient
  exchange is fused into ``mlp_wgrad``'s epilogue (LL words pushed straight to
  the peers, gathered, summed in rank order and applied in the same launch):
  three launches per data-parallel step, no pending gradient;
* or, with ``factor_comm`` (also protocol "push") and ``x_all`` [world, n, 784]
  -- every rank's deterministic batch stream resident on every GPU, as every
  reference process loads the whole dataset (main.py:43-44) -- the ranks
  all-gather only the backprop factors dz1 (40 KB) inside ``mlp_head`` and
  each forms the global W1 gradient itself (sufficient-factor exchange);
* ``global_step`` is a device counter advanced by the kernels (AssignAdd of
  worker.py:32,141); loss/accuracy land in a device ring read back lazily;
* ``shuffle=True`` reshuffles the resident dataset at every epoch boundary, the
  first epoch included, like the reference's ``next_batch`` (worker.py:133).
  Nothing joins the step: the order is changed BETWEEN epochs.  The pristine
  dataset stays resident next to two shuffled buffers; epoch ``e = global_step
  // nbatches`` reads buffer ``e & 1``, whose position j holds original row
  ``ops.shuffle.shuffle_index(shuffle_seed, e, n)[j]`` (a pure function: a run
  resumed with ``seek(global_step)`` and every data-parallel rank reproduce it;
  with ``factor_comm`` every rank's plane of ``x_all`` is shuffled locally).
  The gather for epoch e + 1 (``csrc/kernels/shuffle.hip``) is launched in order
  on the compute stream when the position wraps, between two graph replays;
  the step kernels keep reading plain contiguous batches.  All n rows are
  permuted and the first ``nbatches * B`` positions are fed, so the dropped tail
  differs every epoch.  The update pending across a boundary reads the previous
  epoch's last batch from the OTHER buffer -- hence two; the C++ host loops,
  which wrap inside one base pointer, are called once per epoch, and the
  persistent launch, which wraps inside the kernel, is refused;
* ``optimizer="momentum" | "adam"`` (``--optimizer``): the trainer owns zero-initialised
  slot planes (``slots``: momentum ``[accum]``, adam ``[m, v]``; flat f32 [79510] in the
  parameter layout) and ``parallel/gpu_ps_optim.py``'s formulas are applied INSIDE the
  two-launch step: ``mlp_lean_fwdapply_opt`` forms each W1 tile's gradient in registers as the
  SGD step does, and the lane that owns an element reads and rewrites its slot values next to
  the parameter (slots in place, parameters ping-pong; no gradient buffer, no third launch).
  "Nothing to apply" is an explicit bit (a copy that leaves the slots alone), and Adam's ``t``
  is ``global_step + 1`` of the step being applied, read from a two-word step pair indexed by
  the buffer parity (``ops.mlp_step.PipelinedOpt``) -- never from the counter the same launch
  advances.  ``seek`` sets it, so a restored ``global_step`` restores ``t``.  Graph replay,
  ``run_launched`` (``MlpRunOptPlan``), ``flush``, ``snapshot``, ``evaluate`` and the stats
  work as with sgd; the persistent launch, the three-launch direct step, ``DTFX_MLP_KS=14``,
  the fused flush and the exchange engines are sgd-only and refuse an optimizer.  Data
  parallel: the all-reduce engine applies the reduced gradient with ``ops.optim``'s
  ``scale_`` + ``momentum_`` / ``adam_`` in place (``t`` from the device counter) before the
  next step's launches.
* ``lr_schedule`` (an ``ops.lr_schedule.LRSchedule``; ``--lr_schedule``): the rate of every
  step is computed ON THE DEVICE from the step word the optimizer variants already read, by
  scheduled instantiations of the first launch (``mlp_lean_fwdapply_sched``; scheduled sgd is
  one of them, with the step pair and no slot plane).  ``learning_rate`` is the base rate;
  nothing is baked into a captured graph or a C++ host loop, and ``seek`` puts a resumed run
  back on the curve.  The stats lane publishes each step's rate to an f32 ring parallel to the
  stats ring (``learning_rate()`` / ``learning_rates()``).  ``None`` or the constant kind
  without warm-up is today's trainer and launches exactly today's kernels.  The all-reduce
  engine computes the pending step's rate with a one-wave kernel into a device float that
  ``ops.optim`` reads (``lr_tensor``), sgd included (in place, not the deferred apply).  The
  exchange engines, the persistent launch, the three-launch direct step, ``DTFX_MLP_KS=14``
  and the fused flush refuse a schedule.
* ``dropout`` (``--dropout``; ``ops/dropout.py`` has the definition): inverted dropout on the
  hidden activation, inside the head launch alone -- the logits and ``hbuf`` take the dropped,
  rescaled h, dz1 the mask factor -- so every first launch (sgd, momentum, adam, scheduled,
  shuffled) is the one it was.  The mask is Philox4x32-10 of (``dropout_seed``, global_step,
  ``rank``, row, unit); the head reads the step from the device counter, so nothing is baked
  into a graph or a host loop, a checkpoint carries nothing new and ``seek`` resumes the mask
  sequence.  Recorded stats are training-mode values; ``evaluate`` / ``snapshot`` never drop.
  Works in the two-launch step, the three-launch direct step and the all-reduce engine; the
  exchange engines, the persistent launch, ``DTFX_MLP_KS=14`` and the fused flush refuse it.
  ``dropout=0`` launches exactly today's kernels.
* ``weight_decay`` / ``adamw`` / ``nesterov`` (``--weight_decay``, ``--adamw``, ``--nesterov``;
  ``ops/weight_decay.py`` has the definition, which is ``ops/optim.py``'s and ``torch.optim``'s):
  L2 decay for sgd, momentum and ``adamw=False`` adam, decoupled decay for AdamW, and Nesterov
  momentum, inside the lane expression that owns each element -- the W1 item of the first launch
  and the small-parameter lanes (``mlp_lean_fwdapply_wd``: one instantiation per optimizer, at a
  constant and at a scheduled rate).  The parameter is already in the lane's registers, so no
  load and no launch is added; ``apply == 0`` stays a pure copy; the decoupled term uses the
  rate of the step applied.  Decay is uniform over the flat buffer, biases included; the
  recorded loss stays the cross-entropy.  Works with every optimizer, schedule, shuffle and
  dropout through ``step()``, graph replay, ``run_launched``, ``flush``, ``snapshot``, ``seek``
  and the all-reduce engine (``ops.optim``'s own arguments; sgd then applies in place).  The
  exchange engines, the three-launch direct step, the persistent launch, ``DTFX_MLP_KS=14`` and
  the fused flush refuse them.  ``weight_decay=0, nesterov=False`` launches exactly today's
  kernels.
* ``activation`` (``--activation``; ``ops/hidden_act.py`` has the definition): the hidden
  activation, ``sigmoid`` (the reference's, the default), ``relu`` or ``tanh``.  The activation
  and its derivative live in the head launch alone, and every derivative is formed from the h
  the lane already holds (``h (1 - h)``, ``[h > 0]``, ``1 - h^2``): no load, no launch and no
  workspace word is added, and every first launch, the flush and the weight-gradient launch
  are the ones they were (they read the factors).  relu / tanh instantiations exist for the
  lean head and the three-launch head, plain and with dropout (the derivative then uses the
  undropped h).  Works with every optimizer, schedule, decay, shuffle and dropout through
  ``step()``, graph replay, ``run_launched``, ``flush``, ``snapshot``, ``seek`` and the
  all-reduce engine; ``evaluate`` evaluates with the trainer's activation.  Initialisation is
  the caller's (the reference's) and a checkpoint does not record the activation.  The
  exchange engines, the persistent launch, ``DTFX_MLP_KS=14`` and the fused flush have sigmoid
  heads only and refuse another activation.  ``activation="sigmoid"`` launches exactly today's
  kernels.
* ``ema_decay`` / ``ema_num_updates`` (``--ema_decay``, ``--ema_num_updates``; ``ops/ema.py`` has
  the definition, which is ``tf.train.ExponentialMovingAverage``'s): a shadow plane (``ema``: flat
  f32 [79510] in the parameter layout, initialised from ``params`` at construction) follows the
  parameters, ``shadow -= (1 - d_t) * (shadow - p_new)`` after every update, inside the first
  launch: the lane that stores a new parameter value also reads and rewrites its shadow value,
  exactly as it does its slot values (``mlp_lean_fwdapply_ema``: one instantiation per optimizer,
  at a constant and at a scheduled rate, with or without decay; plain sgd takes it too, with the
  step pair).  No launch and no gradient buffer is added; ``apply == 0`` touches no shadow byte;
  the shadow never feeds back into training (parameters and slots are bit-identical to
  ``ema_decay=0``).  With ``ema_num_updates`` ``d_t = min(decay, (1 + t) / (10 + t))`` comes from
  the step word, once per wave, so ``seek`` restores it and leaves the shadow alone.
  ``load_params`` does NOT reset the shadow (``load_ema`` sets it; a restore without averaged
  variables calls ``load_ema(params)``).  ``snapshot(with_ema=True)`` and ``evaluate(ema=True)``
  return / evaluate the shadow after every step run so far.  Works with every optimizer,
  schedule, decay, shuffle, dropout and activation through ``step()``, graph replay,
  ``run_launched``, ``flush``, ``seek`` and the all-reduce engine (``ops.optim.ema_`` after the
  optimizer; sgd then applies in place).  The exchange engines, the three-launch direct step, the
  persistent launch, ``DTFX_MLP_KS=14`` and the fused flush refuse it.  ``ema_decay=0`` launches
  exactly today's kernels.

Data-parallel update order: the all-reduced gradient of step t is applied at
the start of step t+1 (ping-pong parameter buffers make the apply race-free
across the launch's workgroups).  ``flush()`` applies the pending gradient,
so ``params`` after ``flush()`` is exactly the result of t full SGD steps.
"""
from __future__ import annotations

import os
import time

import torch

from ..ops import dropout as dropout_mod
from ..ops import ema as ema_mod
from ..ops import hidden_act
from ..ops import lr_schedule as lr_schedule_mod
from ..ops import mlp_step, optim
from ..ops import weight_decay as weight_decay_mod
from ..ops._ext import stream_handle
from ..parallel import gpu_ps_optim


class FusedMLPTrainer:
    def __init__(self, params, x, labels, batch_size=100, learning_rate=0.001, allreduce=None,
                 world_size=1, stats_ring=4096, global_step=0, max_graph_steps=1024,
                 fused_comm=None, factor_comm=None, x_all=None, rank=0, pipeline=True,
                 shuffle=False, shuffle_seed=0, optimizer="sgd", momentum=0.9, beta1=0.9,
                 beta2=0.999, epsilon=1e-8, lr_schedule=None, dropout=0.0, dropout_seed=0,
                 weight_decay=0.0, adamw=True, nesterov=False, activation="sigmoid",
                 ema_decay=0.0, ema_num_updates=False):
        # --ema_decay: refused first where no launch carries a shadow plane
        self.avg = ema_mod.resolve(ema_decay, ema_num_updates)
        if self.avg is not None:
            if fused_comm is not None or factor_comm is not None:
                raise ValueError("ema_decay: the exchange engines (fused_comm / factor_comm) keep "
                                 "no moving average of the parameters; use the all-reduce engine")
            if not pipeline and allreduce is None and int(world_size) == 1:
                raise ValueError("ema_decay: the three-launch direct step (pipeline=False) has "
                                 "no moving-average variant; use the two-launch step "
                                 "(pipeline=True)")
            if params.is_cuda and allreduce is None and int(world_size) == 1:
                from ..ops._ext import hip

                if hip().mlp_single_ks() != 28:
                    raise ValueError("ema_decay: DTFX_MLP_KS=14 has no moving-average variant; "
                                     "use the default K slicing")
        # --activation: refused first where only the sigmoid head exists
        self.activation = hidden_act.check(activation)
        if self.activation != "sigmoid":
            if fused_comm is not None or factor_comm is not None:
                raise ValueError("activation %s: the exchange engines (fused_comm / factor_comm) "
                                 "have sigmoid heads only; use the all-reduce engine"
                                 % self.activation)
            if params.is_cuda and pipeline and allreduce is None and int(world_size) == 1:
                from ..ops._ext import hip

                if hip().mlp_single_ks() != 28:
                    raise ValueError("activation %s: DTFX_MLP_KS=14 has no relu / tanh variant; "
                                     "use the default K slicing" % self.activation)
        # --weight_decay / --nesterov: refused first where the update has no such term
        self.decay = weight_decay_mod.resolve(gpu_ps_optim.check_kind(optimizer), weight_decay,
                                              adamw, nesterov, momentum)
        if self.decay is not None:
            if fused_comm is not None or factor_comm is not None:
                raise ValueError("weight_decay / nesterov: the exchange engines (fused_comm / "
                                 "factor_comm) apply plain gradient descent; use the all-reduce "
                                 "engine")
            if not pipeline and allreduce is None and int(world_size) == 1:
                raise ValueError("weight_decay / nesterov: the three-launch direct step "
                                 "(pipeline=False) has no weight-decay variant; use the "
                                 "two-launch step (pipeline=True)")
            if params.is_cuda and allreduce is None and int(world_size) == 1:
                from ..ops._ext import hip

                if hip().mlp_single_ks() != 28:
                    raise ValueError("weight_decay / nesterov: DTFX_MLP_KS=14 has no "
                                     "weight-decay variant; use the default K slicing")
        # --dropout: refused first where no head with the mask exists
        self.drop = dropout_mod.resolve(dropout, dropout_seed, int(rank))
        if self.drop is not None:
            if fused_comm is not None or factor_comm is not None:
                raise ValueError("dropout: the exchange engines (fused_comm / factor_comm) have "
                                 "no dropout variant; use the all-reduce engine")
            if params.is_cuda and pipeline and allreduce is None and int(world_size) == 1:
                from ..ops._ext import hip

                if hip().mlp_single_ks() != 28:
                    raise ValueError("dropout: DTFX_MLP_KS=14 has no dropout variant")
        # --lr_schedule: refused first where the rate is a by-value argument of every launch
        self.sched = lr_schedule_mod.resolve(lr_schedule)
        if self.sched is not None:
            if fused_comm is not None or factor_comm is not None:
                raise ValueError("lr_schedule: the exchange engines (fused_comm / factor_comm) "
                                 "train at a constant rate; use the all-reduce engine")
            if not pipeline and allreduce is None and int(world_size) == 1:
                raise ValueError("lr_schedule: the three-launch direct step (pipeline=False) "
                                 "trains at a constant rate")
            if params.is_cuda and allreduce is None and int(world_size) == 1:
                from ..ops._ext import hip

                if hip().mlp_single_ks() != 28:
                    raise ValueError("lr_schedule: DTFX_MLP_KS=14 has no learning-rate schedule "
                                     "variant")
        # --optimizer momentum | adam: refused first where only gradient descent exists
        self.optimizer = gpu_ps_optim.check_kind(optimizer)
        if self.optimizer != "sgd":
            if fused_comm is not None or factor_comm is not None:
                raise ValueError("optimizer %s: the exchange engines (fused_comm / factor_comm) "
                                 "apply gradient descent only; use the all-reduce engine"
                                 % self.optimizer)
            if not pipeline and allreduce is None and int(world_size) == 1:
                raise ValueError("optimizer %s: the three-launch direct step (pipeline=False) "
                                 "applies gradient descent only" % self.optimizer)
        if not params.is_cuda:
            raise ValueError("FusedMLPTrainer runs on the GPU; use the generic path on CPU")
        if params.numel() != mlp_step.NPARAM:
            raise ValueError("params must be the flat 79,510-element MLP buffer")
        self.device = params.device
        self.B = int(batch_size)
        self.lr = float(learning_rate)
        self.world_size = int(world_size)
        self.allreduce = allreduce
        self.fused_comm = fused_comm
        if fused_comm is not None and (allreduce is not None or world_size < 2):
            raise ValueError("fused_comm replaces allreduce and needs world_size >= 2")
        self.factor_comm = factor_comm
        self.xstride = 0
        if factor_comm is not None:
            if fused_comm is not None or allreduce is not None or world_size < 2:
                raise ValueError("factor_comm replaces allreduce/fused_comm and needs world >= 2")
            if (x_all is None or x_all.dim() != 3 or x_all.shape[0] != world_size
                    or not x_all.is_contiguous() or x_all.dtype != torch.float32
                    or x_all.device != self.device):
                raise ValueError("factor_comm needs x_all: contiguous f32 [world, n, 784] on the GPU")
            x = x_all[int(rank)]  # a view: the other ranks' batches sit at +/- xstride
            self.xstride = x_all.stride(0)
            self.dz1A = torch.zeros(world_size * mlp_step.factor_plane(int(batch_size)),
                                    device=self.device, dtype=torch.float32)
        x = x.reshape(-1, mlp_step.D).to(self.device, torch.float32).contiguous()
        if factor_comm is not None and x.data_ptr() != x_all[int(rank)].data_ptr():
            raise ValueError("x_all slice must stay a view")
        labels = labels.reshape(-1).to(self.device, torch.int32).contiguous()
        self.nbatches = x.shape[0] // self.B
        if self.nbatches < 1:
            raise ValueError("dataset smaller than one batch")
        self.x, self.labels = x, labels
        self.shuffle = bool(shuffle)
        self.shuffle_seed = int(shuffle_seed)
        self.epoch = 0  # epoch of the next step (advanced in shuffle mode only)
        self.bufs = [params.detach().clone().contiguous(), torch.empty_like(params)]
        self.cur = 0
        self.grad = torch.zeros_like(params)
        self.ws = mlp_step.StepWorkspace(self.B, self.device, stats_ring)
        self.ws.set_global_step(global_step)
        self.pos = int(global_step) % self.nbatches  # next batch (host mirror)
        self.pending = False
        # single GPU without a communicator, the fused engine or the factor engine (batch
        # <= 128): the two-launch pipelined step
        self.pipelined = bool(pipeline and allreduce is None and (
            (self.world_size == 1 and factor_comm is None and fused_comm is None)
            or fused_comm is not None
            or (factor_comm is not None and self.B <= 128)))
        # --optimizer momentum | adam (module docstring): slot planes owned by the trainer
        # lr_schedule: the same object also carries the schedule block and the rate ring, and
        # exists for scheduled sgd too (no slot plane) -- the scheduled step is an OptArgs one
        self.opt = None
        # ema_decay: it owns the shadow plane too, plain sgd included
        if (self.optimizer != "sgd" or self.sched is not None or self.decay is not None
                or self.avg is not None):
            self.opt = mlp_step.PipelinedOpt(self.optimizer, self.device, momentum, beta1, beta2,
                                             epsilon, schedule=self.sched, stats_ring=stats_ring,
                                             decay=self.decay, ema=self.avg)
            self.opt.set_step(global_step)
            if self.avg is not None:
                self.opt.shadow.copy_(self.bufs[0])  # shadow_0: the initial parameters, as in TF
        # the all-reduce engine's scheduled rate (ops.optim's lr_tensor)
        self._lr_dev = (torch.zeros(1, device=self.device, dtype=torch.float32)
                        if self.sched is not None else None)
        self.max_graph_steps = int(max_graph_steps)
        self._graphs = {}
        self._pool = None
        self._ll = None   # granule buffer of the persistent engine (allocated on first use)
        self._ebase = 0   # epoch base of its next launch
        self._unchecked = False  # a persistent launch whose hand-offs were not verified yet
        self._host_args = None   # run_launched's cached launcher and buffer addresses
        if self.shuffle:
            # the pristine dataset (x0 / labels0, with factor_comm the whole x_all) plus TWO
            # shuffled buffers: epoch e reads buffer e & 1, and the update pending across the
            # boundary still reads epoch e - 1's last batch from the other one.  ``x`` /
            # ``labels`` / ``_host_args`` always name the CURRENT epoch's buffer (``_bind``).
            self.x0, self.labels0 = x, labels
            src = x_all if factor_comm is not None else x
            self._src = src
            self._dst = [torch.empty_like(src), torch.empty_like(src)]
            self.xs = [d[int(rank)] if factor_comm is not None else d for d in self._dst]
            self.ys = [torch.empty_like(labels), torch.empty_like(labels)]
            self._hargs = [None, None]
            self.run_launched = self._run_launched_epochs
            self._bind(int(global_step) // self.nbatches)
            self._gather()

    # -- state --------------------------------------------------------------
    @property
    def direct(self):
        """SGD apply fused into the backward kernel (one GPU, or the fused xGMI exchange)."""
        return not self.pipelined and (
            self.fused_comm is not None or self.factor_comm is not None
            or (self.allreduce is None and self.world_size == 1))

    def _verified(self):
        """Raise before parameters or stats of a persistent launch whose in-kernel hand-off
        timed out are used (that launch writes zeros instead of valid parameters)."""
        if self._unchecked:
            self._unchecked = False
            self.check()

    @property
    def params(self):
        """Current parameters (excludes a pending, not yet applied gradient)."""
        self._verified()
        return self.bufs[self.cur]

    @property
    def slots(self):
        """The optimizer's slot planes (momentum: [accum]; adam: [m, v]; sgd: []), flat f32
        [79510] in the parameter layout -- like ``params``, without a pending update."""
        self._verified()
        return [] if self.opt is None else self.opt.slots

    def load_slots(self, slots):
        """Set the slot planes (a restored checkpoint's); as ``load_params``, nothing is
        pending afterwards."""
        own = self.slots
        slots = list(slots)
        if len(slots) != len(own):
            raise ValueError("optimizer %s has %d slot planes, got %d"
                             % (self.optimizer, len(own), len(slots)))
        for d, t in zip(own, slots):
            d.copy_(t.reshape(-1))
        self.pending = False

    @property
    def ema(self):
        """The moving average of the parameters (the shadow plane: flat f32 [79510] in the
        parameter layout) -- like ``params`` and ``slots``, without a pending update."""
        self._verified()
        if self.avg is None:
            raise RuntimeError("ema: the trainer keeps no moving average (ema_decay is 0)")
        return self.opt.shadow

    def load_ema(self, plane):
        """Set the shadow plane (a restored checkpoint's averaged variables, or the restored
        parameters when it has none); as ``load_slots``, nothing is pending afterwards."""
        self.ema.copy_(plane.reshape(-1))
        self.pending = False

    @property
    def _inplace(self):
        """All-reduce engine with an optimizer: the reduced gradient is applied in place on the
        current buffer (``ops.optim``), so the parity never moves."""
        return self.opt is not None and not self.pipelined

    def _apply_reduced(self, p, slots, publish=True, shadow=None):
        """The pending all-reduced gradient through the optimizer, in place on ``p`` /
        ``slots`` (graph-capturable: Adam's t is the device counter, which the step that
        produced the gradient already advanced to its ``global_step + 1``).  With a schedule
        the pending step's rate -- step ``counter - 1`` -- is computed on the device first and
        read by the optimizer kernel (``publish``: also written to the rate ring).  With a
        moving average ``shadow`` (default: the trainer's own) then follows the new ``p``
        (``ops.optim.ema_``; its t is the same counter)."""
        optim.scale_(self.grad, 1.0 / self.world_size)
        h = self.opt.hyper
        lrt = None
        if self.sched is not None:
            lrt = mlp_step.scheduled_rate(self.ws, self.opt, self.lr, self._lr_dev, publish)
        d = self.decay  # (weight decay / Nesterov: the arguments ops.optim already takes)
        if self.optimizer == "sgd":
            optim.sgd_(p, self.grad, self.lr, lr_tensor=lrt, **(d.sgd_kw if d else {}))
        elif self.optimizer == "momentum":
            optim.momentum_(p, self.grad, slots[0], self.lr, momentum=h[0], lr_tensor=lrt,
                            **(d.momentum_kw if d else {}))
        else:
            kw = d.adam_kw if d else dict(weight_decay=0.0, adamw=False)
            optim.adam_(p, self.grad, slots[0], slots[1], self.lr, 0, beta1=h[0], beta2=h[1],
                        eps=h[2], step_tensor=self.ws.ctr, lr_tensor=lrt, **kw)
        if self.avg is not None:
            optim.ema_(self.opt.shadow if shadow is None else shadow, p, self.avg,
                       step_tensor=self.ws.ctr)

    def flush(self):
        """Apply the pending update in place (DP: p -= lr/N * grad; pipelined: the last
        step's factors)."""
        self._verified()
        if self.pending:
            if self.pipelined and self.factor_comm is not None:
                xp = self._xprev(self.pos)
                mlp_step.flush_factor(self.bufs[self.cur], xp, self.ws, self.lr / self.world_size,
                                      self.factor_comm, self.dz1A, self.xstride)
            elif self.pipelined and self.fused_comm is not None:
                xp = self._xprev(self.pos)
                mlp_step.flush_xgmi(self.bufs[self.cur], self.bufs[self.cur ^ 1], xp, self.ws,
                                    self.lr / self.world_size, self.fused_comm)
                self.cur ^= 1
            elif self.pipelined and self.opt is not None:
                xp = self._xprev(self.pos)
                mlp_step.flush_pipelined_opt(self.bufs[self.cur], self.bufs[self.cur ^ 1], xp,
                                             self.ws, self.lr, self.cur, self.opt)
                self.cur ^= 1
            elif self.pipelined:
                xp = self._xprev(self.pos)
                mlp_step.flush_pipelined(self.bufs[self.cur], self.bufs[self.cur ^ 1], xp, self.ws,
                                         self.lr)
                self.cur ^= 1
            elif self.opt is not None:
                self._apply_reduced(self.bufs[self.cur], self.opt.slots)
            else:
                optim.sgd_(self.bufs[self.cur], self.grad, self.lr / self.world_size)
            self.pending = False
        return self.bufs[self.cur]

    def snapshot(self, with_slots=False, with_ema=False):
        """``with_slots``: ``(parameters, [slot planes])`` instead, the slots by the same rules
        (new tensors; an optimizer's pending all-reduced gradient is applied to copies of the
        parameters AND the slots, so the trainer's state does not move).  ``with_ema``: the
        shadow plane after every step run so far is appended, by the same rules -- ``(parameters,
        shadow)``, or ``(parameters, [slot planes], shadow)`` with both.

        Parameters after every step run so far (a pending update included) as a NEW
        tensor, WITHOUT changing the trainer: no peer exchange starts and the replicas' update
        sequence is untouched, so one rank alone may call it (chief-only checkpoints and
        evals).  The all-reduce engine's pending gradient is already reduced: applied to a
        copy.  A pending update of the pipelined exchange engines needs every rank's
        exchange: raises (call flush() on every rank instead)."""
        self._verified()
        if with_ema and self.avg is None:
            raise RuntimeError("snapshot(with_ema=True): the trainer keeps no moving average "
                               "(ema_decay is 0)")
        if with_slots or with_ema:
            if self.pending and self._inplace:
                out, sl = self.bufs[self.cur].clone(), [t.clone() for t in self.opt.slots]
                sh = self.opt.shadow.clone() if self.avg is not None else None
                g = self.grad.clone()  # (_apply_reduced scales the gradient in place)
                # (the rate ring and the trainer's shadow do not move)
                self._apply_reduced(out, sl, publish=False, shadow=sh)
                self.grad.copy_(g)
            else:
                out = self.snapshot()  # (pipelined on one GPU: flushed; slots then current)
                sl = [t.clone() for t in self.slots]
                sh = self.opt.shadow.clone() if with_ema else None
            return (out,) + ((sl,) if with_slots else ()) + ((sh,) if with_ema else ())
        p = self.bufs[self.cur]
        if not self.pending:
            return p.clone()
        if self._inplace:
            return self.snapshot(with_slots=True)[0]
        if not self.pipelined:
            out = p.clone()
            optim.sgd_(out, self.grad, self.lr / self.world_size)
            return out
        if self.world_size == 1:
            return self.flush().clone()
        raise RuntimeError("snapshot(): the pending update is a peer exchange; flush() on "
                           "every rank first")

    def evaluate(self, x, labels=None, ema=False, **kw):
        """``ops.mlp_eval.evaluate`` of the parameters after every step run so far on ``x``
        [n, 784] / ``labels`` (int32 [n]): one fused launch, no host synchronisation; the
        keyword arguments (``predictions``, ``probs``, ``acc``) are the op's.  The parameters
        are ``snapshot()``'s, by its rules: a pending pipelined update on one GPU is flushed,
        the all-reduce engine's pending gradient is applied to a copy, a pending peer exchange
        raises.  ``global_step()`` is unchanged.  The hidden activation is the trainer's.
        ``ema=True``: the moving average of the parameters (``snapshot(with_ema=True)``'s
        shadow) is evaluated instead."""
        from ..ops import mlp_eval

        kw.setdefault("activation", self.activation)
        p = self.snapshot(with_ema=True)[1] if ema else self.snapshot()
        return mlp_eval.evaluate(p, x, labels, **kw)

    def load_params(self, p):
        """Set the parameters; nothing is pending afterwards.  The moving average is NOT reset:
        a restore sets it with ``load_ema`` (the checkpoint's averaged variables, or these
        parameters when it has none)."""
        self.bufs[self.cur].copy_(p)
        self.pending = False

    def global_step(self) -> int:
        # the pipelined step records step t (stats, global_step += 1) inside step t+1's
        # first launch (or flush())
        return self.ws.global_step() + (1 if (self.pipelined and self.pending) else 0)

    def batch(self, i):
        sl = slice(i * self.B, (i + 1) * self.B)
        return self.x[sl], self.labels[sl]

    def _xprev(self, pos):
        """The batch before position ``pos`` of the stream: the pending update's input.  In
        shuffle mode the batch before position 0 is the LAST batch of the previous epoch, which
        lives in the other shuffled buffer."""
        i = (pos - 1) % self.nbatches
        x = self.xs[(self.epoch - 1) & 1] if (self.shuffle and pos == 0) else self.x
        return x[i * self.B:(i + 1) * self.B]

    # -- per-epoch reshuffle (shuffle=True) ------------------------------------
    def _bind(self, epoch):
        """Point ``x`` / ``labels`` / the host loop's cached addresses at ``epoch``'s buffer
        (host mirrors only: nothing is launched)."""
        self._hargs[self.epoch & 1] = self._host_args
        self.epoch = int(epoch)
        k = self.epoch & 1
        self.x, self.labels, self._host_args = self.xs[k], self.ys[k], self._hargs[k]

    def _gather(self):
        """Write the current epoch's order into its buffer: position j <- original row
        ``shuffle_index(shuffle_seed, epoch, n)[j]`` (every plane of x_all with factor_comm),
        in order on the compute stream."""
        from ..ops.shuffle import shuffle_rows_

        k = self.epoch & 1
        shuffle_rows_(self._dst[k], self.ys[k], self._src, self.labels0, self.shuffle_seed,
                      self.epoch)

    def _wrapped(self):
        """After the step(s) that moved ``pos``: at an epoch boundary in shuffle mode, move to
        the next epoch's buffer and fill it.  The buffer it overwrites held epoch e - 1, whose
        last reader (the first step of epoch e) was launched before."""
        if self.shuffle and self.pos == 0:
            self._bind(self.epoch + 1)
            self._gather()

    def seek(self, global_step):
        """Position the trainer at ``global_step``: the device counter, the batch position and
        (shuffle mode) the epoch, whose buffer is regenerated -- a resumed run continues in the
        order an uninterrupted one has.  A pending update is applied first; nothing is pending
        afterwards."""
        self.flush()
        s = int(global_step)
        self.ws.set_global_step(s)
        if self.opt is not None:
            self.opt.set_step(s)  # Adam's t of the next applied step: s + 1
        self.pos = s % self.nbatches
        if self.shuffle:
            self._bind(s // self.nbatches)
            self._gather()

    # -- one step (eager) -----------------------------------------------------
    def _step_launches(self):
        xb, yb = self.batch(self.pos)
        p0 = self.pos
        self.pos = (self.pos + 1) % self.nbatches
        if self.factor_comm is not None and self.pipelined:
            xp = self._xprev(p0)
            mlp_step.step_factor_pipelined(self.bufs[self.cur], self.bufs[self.cur ^ 1], xp, xb,
                                           yb, self.ws, self.lr / self.world_size, self.pending,
                                           self.factor_comm, self.dz1A, self.xstride)
            self.cur ^= 1
            self.pending = True
            return
        if self.factor_comm is not None:
            mlp_step.step_factor(self.bufs[self.cur], xb, yb, self.ws, self.lr / self.world_size,
                                 self.factor_comm, self.dz1A, self.xstride)
            return
        if self.fused_comm is not None and self.pipelined:
            xp = self._xprev(p0)
            mlp_step.step_xgmi_pipelined(self.bufs[self.cur], self.bufs[self.cur ^ 1], xp, xb,
                                         yb, self.ws, self.lr / self.world_size, self.pending,
                                         self.fused_comm)
            self.cur ^= 1
            self.pending = True
            return
        if self.fused_comm is not None:
            mlp_step.step_xgmi(self.bufs[self.cur], xb, yb, self.ws, self.lr / self.world_size,
                               self.fused_comm)
            return
        if self.direct:
            mlp_step.step_direct(self.bufs[self.cur], xb, yb, self.ws, self.lr, dropout=self.drop,
                                 activation=self.activation)
            return
        if self.pipelined and self.opt is not None:
            xp = self._xprev(p0)
            mlp_step.step_pipelined_opt(self.bufs[self.cur], self.bufs[self.cur ^ 1], xp, xb, yb,
                                        self.ws, self.lr, self.pending, self.cur, self.opt,
                                        dropout=self.drop, activation=self.activation)
            self.cur ^= 1
            self.pending = True
            return
        if self.pipelined:
            xp = self._xprev(p0)
            mlp_step.step_pipelined(self.bufs[self.cur], self.bufs[self.cur ^ 1], xp, xb, yb,
                                    self.ws, self.lr, apply=self.pending, dropout=self.drop,
                                    activation=self.activation)
            self.cur ^= 1
            self.pending = True
            return
        cur = self.bufs[self.cur]
        if self.opt is not None:
            # all-reduce engine with an optimizer: the reduced gradient of the previous step
            # through ops.optim in place, then the step without its deferred apply
            if self.pending:
                self._apply_reduced(cur, self.opt.slots)
            mlp_step.step_grad(cur, xb, yb, self.ws, self.grad, dropout=self.drop,
                               activation=self.activation)
        elif self.pending:
            mlp_step.step_grad(cur, xb, yb, self.ws, self.grad, prev_grad=self.grad,
                               lr=self.lr / self.world_size, p_new=self.bufs[self.cur ^ 1],
                               dropout=self.drop, activation=self.activation)
            self.cur ^= 1
        else:
            mlp_step.step_grad(cur, xb, yb, self.ws, self.grad, dropout=self.drop,
                               activation=self.activation)
        if self.allreduce is not None:
            self.allreduce(self.grad)
        self.pending = True

    def step(self):
        self._step_launches()
        self._wrapped()

    # -- hipGraph capture/replay ---------------------------------------------
    def _graph(self, n):
        """Graph of ``n`` steps starting at batch ``self.pos`` and parity ``self.cur``.

        Capture records without executing, so only the host mirrors (batch
        position, ping-pong parity, pending flag) move during capture; they are
        restored afterwards and advanced by the caller at replay.
        """
        key = (n, self.pos, self.cur, self.epoch & 1)  # (the x pointers: the shuffle buffer)
        g = self._graphs.get(key)
        if g is None:
            pos, cur, pend = self.pos, self.cur, self.pending
            assert self.direct or pend
            s = torch.cuda.Stream(self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, pool=self._pool, stream=s):
                    for _ in range(n):
                        self._step_launches()
            torch.cuda.current_stream(self.device).wait_stream(s)
            self._pool = g.pool()
            self.pos, self.cur, self.pending = pos, cur, pend
            self._graphs[key] = g
        return g

    def _plan(self, steps):
        """Split ``steps`` into epoch-aligned graph chunks -> list of n."""
        out, pos = [], self.pos
        while steps > 0:
            n = min(steps, self.nbatches - pos, self.max_graph_steps)
            out.append(n)
            pos = (pos + n) % self.nbatches
            steps -= n
        return out

    @property
    def host_loop_ok(self):
        """The step can be issued by a C++ host loop: the plain single-GPU pipelined step
        (``mlp_run_pipelined``) or a pipelined exchange engine -- fused2 / fused2x / factor2
        (``XgmiComm`` ``mlp_run_engine``)."""
        if not self.pipelined or self.allreduce is not None:
            return False
        if self.world_size == 1:
            return self.fused_comm is None and self.factor_comm is None
        c = self.fused_comm if self.fused_comm is not None else self.factor_comm
        return c is not None and hasattr(getattr(c, "_h", None), "mlp_run_engine")

    def run_launched(self, steps, flush=False):
        """``steps`` pipelined single-GPU steps issued by ONE C++ call (kernel launches, no
        graph): no ~15 us graph-submission latency before the first kernel.  ``flush``: the
        last step's update is applied by the same call (one more launch, as ``flush()``).
        The buffer addresses are read once: a short timed region (bench.py --steps 20) pays
        the Python side of this call before its first kernel starts."""
        steps = int(steps)
        if not self.host_loop_ok:
            raise RuntimeError("run_launched: pipelined single-GPU step or exchange engine only")
        if steps <= 0:
            if flush:
                self.flush()
            return
        if self.world_size > 1:
            return self._run_launched_engine(steps, flush)
        if self.drop is not None and flush and _flush_fused():
            raise ValueError("dropout: the fused flush (DTFX_MLP_FLUSH_FUSED) has no dropout "
                             "variant")
        if self.activation != "sigmoid" and flush and _flush_fused():
            raise ValueError("activation %s: the fused flush (DTFX_MLP_FLUSH_FUSED) has a sigmoid "
                             "head only; flush in its own launch" % self.activation)
        if self.decay is not None and flush and _flush_fused():
            raise ValueError("weight_decay / nesterov: the fused flush (DTFX_MLP_FLUSH_FUSED) has "
                             "no weight-decay variant; flush in its own launch")
        if self.avg is not None and flush and _flush_fused():
            raise ValueError("ema_decay: the fused flush (DTFX_MLP_FLUSH_FUSED) has no "
                             "moving-average variant; flush in its own launch")
        a = self._host_args
        if a is None:
            from ..ops._ext import hip, ptr

            ws = self.ws
            if self.opt is not None:  # the optimizer form of the plan (slot pointers bound too)
                oargs = (self.opt.ema_args() if self.avg is not None
                         else self.opt.wd_args() if self.decay is not None
                         else self.opt.args() if self.sched is None else self.opt.sched_args())
                plan = hip().MlpRunOptPlan(ptr(self.bufs[0]), ptr(self.bufs[1]), ptr(self.x),
                                           ptr(self.labels), self.nbatches, ptr(ws.buf),
                                           ptr(ws.ctr), ptr(ws.stats), ws.stats_ring, self.B,
                                           *oargs)
                if self.drop is not None:
                    plan.set_drop(*self.drop.args())
                if self.activation != "sigmoid":
                    plan.set_act(hidden_act.act_id(self.activation))
                a = self._host_args = (plan.run, self.device.index, None)
            elif (self.drop is not None or self.activation != "sigmoid"
                  or os.environ.get("DTFX_MLP_PLAN", "1") != "0"):
                # the buffers bound once in a C++ plan: the call before the first kernel
                # converts 7 arguments instead of 17 (a short timed region starts on the host)
                plan = hip().MlpRunPlan(ptr(self.bufs[0]), ptr(self.bufs[1]), ptr(self.x),
                                        ptr(self.labels), self.nbatches, ptr(ws.buf),
                                        ptr(ws.ctr), ptr(ws.stats), ws.stats_ring, self.B)
                if self.drop is not None:
                    plan.set_drop(*self.drop.args())
                if self.activation != "sigmoid":
                    plan.set_act(hidden_act.act_id(self.activation))
                a = self._host_args = (plan.run, self.device.index, None)
            else:  # (A/B: the 17-argument entry point)
                a = self._host_args = (hip().mlp_run_pipelined, self.device.index,
                                       (ptr(self.bufs[0]), ptr(self.bufs[1]), ptr(self.x),
                                        ptr(self.labels), ptr(ws.buf), ptr(ws.ctr),
                                        ptr(ws.stats), ws.stats_ring))
        run, dix, full = a
        if full is None:
            run(self.cur, 1 if self.pending else 0, self.lr, self.pos, steps, 1 if flush else 0,
                stream_handle(dix))
        else:
            p0, p1, xp, lp, wb, wc, wst, ring = full
            run(p0, p1, self.cur, 1 if self.pending else 0, self.lr, xp, lp, self.nbatches,
                self.pos, steps, wb, wc, wst, ring, self.B, stream_handle(dix), 1 if flush else 0)
        self.pos = (self.pos + steps) % self.nbatches
        self.cur ^= (steps + (1 if flush else 0)) & 1
        self.pending = not flush

    def _run_launched_epochs(self, steps, flush=False):
        """``run_launched`` of a shuffle-mode trainer (bound over it in ``__init__``, so the
        shuffle-free call stays exactly as it is: a driver-sized timed region pays its Python
        side before the first kernel).  The C++ host loops take ONE base pointer and wrap
        inside it, so they are called once per epoch with that epoch's buffer; the step right
        after a boundary, whose pending update reads the previous epoch's last batch from the
        other buffer, is issued with explicit pointers.  A ``flush`` that ends an epoch runs
        inside the C++ call (its x_prev is that epoch's own last batch)."""
        steps = int(steps)
        if not self.host_loop_ok:
            raise RuntimeError("run_launched: pipelined single-GPU step or exchange engine only")
        while steps > 0:
            if self.pos == 0 and self.pending:
                self.step()
                steps -= 1
                continue
            n = min(steps, self.nbatches - self.pos)
            FusedMLPTrainer.run_launched(self, n, flush and n == steps)
            self._wrapped()
            steps -= n
        if flush:
            self.flush()

    def _run_launched_engine(self, steps, flush):
        """run_launched for the pipelined exchange engines: every rank issues the same steps
        from one C++ call (the in-kernel exchanges pair them up across ranks)."""
        from ..ops._ext import ptr

        factor = self.factor_comm is not None
        comm = self.factor_comm if factor else self.fused_comm
        kind = 2 if factor else (1 if getattr(comm, "two_shot", False) else 0)
        a = self._host_args
        if a is None:
            ws = self.ws
            a = self._host_args = (comm._h.mlp_run_engine, ptr(self.bufs[0]), ptr(self.bufs[1]),
                                   ptr(self.x), ptr(self.labels), ptr(ws.buf), ptr(ws.ctr),
                                   ptr(ws.stats), ws.stats_ring,
                                   ptr(self.dz1A) if factor else 0)
        fn, p0, p1, xp, lp, wb, wc, wst, ring, dz = a
        fn(kind, p0, p1, self.cur, 1 if self.pending else 0, self.lr / self.world_size, xp,
           int(self.xstride), lp, self.nbatches, self.pos, steps, wb, wc, wst, ring, self.B, dz,
           stream_handle(self.device.index), float(comm.timeout_s),
           1 if flush else 0)
        self.pos = (self.pos + steps) % self.nbatches
        self.cur ^= (steps + (1 if (flush and not factor) else 0)) & 1
        self.pending = not flush

    # -- persistent single-launch engine (csrc/kernels/mlp_persistent.hip) ----------------
    @property
    def persistent_ok(self):
        """The plain single-GPU step with batch <= 128 can run as ONE persistent launch (not in
        shuffle mode: that launch wraps around one dataset buffer inside the kernel)."""
        return (self.host_loop_ok and self.world_size == 1 and self.B <= 128
                and not self.shuffle and self.opt is None and self.drop is None
                and self.activation == "sigmoid")

    def run_persistent(self, steps, timeout_s=2.0, trace=None):
        """``steps`` complete SGD steps (every update applied, nothing left pending) in ONE
        launch: 105 co-resident workgroups hand z1 partials / backprop factors / small
        parameters to each other as epoch-tagged 8-byte granules instead of ending a kernel.
        Same trajectory as the pipelined two-launch step (to f32 rounding).  ``timeout_s`` bounds every in-kernel
        wait; a timed-out run raises at the next ``check()``.  ``trace``: optional int64
        [blocks, trace_steps, 12] buffer of in-kernel s_memrealtime stamps (probe only)."""
        from ..ops._ext import hip, ptr, stream_handle

        steps = int(steps)
        if self.sched is not None:
            raise ValueError("run_persistent: the persistent launch trains at a constant rate "
                             "(lr_schedule is not supported)")
        if self.drop is not None:
            raise ValueError("run_persistent: the persistent launch has no dropout variant")
        if self.activation != "sigmoid":
            raise ValueError("run_persistent: the persistent launch has a sigmoid head only "
                             "(activation %s is not supported)" % self.activation)
        if self.decay is not None:
            raise ValueError("run_persistent: the persistent launch has no weight-decay or "
                             "Nesterov variant; use run() / run_launched()")
        if self.avg is not None:
            raise ValueError("run_persistent: the persistent launch keeps no moving average of "
                             "the parameters (ema_decay is not supported); use run() / "
                             "run_launched()")
        if not self.persistent_ok:
            raise RuntimeError("run_persistent: single-GPU step with batch <= 128 only "
                               "(shuffle off, optimizer sgd)")
        if steps <= 0:
            return
        self.flush()  # a pending pipelined update is applied first (params exact)
        h = hip()
        if self._ll is None or self._ebase + steps + 2 >= 2 ** 32:
            self._ll = torch.zeros(int(h.mlp_persistent_ll_words()), dtype=torch.int64,
                                   device=self.device)
            self._ebase = 0
        ws = self.ws
        h.mlp_persistent(ptr(self.bufs[self.cur]), ptr(self.x), ptr(self.labels), self.nbatches,
                         self.pos, steps, self.lr, self._ebase, ptr(self._ll), ptr(ws.ctr),
                         ptr(ws.stats), ws.stats_ring, self.B, int(timeout_s * 1e8),
                         stream_handle(), 0 if trace is None else ptr(trace))
        self._ebase += steps + 1
        self.pos = (self.pos + steps) % self.nbatches
        self._unchecked = True

    def check(self):
        """Raise if an in-kernel wait of the persistent engine, or of the terminal head +
        apply launch of ``run_launched(.., flush=True)``, ever timed out."""
        if self._ll is not None and int(self._ll[-32].item()) != 0:
            raise RuntimeError("persistent MLP engine: an in-kernel hand-off timed out "
                               "(parameters are not valid)")
        ws = getattr(self, "ws", None)
        if ws is not None and ws.buf.is_cuda:
            sync = ws.buf[-4:].view(torch.int32)  # mlp::Bufs::sync (the workspace's last words)
            if int(sync[2].item()) != 0:
                sync.zero_()
                raise RuntimeError("fused MLP step: the terminal head + apply hand-off timed "
                                   "out (the last update was not applied)")
        self._unchecked = False  # verified

    def run(self, steps, use_graph=True, lead=0):
        """Run ``steps`` training steps (epoch-aligned hipGraph replays).  ``lead`` > 0 (single
        GPU): the first ``lead`` steps are launched directly from C++ so the GPU starts at
        once, and the graph replay of the rest is submitted while they run."""
        steps = int(steps)
        if not use_graph:
            for _ in range(steps):
                self.step()
            return
        if lead > 0 and self.host_loop_ok:
            k = min(int(lead), steps)
            self.run_launched(k)
            steps -= k
        if steps > 0 and not self.direct and not self.pending:
            self.step()  # the first DP step has nothing to apply
            steps -= 1
        for n in self._plan(steps):
            self._graph(n).replay()
            self.pos = (self.pos + n) % self.nbatches
            if not self.direct and not self._inplace:
                self.cur ^= n & 1
            if self.shuffle and self.pos == 0:  # the next epoch's gather, between two replays
                self._wrapped()

    def prepare(self, steps, lead=0):
        """Capture (not run) every graph a following ``run(steps, lead=lead)`` replays."""
        steps = int(steps)
        if steps > 0 and not self.direct and not self.pending:
            raise RuntimeError("prepare() in DP mode needs one eager step first")
        pos, cur, epoch = self.pos, self.cur, self.epoch
        if lead > 0 and self.host_loop_ok:
            k = min(int(lead), steps)
            if self.shuffle:
                self._bind(self.epoch + (self.pos + k) // self.nbatches)
            self.pos = (self.pos + k) % self.nbatches
            self.cur ^= k & 1
            steps -= k
        for n in self._plan(steps):
            self._graph(n)
            self.pos = (self.pos + n) % self.nbatches
            if not self.direct and not self._inplace:
                self.cur ^= n & 1
            if self.shuffle and self.pos == 0:
                self._bind(self.epoch + 1)  # (host mirrors only: which buffer the graph reads)
        self.pos, self.cur = pos, cur
        if self.shuffle:
            self._bind(epoch)

    # -- observability ------------------------------------------------------
    def stats(self, step=None):
        """(loss, accuracy) recorded by the kernel for ``step`` (default: last)."""
        self._verified()
        if self.pipelined and self.pending:
            self.flush()  # the last step's record is written by its apply
        s = (self.global_step() - 1) if step is None else int(step)
        v = self.ws.stats[s % self.ws.stats_ring].tolist()
        return float(v[0]), float(v[1])

    def stats_range(self, start, end):
        """Loss/accuracy for steps [start, end) as a CPU tensor [n, 2]."""
        self._verified()
        if self.pipelined and self.pending:
            self.flush()
        ring = self.ws.stats_ring
        if end - start > ring:
            start = end - ring
        idx = torch.arange(start, end) % ring
        return self.ws.stats[idx.to(self.device)].cpu()

    def _rates(self):
        """The rate ring, every step run so far recorded (a step's rate is written by the
        launch that applies it: a pending update is applied first, as ``stats()`` does)."""
        if self.sched is None:
            raise RuntimeError("learning_rate(): the trainer has no lr_schedule (the rate is "
                               "the constant learning_rate)")
        self._verified()
        if self.pending and (self.pipelined or self._inplace):
            self.flush()
        return self.opt.rates

    def learning_rate(self, step=None):
        """The rate the kernel applied for ``step`` (default: the last step), as f32."""
        r = self._rates()
        s = (self.global_step() - 1) if step is None else int(step)
        return float(r[s % self.ws.stats_ring].item())

    def learning_rates(self, start, end):
        """The applied rates of steps [start, end) as a CPU f32 tensor [n]."""
        r = self._rates()
        ring = self.ws.stats_ring
        if end - start > ring:
            start = end - ring
        idx = torch.arange(start, end) % ring
        return r[idx.to(self.device)].cpu()


def _flush_fused():
    """Whether run_launched(.., flush=True) folds the flush into the last head (the opt-in
    DTFX_MLP_FLUSH_FUSED form): the setter returns the previous setting, so read and restore."""
    from ..ops._ext import hip

    h = hip()
    on = h.mlp_set_flush_fused(0)
    h.mlp_set_flush_fused(on)
    return bool(on)


def benchmark_steps(trainer, steps, warmup, barrier=None, use_graph=True):
    """Time exactly ``steps`` steps after ``warmup`` (synchronised both sides)."""
    trainer.run(warmup, use_graph)
    if use_graph:
        trainer.prepare(steps)
    if barrier:
        barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.run(steps, use_graph)
    torch.cuda.synchronize()
    if barrier:
        barrier()
    return time.perf_counter() - t0
