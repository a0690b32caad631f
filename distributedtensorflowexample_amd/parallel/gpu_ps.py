"""GPU-resident parameter store for the async-PS mode (``--ps_device gpu``).

The reference keeps its global variables on the ps task (``replica_device_setter``,
worker.py:24-32) and moves them over gRPC every step: a pull of 318 KB (worker.py:131), a
push + remote ``ApplyGradientDescent`` (worker.py:79,135-137) and an ``AssignAdd`` on
``global_step`` (worker.py:32,141).  This store keeps the same variables -- same TF names,
same semantics (lock-free apply unless ``use_locking``, ``fetch_add`` returning the old step)
-- in ONE uncached allocation on the chief worker's GPU (``csrc/kernels/gpu_ps.cpp``); every
other worker maps it over IPC, so a pull is a peer read and an apply a peer read-modify-write
over xGMI, issued from the worker's own stream with no host copy of parameters or gradients.

The TCP parameter server stays the control plane only: it carries the allocation's IPC handle,
a detach counter (the owner frees the memory only after every other worker detached, so
no peer is ever left with a dangling mapping; a peer that never detaches within the close
timeout leaves the allocation alive until the owner's process exits) and a store generation.

Failure semantics differ from the reference's in one respect: the variables live in the
CHIEF's process, not on the ps task, so a chief failure loses them (a restarted chief
restores the last checkpoint into a NEW store).  The chief bumps the generation at every
``create()``; the other workers compare it periodically (``check_generation``) and exit
non-zero instead of training on a stale mapping.  Checkpoint / restore / readiness read and
write the GPU store (``read_all`` / ``assign`` / ``uninitialized``), so the Supervisor and
Saver work unchanged.

``--sync_replicas`` (``sync_replicas = R >= 1``): the allocation also holds a sync control
region and R gradient slots, and a step is pull, compute, :meth:`GpuPSStore.sync_push_flat`
-- TF's ``SyncReplicasOptimizer`` on the device: a ticket of the open round, the gradient into
the ticket's slot, the mean of the R slots applied ONCE by the last arrival of each 1024-float
chunk, ``global_step`` advanced by the block that finishes the round.  No kernel waits on
another process; the wait for the round to close is a host poll (``parallel/gpu_ps_sync.py``).

``optimizer="momentum" | "adam"`` (``--optimizer``): the allocation ends with the optimizer's
slot planes (``parallel/gpu_ps_optim.py``), one parameter-sized plane per slot, and the store's
apply kernels update them -- in the async apply and in a sync round's closer.  The slots are
variables like the others: ``global/dense/kernel/Momentum``, ``.../Adam``, ``.../Adam_1`` in
``uninitialized`` / ``assign`` / ``pull`` / ``read_all``, in TF layout (a kernel's slot is
transposed exactly as the kernel is).  Adam's ``t`` is ``global_step + 1`` at apply time.

Internal layout: the flat MLP buffer of ``ops/mlp_step.py`` (W1 stored [out, in]); TF layouts
are converted at the ``assign`` / ``pull`` / ``read_all`` boundary.
"""
from __future__ import annotations

import time

import numpy as np
import torch

from ..ops import mlp_step
from ..ops._ext import hip, stream_handle
from . import gpu_ps_optim, gpu_ps_sync
from .ps import PSVariableStore

HANDLE = "gpu_ps/ipc_handle"
DETACHED = "gpu_ps/detached"
GENERATION = "gpu_ps/generation"
STEP_SLOT, INIT_SLOT = 0, 1


VAR_NAMES = ("global/dense/kernel", "global/dense/bias", "global/dense_1/kernel",
             "global/dense_1/bias")


def _flat_from_tf(values, out, names=VAR_NAMES):
    W1t, b1, W2t, b2 = mlp_step.unflatten(out)
    k1, c1, k2, c2 = names
    W1t.copy_(torch.as_tensor(values[k1]).t())
    b1.copy_(torch.as_tensor(values[c1]))
    W2t.copy_(torch.as_tensor(values[k2]).t())
    b2.copy_(torch.as_tensor(values[c2]))
    return out


def _tf_from_flat(p, names=VAR_NAMES):
    W1t, b1, W2t, b2 = mlp_step.unflatten(p)
    k1, c1, k2, c2 = names
    return {k1: W1t.t().contiguous(), c1: b1.clone(), k2: W2t.t().contiguous(), c2: b2.clone()}


class GpuPSStore:
    """Drop-in for ``PSVariableStore`` (the MLP's GLOBAL_SPECS) with the variables in GPU
    memory.  ``create()`` (chief) allocates on ``device``; ``lookup()`` (other workers) opens
    the chief's allocation.  Fast path: ``pull_into`` / ``push_apply_flat`` on device
    buffers."""

    STEP = "global/global_step"

    def __init__(self, ps_addresses, device, num_workers, setter=None, connect_timeout=120.0,
                 sync_replicas=0, optimizer="sgd", momentum=gpu_ps_optim.DEFAULTS["momentum"],
                 beta1=gpu_ps_optim.DEFAULTS["beta1"], beta2=gpu_ps_optim.DEFAULTS["beta2"],
                 epsilon=gpu_ps_optim.DEFAULTS["epsilon"]):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("GpuPSStore needs a GPU device")
        self.num_workers = int(num_workers)
        self.sync_replicas = int(sync_replicas)
        if self.sync_replicas < 0:
            raise ValueError("gpu_ps: sync_replicas must be >= 0")
        self._rounds = None
        # the optimizer's slot planes: [[TF names of plane k]], and the kernels' hyper words
        self.optimizer = gpu_ps_optim.check_kind(optimizer)
        self.slot_names = gpu_ps_optim.slot_names(self.optimizer, VAR_NAMES)
        self._hyper = gpu_ps_optim.hyper_args(self.optimizer, momentum, beta1, beta2, epsilon)
        nbytes = hip().GpuParamStore.handle_size()
        self._hwords = nbytes // 4
        self.ctl = PSVariableStore(ps_addresses, [(HANDLE, (self._hwords,), "float32"),
                                                  (DETACHED, (), "int64"),
                                                  (GENERATION, (), "int64")],
                                   connect_timeout=connect_timeout, setter=setter)
        self.generation = None
        self._kept_alive = None  # an allocation a peer never detached from (owner)
        self.n = mlp_step.NPARAM
        self._st = None
        self._owner = False
        self._host = torch.empty(self.n, dtype=torch.float32, pin_memory=True)

    # -- bring-up -----------------------------------------------------------
    def create(self):
        """Chief: allocate the store on this GPU and publish its IPC handle."""
        self.ctl.create()
        self._st = self._new_store(True)
        self._owner = True
        h = np.frombuffer(self._st.handle(), dtype=np.float32).copy()
        self.ctl.assign({DETACHED: 0})
        if GENERATION in self.ctl.uninitialized():  # first store of this ps
            self.ctl.assign({GENERATION: 1})
            self.generation = 1
        else:  # a restarted chief: a new store generation
            self.generation = self.ctl.fetch_add(GENERATION, 1) + 1
        self.ctl.assign({HANDLE: torch.from_numpy(h)})
        return self

    def lookup(self, timeout=120.0, poll=0.05):
        """Non-chief: wait for the chief's handle, then map the store."""
        self.ctl.lookup(timeout=timeout, poll=poll)
        t0 = time.time()
        while True:
            if not self.ctl.uninitialized():
                h = self.ctl.pull([HANDLE])[HANDLE].numpy().tobytes()
                if any(h):
                    break
            if time.time() - t0 > timeout:
                raise TimeoutError("gpu_ps: the chief never published the store")
            time.sleep(poll)
        self.generation = self.ctl.read_int(GENERATION)
        self._st = self._new_store(False)
        self._st.open(h)  # raises if the chief's store has another sync_replicas
        return self

    def _new_store(self, owner):
        if not self.sync_replicas and not self.slot_names:
            # the async sgd store: exactly the allocation it always was
            return hip().GpuParamStore(self.device.index or 0, self.n, owner)
        args = (self.device.index or 0, self.n, owner, self.sync_replicas)
        if self.slot_names:  # the planes behind everything else
            args += (len(self.slot_names),)
        st = hip().GpuParamStore(*args)
        if self.sync_replicas:
            self._rounds = gpu_ps_sync.SyncRounds(st, self.sync_replicas,
                                                  stream=lambda: stream_handle(self.device),
                                                  hyper=self._hyper)
        return st

    def check_generation(self):
        """Non-chief: raise if the chief re-created the store since ``lookup`` (its process
        restarted: this worker's mapping no longer holds the global variables)."""
        if self._owner or self.generation is None:
            return
        g = self.ctl.read_int(GENERATION)
        if g != self.generation:
            raise RuntimeError("gpu_ps: the chief re-created the parameter store (generation "
                               "%d -> %d); this worker's mapping is stale" % (self.generation, g))

    def _ctrl(self, slot, delta):
        return int(self._st.fetch_add(slot, int(delta), stream_handle(self.device)))

    def uninitialized(self):
        """report_uninitialized_variables: every variable until the first assign."""
        if self._st is None or self._ctrl(INIT_SLOT, 0) == 0:
            return (list(VAR_NAMES) + [self.STEP]
                    + [name for plane in self.slot_names for name in plane])
        return []

    def assign(self, values):
        """Init / restore: {TF name: tensor/array/int}; the float variables are assigned
        together (all four are required), so are the optimizer's slot variables (every slot
        of every variable), global_step alone is allowed."""
        slots = [name for plane in self.slot_names for name in plane]
        given = [k for k in values if k in slots]
        floats = [k for k in values if k != self.STEP and k not in slots]
        if floats:
            if len(floats) != 4:
                raise ValueError("gpu_ps: assign all four float variables together")
            _flat_from_tf(values, self._host)
            self._st.write(self._host.data_ptr(), 0, self.n * 4)
        if given:
            if len(given) != len(slots):
                raise ValueError("gpu_ps: assign the %s optimizer's %d slot variables together"
                                 % (self.optimizer, len(slots)))
            for k, plane in enumerate(self.slot_names):
                _flat_from_tf(values, self._host, plane)
                self._st.write(self._host.data_ptr(), self._st.opt_offset(k), self.n * 4)
        if self.STEP in values:
            s = int(torch.as_tensor(values[self.STEP]).item())
            if self.sync_replicas:  # also the round word (step << 32); counters re-armed
                torch.cuda.synchronize(self.device)
                self._st.set_step(s)
                self._rounds.joined_round = None
            else:
                cur = self._ctrl(STEP_SLOT, 0)
                self._ctrl(STEP_SLOT, s - cur)
        if self._ctrl(INIT_SLOT, 0) == 0:
            self._ctrl(INIT_SLOT, 1)

    # -- per-step traffic -----------------------------------------------------
    def pull_into(self, dst):
        """sync_op on the device: dst (flat f32 [NPARAM] on this GPU) <- store."""
        self._st.pull(dst.data_ptr(), stream_handle(self.device))

    def push_apply_flat(self, grad, lr, use_locking=False):
        """ApplyGradientDescent (or the store's ApplyMomentum / ApplyAdam, slots included) on
        the store from a flat device gradient (stream-ordered)."""
        if self.slot_names:
            if use_locking:
                raise ValueError("gpu_ps: use_locking needs the sgd optimizer")
            self._st.push_apply_opt(grad.data_ptr(), float(lr), *self._hyper,
                                    stream_handle(self.device))
            return
        self._st.push_apply(grad.data_ptr(), float(lr), bool(use_locking),
                            stream_handle(self.device))

    def pull(self, names=None):
        """{TF name: CPU tensor} of the variables and the optimizer's slots (or of ``names``):
        one host read per plane, as many as ``names`` needs."""
        host = torch.empty(self.n, dtype=torch.float32, pin_memory=True)  # saver thread too
        planes = [(0, VAR_NAMES)] + [(self._st.opt_offset(k), plane)
                                     for k, plane in enumerate(self.slot_names)]
        v = {}
        for off, plane in planes:
            if names is None or any(k in plane for k in names):
                self._st.read(host.data_ptr(), off, self.n * 4)
                v.update(_tf_from_flat(host, plane))
        return {k: v[k] for k in (names or v)}

    def push_apply(self, grads, lr, use_locking=False):
        g = _flat_from_tf(grads, torch.zeros(self.n, dtype=torch.float32)).to(self.device)
        self.push_apply_flat(g, lr, use_locking)
        torch.cuda.synchronize(self.device)

    # -- synchronous replicas ---------------------------------------------------
    def _need_sync(self):
        if self._rounds is None:
            raise RuntimeError("gpu_ps: the store was built without sync_replicas "
                               "(or is not created / looked up yet)")
        return self._rounds

    def sync_push_flat(self, grad, lr, local_step, timeout_s=60.0, record=None):
        """One synchronous-replicas step from a flat device gradient: join the round
        ``local_step`` and push (two launches, one read-back), then poll on the host until the
        round has closed.  Returns ``(step, applied, record)``: the new global step (the next
        local step), whether this gradient is part of the applied mean, and the floats of
        ``record`` (a small f32 device tensor: the step's loss / accuracy) read back in the
        same copy.  A stale push (the round closed without it) returns ``(current step,
        False, ...)`` at once; a backup replica's push into a full round waits for the close
        and returns ``(step, False, ...)``.

        Unlike the TCP parameter server, a push that times out (``TimeoutError`` naming the
        round and ``k of R``) is NOT withdrawn: its slot may already be counted.  Keep
        waiting with :meth:`sync_push_wait`; pushing again for the same round is refused."""
        r = self._need_sync()
        ptr, k = (record.data_ptr(), record.numel()) if record is not None else (0, 0)
        return r.push(grad.data_ptr(), lr, local_step, timeout_s, ptr, k)

    @property
    def sync_polls(self):
        """Host polls of the round word so far (all rounds)."""
        return self._rounds.polls if self._rounds is not None else 0

    def sync_push_wait(self, local_step, timeout_s=60.0):
        """Wait (host poll) until the round ``local_step`` has closed; -> the new global step."""
        return self._need_sync().wait(local_step, timeout_s)

    def sync_push(self, grads, lr, replicas_to_aggregate, local_step,
                  step_name="global/global_step", timeout_s=600.0):
        """``PSVariableStore.sync_push`` on the GPU store: {TF name: tensor} gradients (as
        ``push_apply`` takes them) -> ``(new_global_step, applied)``.  The store's R is fixed
        at creation: another ``replicas_to_aggregate`` is a ValueError."""
        if step_name != self.STEP:
            raise KeyError(step_name)
        if int(replicas_to_aggregate) != self.sync_replicas:
            raise ValueError("gpu_ps: the store aggregates %d replicas per round, not %d"
                             % (self.sync_replicas, int(replicas_to_aggregate)))
        self._need_sync()
        g = _flat_from_tf(grads, torch.zeros(self.n, dtype=torch.float32)).to(self.device)
        step, applied, _ = self.sync_push_flat(g, lr, local_step, timeout_s)
        return step, applied

    def fetch_add(self, name, delta=1):
        if name != self.STEP:
            raise KeyError(name)
        if self.sync_replicas and int(delta) != 0:
            raise RuntimeError("gpu_ps: with sync_replicas the rounds own global_step "
                               "(assign it; a round advances it)")
        return self._ctrl(STEP_SLOT, delta)

    def fetch_add_record(self, record, delta=1):
        """global_step fetch-add that also reads back ``record`` (a small f32 device tensor:
        the step's loss / accuracy) in the same copy -- one host round trip per step."""
        if self.sync_replicas and int(delta) != 0:
            raise RuntimeError("gpu_ps: with sync_replicas the rounds own global_step")
        old, vals = self._st.fetch_add_read(STEP_SLOT, int(delta), stream_handle(self.device),
                                            record.data_ptr(), record.numel())
        return int(old), vals

    def read_int(self, name):
        return self.fetch_add(name, 0)

    def read_all(self):
        out = self.pull()
        out[self.STEP] = torch.tensor(self.read_int(self.STEP), dtype=torch.int32)
        return out

    def close(self, timeout=60.0, poll=0.05):
        """Detach (non-owner) or wait for every other worker to detach, then free (owner).

        Owner: once the wait ends the published handle is cleared BEFORE anything is freed,
        so a worker that looks the store up later fails cleanly instead of mapping memory
        about to be freed (one that joins during the wait trains and detaches).  If some peer has not
        detached within ``timeout`` seconds the allocation is NOT freed (a peer may still be
        pulling or applying through its mapping): it stays alive until this process exits,
        with a warning."""
        if self._st is None:
            return
        torch.cuda.synchronize(self.device)
        if self._owner:
            t0 = time.time()
            while (self.ctl.read_int(DETACHED) < self.num_workers - 1
                   and time.time() - t0 < timeout):
                time.sleep(poll)
            # late lookups from here on find no handle and fail cleanly
            self.ctl.assign({HANDLE: torch.zeros(self._hwords)})
            missing = self.num_workers - 1 - self.ctl.read_int(DETACHED)
            if missing > 0:
                import warnings

                warnings.warn("gpu_ps: %d worker(s) never detached within %.0f s; the store "
                              "stays allocated until this process exits" % (missing, timeout))
                self._kept_alive = self._st
            else:
                self._st.close()
        else:
            self._st.close()
            self.ctl.fetch_add(DETACHED, 1)
        self._st = None
