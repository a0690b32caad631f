"""Cost of synchronous replicas on the GPU-resident parameter store.

``--part push``: device time of one sync push (join + push launches, R = 1, n = 79510)
against the async ``push_apply``, timed with events over blocks of queued calls, the two
interleaved block by block in one process; and the host time of a whole ``sync_begin``
(launches + read-back + stream wait) against ``push_apply`` + ``fetch_add``.

``--part cluster``: steps/s of 1 ps + two ``--sync_replicas`` workers sharing one GPU, with
the variables in the GPU store (``--ps_device gpu``) against the TCP parameter server
(``--ps_device cpu``: the only way before the GPU rounds existed, the baseline), run
alternately; the GPU-store workers also report their host polls per round.

``--part optim``: device time of one push per optimizer (sgd, momentum, adam; n = 79510):
the async apply, and the sync push with R = 1 through ``sync_enqueue`` (every push closes its
round and runs the optimizer), six variants interleaved block by block in one process.

    python tools/probes/gpu_ps_sync_cost.py --part push
    python tools/probes/gpu_ps_sync_cost.py --part optim
    python tools/probes/gpu_ps_sync_cost.py --part cluster --steps 6000 --reps 2
"""
import argparse
import glob
import json
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def part_push(a):
    import torch

    from distributedtensorflowexample_amd.ops import hip, mlp_step
    from distributedtensorflowexample_amd.ops._ext import stream_handle

    dev = torch.device("cuda:0")
    n = mlp_step.NPARAM
    s = stream_handle(dev)
    sync_st = hip().GpuParamStore(0, n, True, 1)
    async_st = hip().GpuParamStore(0, n, True)
    g = torch.randn(n, device=dev) * 1e-3
    step = 0

    def sync_block(k):
        nonlocal step
        for _ in range(k):
            sync_st.sync_enqueue(g.data_ptr(), 0.01, step, s)
            step += 1

    def async_block(k):
        for _ in range(k):
            async_st.push_apply(g.data_ptr(), 0.01, False, s)

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(k)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k  # us per call

    for fn in (sync_block, async_block):
        timed(fn, a.block)  # warm-up: code load, first launches
    dev_us = {"sync": [], "async": []}
    for _ in range(a.blocks):  # interleaved: clocks and neighbours change together for both
        dev_us["sync"].append(timed(sync_block, a.block))
        dev_us["async"].append(timed(async_block, a.block))
    rnd, taken = sync_st.sync_poll(s)
    assert (rnd, taken) == (step, 0), (rnd, taken, step)  # every queued push closed its round

    # whole host calls, one at a time (what a worker's step pays)
    host_us = {"sync_begin": [], "push_apply+fetch_add": [], "sync_poll": []}
    for _ in range(a.blocks * 20):
        t0 = time.perf_counter()
        sync_st.sync_begin(g.data_ptr(), 0.01, step, s, 0, 0)
        t1 = time.perf_counter()
        async_st.push_apply(g.data_ptr(), 0.01, False, s)
        async_st.fetch_add(0, 1, s)
        t2 = time.perf_counter()
        sync_st.sync_poll(s)
        t3 = time.perf_counter()
        step += 1
        host_us["sync_begin"].append((t1 - t0) * 1e6)
        host_us["push_apply+fetch_add"].append((t2 - t1) * 1e6)
        host_us["sync_poll"].append((t3 - t2) * 1e6)

    def summary(v):
        v = sorted(v)
        return {"median_us": round(statistics.median(v), 2), "min_us": round(v[0], 2),
                "max_us": round(v[-1], 2), "n": len(v)}

    print(json.dumps({"part": "push", "n": n, "R": 1, "calls_per_block": a.block,
                      "device_time_per_call": {k: summary(v) for k, v in dev_us.items()},
                      "host_time_per_call": {k: summary(v) for k, v in host_us.items()}}))
    sync_st.close()
    async_st.close()
    return 0


def part_optim(a):
    import torch

    from distributedtensorflowexample_amd.ops import hip, mlp_step
    from distributedtensorflowexample_amd.ops._ext import stream_handle
    from distributedtensorflowexample_amd.parallel import gpu_ps_optim

    dev = torch.device("cuda:0")
    n = mlp_step.NPARAM
    s = stream_handle(dev)
    g = torch.randn(n, device=dev) * 1e-3
    stores, blocks = [], {}
    for kind in gpu_ps_optim.KINDS:
        k, hyper = gpu_ps_optim.num_slots(kind), gpu_ps_optim.hyper_args(kind)
        async_st = hip().GpuParamStore(0, n, True, 0, k)
        sync_st = hip().GpuParamStore(0, n, True, 1, k)
        stores += [async_st, sync_st]
        step = [0]

        def async_block(count, st=async_st, hyper=hyper):
            for _ in range(count):
                if hyper:
                    st.push_apply_opt(g.data_ptr(), 0.001, *hyper, s)
                else:
                    st.push_apply(g.data_ptr(), 0.001, False, s)

        def sync_block(count, st=sync_st, hyper=hyper, step=step):
            for _ in range(count):
                st.sync_enqueue(g.data_ptr(), 0.001, step[0], s, *hyper)
                step[0] += 1

        blocks["async " + kind] = async_block
        blocks["sync " + kind] = sync_block

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(k)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k  # us per call

    for fn in blocks.values():
        timed(fn, a.block)  # warm-up: code load, first launches
    dev_us = {name: [] for name in blocks}
    for _ in range(a.blocks):  # interleaved: clocks and neighbours change together for all
        for name, fn in blocks.items():
            dev_us[name].append(timed(fn, a.block))
    for st in stores[1::2]:  # every queued sync push closed its round
        assert st.sync_poll(s) == ((a.blocks + 1) * a.block, 0)

    def summary(v):
        v = sorted(v)
        return {"median_us": round(statistics.median(v), 2), "min_us": round(v[0], 2),
                "max_us": round(v[-1], 2), "n": len(v)}

    print(json.dumps({"part": "optim", "n": n, "R": 1, "calls_per_block": a.block,
                      "device_time_per_push": {k: summary(v) for k, v in dev_us.items()}}))
    for st in stores:
        st.close()
    return 0


def part_cluster(a):
    from distributedtensorflowexample_amd.launch import launch_ps

    runs = []
    for rep in range(a.reps):
        for ps_device in ("cpu", "gpu"):  # alternately: the machine's state drifts for both
            tmp = tempfile.mkdtemp(prefix="pssync")
            t0 = time.perf_counter()
            rc = launch_ps(2, 1, None, 1, base_port=a.base_port + 10 * len(runs),
                           log_dir=os.path.join(tmp, "logs"), quiet=True, timeout=a.timeout,
                           extra=["--training_steps", str(a.steps), "--log_every",
                                  str(a.log_every), "--eval_every", str(10 ** 9), "--logdir",
                                  os.path.join(tmp, "m"), "--save_model_secs", "1e9",
                                  "--save_summaries_secs", "1e9", "--batch_size", "100",
                                  "--ps_device", ps_device, "--sync_replicas"])
            wall = time.perf_counter() - t0
            speeds, polls = [], []
            for p in glob.glob(os.path.join(tmp, "logs", "worker*.log")):
                txt = open(p).read()
                for m in re.finditer(r"step: (\d+)\t\| cost: [^|]+\| speed: ([0-9.eE+-]+)step/sec",
                                     txt):
                    if int(m.group(1)) > 2 * a.log_every:  # skip warm-up prints
                        speeds.append(float(m.group(2)))
                polls += [float(m.group(1)) for m in
                          re.finditer(r"sync rounds: ([0-9.]+) host polls per round", txt)]
            run = {"ps_device": ps_device, "rep": rep, "rc": rc, "wall_seconds": round(wall, 1),
                   "steps_per_sec": round(statistics.median(speeds), 1) if speeds else None,
                   "n_speed_samples": len(speeds),
                   "host_polls_per_round": [round(p, 2) for p in polls]}
            runs.append(run)
            print(json.dumps(run), flush=True)
            if any(rc.values()) or not speeds:
                return 1
    med = {d: statistics.median(r["steps_per_sec"] for r in runs if r["ps_device"] == d)
           for d in ("cpu", "gpu")}
    print(json.dumps({"part": "cluster", "num_workers": 2, "steps": a.steps,
                      "steps_per_sec_tcp_ps": med["cpu"], "steps_per_sec_gpu_store": med["gpu"],
                      "gpu_over_tcp": round(med["gpu"] / med["cpu"], 3)}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["push", "optim", "cluster"], required=True)
    ap.add_argument("--block", type=int, default=200, help="push: calls queued per timed block")
    ap.add_argument("--blocks", type=int, default=20, help="push: timed blocks per variant")
    ap.add_argument("--steps", type=int, default=6000)
    ap.add_argument("--log_every", type=int, default=500)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--base_port", type=int, default=25222)
    ap.add_argument("--timeout", type=float, default=240.0)
    a = ap.parse_args()
    return {"push": part_push, "optim": part_optim, "cluster": part_cluster}[a.part](a)


if __name__ == "__main__":
    sys.exit(main())
