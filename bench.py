#!/usr/bin/env python3
"""RBC data-path benchmark (BASELINE.json metric: "RBC shard GB/s (RS
encode+decode + Merkle verify) per GPU & node, N=128").

One step = one full RBC round of the data path over the instances this rank
owns, resident in HBM (default C2: N=128, f=42, 1 MiB values, 1024 per GPU):
  1. shard+commit   rbc_dev_encode (Split+Encode), rbc_dev_leaves (SHA-256 of
                    every shard), rbc_dev_merkle_build (root + N branches)
  2. Byzantine input: 10 % of instances get one corrupted ECHO shard
  3. receive        ECHO verify of the N-f received shards (validateMessage)
                    and interpolate from the first k valid: regenerate the
                    other positions, re-hash them, recheck the root, digest
  4. (N GPUs > 1)   RCCL all-gather of the {root, digest} records over xGMI
value = instances x N x S bytes of committed shard output per step, summed
over all ranks, / (max over ranks of the timed wall time).

Schedules: --pipeline 7 (default) commits batch t on the proposer stream
while the receiver stream runs rbc_dev_receive_step(cur = t-1, prev = t-2);
--pipeline 0 runs the stages in order on one stream, and is what the bench
falls back to when the pipeline's shard sets do not fit the HBM this rank
may use (free device memory / ranks sharing the device).  Interpolate's
value is the joined form rbc/rbc.go:88 returns (k*S contiguous bytes per
instance); --row-view times the row view instead (the k data rows of the
shard set, no join), and a shorter second run reports the other form.

A plain run (`bench.py --gpus 1 --steps N --warmup W`) sets up, warms up,
times the N steps and prints the headline line: metric, value, ms_per_step,
the configuration, the timed steps' own event spans (stage_ms) and the ranks'
records.  --dump-outputs DIR also writes what the last timed step computed
(dump_outputs below; the inputs are seeded, so two builds can be compared
array for array).  Everything else runs only under --full, after the timed
steps unless noted: the isolated serial steps (before the warmup), the
correctness guard (every instance decoded to its input, the poisoned receive,
roots / digests against the C oracle, the gathered records; exit 3 when it
fails), the second value-form leg, the rooflines, the CPU baseline, the
host-fed epoch and the batcher sweep.  The --no-* switches below trim a
--full run.

Host-fed leg (--full; every rank, after the device-resident timing; key
pcie_inclusive, never `value`): one epoch of the rank's instances through the
C ABI from pinned NUMA-local host memory -- rbc_shard_commit,
rbc_validate_packed_leaves of every received ECHO and
rbc_interpolate_batch_verified -- all ranks at once (tools/host_bench.epoch).

Scaling: by default every GPU owns `instances` (weak scaling, as the driver
runs N = 1, 2, 4, 8).  --total-instances T partitions T instances over the
ranks in contiguous blocks (strong scaling; BASELINE configs[3] is
`--config c3 --total-instances 8192`).  For N > 1: under torch.distributed.run,
or directly (the process spawns its N ranks before touching any GPU).  Host
coordination is loopback TCP (cleisthenes_amd.rendezvous), never torch, so the
HIP runtime and RCCL that librbc_gpu.so links are the ones mapped; every rank
runs under a watchdog that names its stage if it hangs or fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from cleisthenes_amd import launch  # noqa: E402  (no GPU, no torch)

CONFIGS = {
    # name: (N, f, value bytes, instances per GPU, description)
    "c1": (64, 21, 1 << 20, 1024, "N=64 f=21 1MiB"),
    "c2": (128, 42, 1 << 20, 1024, "N=128 f=42 1MiB"),
    "c3": (128, 42, 4 << 20, 1024, "N=128 f=42 4MiB"),
    "c4": (256, 85, 64 << 10, 16384, "N=256 f=85 64KiB"),
}
# Pipelined issue level of interpolate's GEMV / FFT re-encode (c: commit side, r: receive side):
# the GEMV at r balances the streams at N = 128 and starves C1's one-wave-per-SIMD leaf hashing
# (tools/gpu_runs/gpu_r03t.sh)
DECODE_PRIO = {"c1": "c,c", "c2": "r,c", "c3": "r,c", "c4": "r,c"}
# Stream that verifies each batch's received ECHOs under the pipeline: the receiver's step (one SHA launch
# with the previous batch's regen rows), or the proposer's stream right after the commit it depends on
# (rbc_dev_verify, then the receive step takes the batch as verified) -- VERDICT r05 item 4's A/B at C4
VERIFY_ON = {"c1": "receiver", "c2": "receiver", "c3": "receiver", "c4": "receiver"}
METRIC = "RBC shard GB/s (RS encode+decode + Merkle verify) per GPU & node, N=128"
SEED = 20261015
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md chip table (spec)
# SHA-256 VALU roof: v_alignbit / v_add3 / v_perm 4 clk, v_bitop3 / v_add /
# shifts 2 clk per wave64 instruction (profiles/r01_valu_probe.txt); the
# compression loop issues 833 four-clock + 576 two-clock instructions.
SHA_PEAK_CPS = 1024 * 2.4e9 / (833 * 4 + 576 * 2) * 64
# attainable: the same compression register-resident at 8 waves per SIMD
# (profiles/r01_sha_probe.txt, 5782 clk at the nominal 2.4 GHz)
SHA_PROBE_CPS = 1024 * 2.4e9 / 5782 * 64
# the same probe's dependency-limited rate at 4 waves per SIMD (the row-hashing kernels' occupancy):
# 6131 SIMD clk per wave-compression of 1418 wave64 VALU instructions
SHA_CHAIN_CLK_PER_INSTR = 6131 / 1418
GiB = 1 << 30


def round_up(x, a):
    return (x + a - 1) // a * a


def parse_args(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=150,
                    help="timed steps (the default keeps ~1 s of GPU work in the timed region at C2)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every check and secondary measurement (see the module "
                         "docstring); without it the run only times the steps and prints the headline line")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (float32; seeded samples of "
                         "the large arrays, at most 64 MB in all)")
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--instances", type=int, default=0, help="instances per GPU (weak scaling; default per config)")
    ap.add_argument("--total-instances", type=int, default=0,
                    help="partition this many instances over the ranks (strong scaling)")
    ap.add_argument("--pipeline", type=int, default=7, choices=(0, 7),
                    help="7: proposer stream commit(t) || receiver stream rbc_dev_receive_step(t-1, t-2); "
                         "0: one stream, stages in order")
    ap.add_argument("--row-view", action="store_true",
                    help="time interpolate's row view (the k data rows, no join) instead of the joined value")
    ap.add_argument("--no-second-form", "--no-joined-leg", dest="no_second_form", action="store_true",
                    help="skip the secondary timed run in the other value form (key value_row_view / value_joined)")
    ap.add_argument("--faults-on", default="receiver", choices=("receiver", "proposer"),
                    help="stream that injects the corrupted ECHO shards (synthetic input; the proposer's when "
                         "it also verifies)")
    ap.add_argument("--verify-on", default="", choices=("", "receiver", "proposer"),
                    help="stream that verifies the received ECHOs under the pipeline (default per config, VERIFY_ON)")
    ap.add_argument("--wave-prio", default="",
                    help="commit,receive s_setprio levels (default 0,2 pipelined, 0,0 serial)")
    ap.add_argument("--decode-prio", default="",
                    help="gemv,reencode levels of interpolate's GF transforms: c (commit level), r (receive "
                         "level) or 0..3 (default per config, DECODE_PRIO; serial: commit level)")
    ap.add_argument("--hbm-budget", type=float, default=0,
                    help="bytes of HBM this rank may use (default: free device memory / ranks sharing the device)")
    ap.add_argument("--shard-align", type=int, default=128,
                    help="shard row pitch alignment in bytes (multiple of 64; the C ABI needs 64)")
    ap.add_argument("--force-gather", action="store_true",
                    help="run the RCCL all-gather even with one rank (exercises rbc_comm_*)")
    ap.add_argument("--no-isolated", action="store_true",
                    help="skip the serial steps before the warmup that time each kernel alone (roofline.isolated)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-configs", default="c1,c2,c3,c4",
                    help="configs the CPU port is also timed on (the bench config always is)")
    ap.add_argument("--no-pcie", action="store_true",
                    help="skip the host-fed (PCIe-inclusive) epoch leg on every rank (secondary key, never `value`)")
    ap.add_argument("--host-instances", type=int, default=0,
                    help="instances per rank in the host-fed epoch (default: the rank's, at most 2 GiB of values)")
    ap.add_argument("--no-batcher", action="store_true",
                    help="skip the per-message validate lane sweep (secondary key `batcher`, C2 only, never `value`)")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="the N-rank path on a 1-GPU box: every rank on device 0, RCCL skipped; spawn, "
                         "rendezvous, partition, HBM plan, checks and max-over-ranks run as on N GPUs")
    ap.add_argument("--oracle-samples", type=int, default=16,
                    help="instances whose root and digest are checked against the C oracle after timing")
    ap.add_argument("--watchdog-scale", type=float, default=1.0, help="multiplies every stage deadline")
    args = ap.parse_args(argv)
    args.join = not args.row_view
    # checked before any rank starts or touches a GPU
    if args.wave_prio and not _levels_ok(args.wave_prio, ()):
        ap.error("--wave-prio takes two levels 0..3, e.g. 0,2")
    if args.decode_prio and not _levels_ok(args.decode_prio, ("c", "r")):
        ap.error("--decode-prio takes two of c, r or 0..3, e.g. r,c")
    return args


def _levels_ok(text, names):
    return len(text.split(",")) == 2 and all(x in names + ("0", "1", "2", "3") for x in text.split(","))


def hbm_plan(I, n, d, spitch, vpitch, opitch, join, world_gather, free, sharing, budget_arg, rx_sets=2):
    """Bytes per shard set / receiver set / the rest, and the schedule that fits."""
    set_b = I * (n * spitch + n * 32 + 32 + n * max(d, 1) * 32)
    rx_b = I * (n + n * 32 + 32 + 4 + (opitch if join else 0))
    other = I * (vpitch + n + 4 + 64) + world_gather + GiB  # + decode workspace, events, slack
    budget = budget_arg or (free / sharing) * 0.97
    need = {"pipelined": 3 * set_b + rx_sets * rx_b + other, "serial": set_b + rx_b + other}
    return {"free_bytes": int(free), "ranks_sharing_device": sharing, "budget_bytes": int(budget),
            "need_bytes": {k: int(v) for k, v in need.items()}}, need


def main(argv):
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch.spawn_ranks(args.gpus, argv, os.path.abspath(__file__))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    if world != args.gpus:
        raise SystemExit(f"bench: WORLD_SIZE={world} but --gpus {args.gpus}")
    # ONE JSON line on stdout: keep a private handle on the real stdout and
    # point fd 1 at stderr, so banners native libraries printf (RCCL's
    # version block) cannot precede it
    out = os.fdopen(os.dup(1), "w")
    sys.stdout.flush()
    os.dup2(2, 1)
    wd = launch.Watchdog(rank, world, args.watchdog_scale)
    try:
        return run(args, world, rank, local_rank, wd, out)
    finally:
        wd.close()


def run(args, world, rank, local_rank, wd, out):
    from cleisthenes_amd.rendezvous import Rendezvous
    with wd.stage("rendezvous", 330):
        rdz = Rendezvous(world, rank)
    import cleisthenes_amd as ca
    from cleisthenes_amd import acs, synth

    n, f, B, inst_default, desc = CONFIGS[args.config]
    if args.total_instances:
        total = args.total_instances
        first, I = acs.partition(total, world, rank)
        scaling = "strong"
    else:
        I = args.instances or inst_default
        total, first, scaling = I * world, rank * I, "weak"
    if I < 1:
        raise SystemExit(f"bench: rank {rank} owns no instances ({total} over {world})")
    dev = 0 if args.rehearse_on_one_gpu else local_rank
    me = {"rank": rank, "device": dev, "pci_bus_id": ca.rbc.pci_bus_id(dev)}
    if world > 1:
        me.update(launch.numa_place(me["pci_bus_id"]))
    wd.info.update(me)

    wd.enter("context + inputs", 300)
    ctx = ca.Context(n, f, device=dev)
    k, d = ctx.k, ctx.depth
    S = (B + k - 1) // k
    spitch = round_up(S, args.shard_align)  # rows start on whole 128-B lines: full-line HBM writes
    vpitch = round_up(k * S + 32, 64)
    opitch = round_up(k * S, 16)
    gather = (world > 1 or args.force_gather) and not args.rehearse_on_one_gpu
    slots = acs.max_share(total, world)
    free, _ = ca.rbc.mem_info(dev)
    pverify = (args.verify_on or VERIFY_ON[args.config]) == "proposer"
    plan, need = hbm_plan(I, n, d, spitch, vpitch, opitch, args.join, world * slots * 64 if gather else 0, free,
                          world if args.rehearse_on_one_gpu else 1, args.hbm_budget, 3 if pverify else 2)
    pipe = args.pipeline == 7 and need["pipelined"] <= plan["budget_bytes"]
    if need["serial"] > plan["budget_bytes"]:
        raise SystemExit(f"bench: rank {rank} needs {need['serial'] / 1e9:.1f} GB for {I} instances, "
                         f"has {plan['budget_bytes'] / 1e9:.1f} GB: use more ranks or fewer instances")
    plan["schedule"] = "pipelined" if pipe else "serial"
    pverify = pverify and pipe
    if pverify:
        args.faults_on = "proposer"  # the corrupted ECHOs must be in place before the proposer-side verify
    tx, rx = (int(x) for x in (args.wave_prio or ("0,2" if pipe else "0,0")).split(","))
    ctx.set_wave_priority(tx, rx)
    lv = {"c": tx, "r": rx}
    gv, rv = (lv[x] if x in lv else int(x)
              for x in (args.decode_prio or (DECODE_PRIO[args.config] if pipe else "c,c")).split(","))
    ctx.set_decode_priority(gv, rv)
    stream = ca.Stream(dev)
    mb = lambda x: ca.DeviceBuffer(x, device=dev)  # noqa: E731
    # ---- synthetic inputs: values on the device (the global instance id
    # seeds each row); present sets / corruptions from one seeded stream over
    # all `total` instances, this rank's slice taken
    d_values = mb(I * vpitch)
    ca.rbc.fill_random(dev, stream.ptr, d_values, first, I, vpitch, SEED)
    rng = np.random.default_rng(SEED)
    present_all = np.zeros((total, n), dtype=np.uint8)
    corrupt_all = np.full(total, -1, dtype=np.int32)
    for i in range(total):
        pres = rng.permutation(n)[: n - f]
        present_all[i, pres] = 1
        if rng.random() < 0.10:
            corrupt_all[i] = int(rng.choice(pres))
    present_h, corrupt_h = present_all[first:first + I], corrupt_all[first:first + I]
    nsets = 3 if pipe else 1
    sets = [dict(shards=mb(I * n * spitch), leaves=mb(I * n * 32), roots=mb(I * 32),
                 branches=mb(I * n * max(d, 1) * 32)) for _ in range(nsets)]
    rxb = [dict(valid=mb(I * n), leaves_r=mb(I * n * 32), digests=mb(I * 32), status=mb(I * 4),
                out=mb(I * opitch) if args.join else None) for _ in range((3 if pverify else 2) if pipe else 1)]
    nrx = len(rxb)
    d_present = mb(I * n)
    d_present.upload(present_h)
    d_corrupt = mb(I * 4)
    d_corrupt.upload(corrupt_h)
    d_count = mb(16)
    d_gather = mb(world * slots * 64) if gather else None
    rccl = None
    if gather:
        wd.enter("rccl init", 120)
        uid = rdz.broadcast_bytes(ca.Context.comm_unique_id() if rank == 0 else None)
        ctx.comm_init(world, rank, uid)
        rccl = ctx.comm_info()
        wd.info["rccl"] = {"nranks": rccl["nranks"], "version": rccl["version_str"]}
        if rccl["nranks"] != world:
            raise SystemExit(f"bench: RCCL reports {rccl['nranks']} ranks, expected {world}")
    me["rccl_nranks"] = rccl["nranks"] if rccl else None

    rstream = ca.Stream(dev) if pipe else stream
    names = ("t0", "enc", "leaf", "tree", "pf", "pv", "r0", "rf", "hb", "rh", "hashed", "dbeg", "ddone", "rend", "gather")
    ev_sets = [{nm: ca.Event() for nm in names} for _ in range(max(args.steps, 20))]  # >= the joined leg's steps
    form = {"join": args.join, "start": 0}  # value form of the receive steps; the first step of a run
    vpo = lambda rb: (rb["out"], opitch) if form["join"] else (None, 0)  # noqa: E731

    def rec(ev, name, st):
        if ev is not None:
            ev[name].record(st)

    def commit(P, sp, ev):
        rec(ev, "t0", P)
        ctx.dev_encode(P.ptr, I, d_values, vpitch, None, B, sp["shards"], spitch)
        rec(ev, "enc", P)
        ctx.dev_leaves(P.ptr, I, sp["shards"], spitch, None, S, sp["leaves"])
        rec(ev, "leaf", P)
        ctx.dev_merkle_build(P.ptr, I, sp["leaves"], sp["roots"], sp["branches"])
        rec(ev, "tree", P)

    def step(ev, sp=None, rb=None):
        """serial schedule: every stage in order on one stream"""
        sp, rb = sp or sets[0], rb or rxb[0]
        commit(stream, sp, ev)
        ctx.dev_inject_faults(stream.ptr, I, sp["shards"], spitch, d_corrupt)
        rec(ev, "pf", stream)
        ctx.dev_verify(stream.ptr, I, sp["shards"], spitch, None, S, sp["branches"], sp["roots"], d_present,
                       rb["valid"], rb["leaves_r"])
        rec(ev, "hashed", stream)
        ctx.dev_interpolate(stream.ptr, I, sp["shards"], spitch, None, S, rb["valid"], rb["leaves_r"], 1, sp["roots"],
                            *vpo(rb), rb["digests"], rb["status"])
        rec(ev, "rend", stream)
        if gather:
            ctx.dev_allgather_records(stream.ptr, I, slots, sp["roots"], rb["digests"], rb["status"], d_gather)
        rec(ev, "gather", stream)

    # pipelined schedule: P commits batch t into set t % 3 once batch t-3 is
    # complete; R runs rbc_dev_receive_step(cur = t-1, prev = t-2): verify(t-1)
    # and the regen hashing of t-2 in one SHA launch, t-2's recheck + digest,
    # then t-1's decode; batch t-2 is complete when its work on R is done
    evP = [ca.Event() for _ in range(nsets)]
    evR = [ca.Event() for _ in range(nsets)]
    for e in evP + evR:
        e.record(stream)
    pending = {}

    def pstep(t, ev=None):
        P, R = stream, rstream
        sp = sets[t % nsets]
        P.wait(evR[t % nsets])
        commit(P, sp, ev)
        if args.faults_on == "proposer":
            ctx.dev_inject_faults(P.ptr, I, sp["shards"], spitch, d_corrupt)
        rec(ev, "pf", P)
        if pverify:  # batch t's ECHO verify right behind its commit, on P (rbc_rx_batch.verified)
            rv = rxb[t % nrx]
            ctx.dev_verify(P.ptr, I, sp["shards"], spitch, None, S, sp["branches"], sp["roots"], d_present,
                           rv["valid"], rv["leaves_r"])
            rec(ev, "pv", P)
        evP[t % nsets].record(P)
        if t == form["start"]:
            return
        x = t - 1
        sr, rb = sets[x % nsets], rxb[x % nrx]
        R.wait(evP[x % nsets])
        rec(ev, "r0", R)
        if args.faults_on == "receiver":
            ctx.dev_inject_faults(R.ptr, I, sr["shards"], spitch, d_corrupt)
        rec(ev, "rf", R)
        cur = ctx.rx_batch(I, sr["shards"], spitch, None, S, sr["branches"], sr["roots"], d_present, rb["valid"],
                           rb["leaves_r"], *vpo(rb), rb["digests"], rb["status"], verified=pverify)
        prev = pending.pop(x - 1, None)
        marks = {nm: ev[key] for nm, key in (("hashed", "hashed"), ("decode_begin", "dbeg"), ("decoded", "ddone"),
                                             ("hash_begin", "hb"), ("rows_hashed", "rh"))} if ev is not None else {}
        # batch t-2's set goes back to P after the whole receive step, not at its prev_released mark
        # (after t-2's recheck): P's encode beside t-1's decode lost 14 % at C4 (gpu_r05q.sh)
        ctx.dev_receive_step(R.ptr, cur, prev, **marks)
        pending[x] = cur
        rec(ev, "rend", R)
        if gather and prev is not None:
            pb = rxb[(x - 1) % nrx]
            ctx.dev_allgather_records(R.ptr, I, slots, sets[(x - 1) % nsets]["roots"], pb["digests"], pb["status"],
                                      d_gather)
        rec(ev, "gather", R)
        if prev is not None:
            evR[(x - 1) % nsets].record(R)

    def barrier():
        rstream.sync()
        stream.sync()
        ca.rbc.lib.rbc_device_sync(dev)
        rdz.barrier()

    # the same kernels alone on the chip (serial steps, events per stage),
    # BEFORE the warmup so that the timed launches stay the last ones a
    # rocprof trace holds: under the pipeline a kernel's span also holds the
    # other stream's work, so the roofline carries both figures
    iso = None
    if pipe and args.full and not args.no_isolated:
        wd.enter("isolated steps", 300)
        for _ in range(2):
            step(None)
        for ev in ev_sets[:3]:
            step(ev)
        stream.sync()
        iso = spans(ev_sets[:3], None)
    wd.enter("warmup", 300)
    warm = max(args.warmup, 3) if pipe else args.warmup  # fill the pipeline: a decode before the guard
    for t in range(warm):
        pstep(t) if pipe else step(None)
    barrier()
    wd.enter("timed loop", 600 + 2.0 * args.steps)
    barrier()
    t0 = time.perf_counter()
    for t in range(args.steps):
        pstep(warm + t, ev_sets[t]) if pipe else step(ev_sets[t])
    barrier()
    elapsed = time.perf_counter() - t0
    elapsed_max = rdz.max(elapsed)
    ms_per_step = elapsed_max * 1000.0 / args.steps
    value = total * n * S * args.steps / elapsed_max / 1e9
    if args.dump_outputs and rank == 0:
        # the last timed step's results, before anything else touches their buffers: the commit of batch t,
        # the receive step's verify + decode of t-1 and its recheck + digest of t-2 (serial: one batch)
        wd.enter("dump outputs", 300)
        t_last = warm + args.steps - 1
        dump_outputs(args.dump_outputs, I, n, k, d, B, S, spitch, opitch, args.join,
                     commit=sets[t_last % nsets], cur_set=sets[(t_last - 1) % nsets],
                     cur=rxb[(t_last - 1) % nrx], prev=rxb[(t_last - 2) % nrx])
    stage_ms = spans(ev_sets[: args.steps], args.faults_on if pipe else None, pverify)
    host = launch.host_info()
    head = {
        "metric": METRIC, "value": round(value, 3), "unit": "GB/s", "n_gpus": world, "steps": args.steps,
        "warmup": warm, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": scaling,
        "vs_baseline": None,  # BASELINE.md publishes no number for this metric
        "vs_baseline_basis": "none published (BASELINE.md); GPU / CPU port on the same host: --full, "
                             "cpu_baseline.gpu_over_cpu",
        "dtype": "u8",
        "data": "synthetic (device-generated splitmix64 bytes per instance, seeded; 10% of instances with one "
                "corrupted ECHO shard)",
        "config": {"workload": f"{args.config}: {desc}, {total} instances ({I} on this rank); shard+commit, "
                               "ECHO verify of the N-f received shards, interpolate from the first k valid",
                   "n": n, "f": f, "value_bytes": B, "shard_bytes": S, "instances_total": total,
                   "instances_per_gpu": I,
                   "parallelism": f"instances partitioned over {world} GPU(s) in contiguous blocks"
                                  + (", RCCL all-gather of {root,digest} records" if gather else ""),
                   "gf_codec": ctx.codec,
                   "wave_priority": {"commit": tx, "receive": rx, "decode_gemv": gv, "decode_reencode": rv},
                   "value_form": "joined (k*S contiguous bytes per instance, the []byte rbc/rbc.go:88 returns)"
                                 if args.join else "row view (the k data rows of the shard set, no join)",
                   "faults_on": args.faults_on, "verify_on": "proposer" if pverify else "receiver",
                   "hbm_plan": plan,
                   **({"rehearsal": "all ranks on device 0, no RCCL (not a multi-GPU measurement)"}
                      if args.rehearse_on_one_gpu else {}),
                   "pipeline": (f"commit(t) || receive step: verify(t-1) + rehash(t-2) in one SHA launch, "
                                f"recheck(t-2), decode(t-1) (rbc_dev_receive_step), two streams, {nsets} shard "
                                "sets") if pipe else "serial"},
        "full": args.full, "rccl": rccl, "library": ca.rbc.library_path(),
        "host": {kk: host[kk] for kk in ("cpu_model", "nproc", "cgroup_cpu_quota", "affinity_cpus")},
    }
    if not args.full:
        # the plain run ends here: the timed steps' own event spans and the ranks' records, no checks
        ranks, skew = rank_timing(rdz, me, elapsed, args.steps, stage_ms)
        wd.leave()
        if rank == 0:
            print(json.dumps({**head, "stage_ms": {kk: round(v, 4) for kk, v in stage_ms.items()},
                              "ranks": ranks, "rank_skew": skew}), file=out, flush=True)
        rdz.barrier()
        rdz.close()
        return 0
    wd.enter("checks", 600)
    if pipe:  # complete the batch the last receive step decoded (outside the timed region)
        x_last, cur = pending.popitem()
        ctx.dev_receive_step(rstream.ptr, None, cur)
        last, rb_last = sets[x_last % nsets], rxb[x_last % nrx]
        if gather:  # the guard checks this batch's gathered records
            ctx.dev_allgather_records(rstream.ptr, I, slots, last["roots"], rb_last["digests"], rb_last["status"],
                                      d_gather)
        rstream.sync()
    else:
        last, rb_last = sets[0], rxb[0]
    timed = check_batch(args, ca, dev, stream, I, n, k, B, S, spitch, vpitch, opitch, d_values, last, rb_last,
                        d_count)

    def poisoned_receive():
        """The receive guard: a fresh commit whose every row the receiver must
        regenerate (absent, or the corrupted ECHO) is overwritten with seeded
        garbage before the same receive path runs on it, so a decode that
        skips a row cannot pass on the proposer's intact bytes."""
        sp, rb = sets[0], rxb[0]
        if args.join:  # the joined values of the timed batch are this input's too: overwrite them first
            ca.rbc.fill_random(dev, stream.ptr, rb["out"], 0, I, opitch, SEED + 2)
        commit(stream, sp, None)
        ca.rbc.poison_rows(dev, stream.ptr, sp["shards"], n * spitch, spitch, n, d_present, d_corrupt, I, SEED + 1)
        ctx.dev_inject_faults(stream.ptr, I, sp["shards"], spitch, d_corrupt)
        if pipe:  # the timed receiver: rbc_dev_receive_step, then the flush that completes the batch
            cur = ctx.rx_batch(I, sp["shards"], spitch, None, S, sp["branches"], sp["roots"], d_present, rb["valid"],
                               rb["leaves_r"], *vpo(rb), rb["digests"], rb["status"])
            ctx.dev_receive_step(stream.ptr, cur, None)
            ctx.dev_receive_step(stream.ptr, None, cur)
        else:
            ctx.dev_verify(stream.ptr, I, sp["shards"], spitch, None, S, sp["branches"], sp["roots"], d_present,
                           rb["valid"], rb["leaves_r"])
            ctx.dev_interpolate(stream.ptr, I, sp["shards"], spitch, None, S, rb["valid"], rb["leaves_r"], 1,
                                sp["roots"], *vpo(rb), rb["digests"], rb["status"])
        return sp, rb

    # the timed batch's gathered records are checked before its buffers are reused
    checks = check_results(args, synth, acs, rdz, world, first, I, total, slots, n, f, k, B, vpitch, last, timed,
                           d_gather, gather)
    pset, prb = poisoned_receive()
    poisoned = check_batch(args, ca, dev, stream, I, n, k, B, S, spitch, vpitch, opitch, d_values, pset, prb, d_count)
    checks = fold_guard(args, synth, rdz, first, I, total, n, f, k, B, vpitch, checks, timed, poisoned)

    def second_form_leg():
        """The same pipelined step in the other value form: the row view (the
        k data rows of the shard set, no join) beside a joined `value`, or
        the joined value (k*S contiguous bytes per instance, as rbc/rbc.go:88
        returns it) beside a row-view `value`: a shorter second timed run."""
        join2 = not args.join
        if join2:
            if need["pipelined"] + 2 * I * opitch > plan["budget_bytes"]:
                return {"skipped": "the joined values do not fit the HBM plan"}
            for rb in rxb:
                rb["out"] = mb(I * opitch)
        form.update(join=join2, start=100000)
        stream.sync()
        rstream.sync()
        steps_j = max(20, args.steps // 3)
        for t in range(3):
            pstep(form["start"] + t)
        barrier()
        t1 = time.perf_counter()
        for t in range(steps_j):
            pstep(form["start"] + 3 + t, ev_sets[t])
        barrier()
        el = time.perf_counter() - t1
        x_j, cur_j = pending.popitem()
        ctx.dev_receive_step(rstream.ptr, None, cur_j)
        rstream.sync()
        res = check_batch(args, ca, dev, stream, I, n, k, B, S, spitch, vpitch, opitch, d_values, sets[x_j % nsets],
                          rxb[x_j % nrx], d_count, join=join2)
        sm = spans(ev_sets[:steps_j], args.faults_on, pverify)
        return {"value": round(total * n * S * steps_j / el / 1e9, 3), "unit": "GB/s", "steps": steps_j,
                "ms_per_step": round(el * 1000.0 / steps_j, 4),
                "decoded_ok": int((res["status"] == 0).sum()), "values_ok": res["mism"] == 0,
                "stage_ms": {kk: round(v, 4) for kk, v in sm.items()},
                "value_form": "joined (k*S contiguous bytes per instance, assembled on the device)" if join2
                else "row view (the k data rows of the shard set, no join)",
                "note": "secondary run after the guard, same pipelined schedule; `value` is the "
                        + ("row view" if join2 else "joined form")}

    second = None
    if pipe and world == 1 and not args.no_second_form:
        wd.enter("second value-form leg", 300)
        second = second_form_leg()

    wd.enter("report", 1200)
    rep = report(args, ctx, I, n, k, d, S, present_h, corrupt_h, stage_ms, iso, elapsed_max)
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(args, host)
        cpu["gpu_over_cpu"] = round(value / cpu["value"], 2)
        for ph in ("encode_commit", "verify_decode"):
            rep["phases"][ph]["cpu_gbs"] = cpu["phases"][ph]
            rep["phases"][ph]["gpu_over_cpu"] = round(rep["phases"][ph]["gpu_gbs"] / cpu["phases"][ph], 1)
    pcie = None
    if not args.no_pcie:
        # host feeding is the scaling risk -- every rank runs one
        # epoch from pinned NUMA-local host memory at once (barrier-bracketed),
        # after the device-resident timing
        wd.enter("host-fed epoch", 600)
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import host_bench
        hi = args.host_instances or min(I, max(1, (2 * GiB) // B))
        sub = max(1, min(hi, int(400e6 // (n * S))))
        h = host_bench.epoch(ca, n, f, B, instances=hi, sub=sub, device=dev, seed=SEED + 7 + rank,
                             barrier=rdz.barrier)
        me["host_fed"] = {kk: h[kk] for kk in ("GBps", "seconds", "instances", "pcie_GBps", "ok")}
        me["host_fed"]["fused_GBps"] = h["fused"]["GBps"]
        per = rdz.allgather(h)
        pcie = host_fed_aggregate(per, n, S)
        fused = host_fed_aggregate([dict(x["fused"], instances=x["instances"]) for x in per], n, S)
        pcie["fused"] = {kk: fused[kk] for kk in ("aggregate_GBps", "per_rank_GBps", "slowest_rank", "min_over_max",
                                                  "ok")}
        pcie["fused"]["path"] = per[0]["fused"]["path"]
        kept = host_fed_aggregate([dict(x["kept"], instances=x["instances"]) for x in per], n, S)
        pcie["kept"] = {kk: kept[kk] for kk in ("aggregate_GBps", "per_rank_GBps", "slowest_rank", "min_over_max",
                                                "ok")}
        pcie["kept"]["path"] = per[0]["kept"]["path"]
        me["host_fed"]["kept_GBps"] = h["kept"]["GBps"]
        pcie.update({
                "unit": "GB/s of committed shard bytes (N*S per instance), host memory in and out",
                "path": "one epoch per rank through the C ABI from pinned host memory, all ranks at once: "
                        "rbc_shard_commit (values in; shards, roots, branches out) || "
                        "rbc_validate_packed_leaves of every received ECHO (N-f per instance, 10% of instances "
                        "with one corrupted ECHO; only the received rows cross PCIe) -> "
                        "rbc_interpolate_batch_verified of the valid ECHOs reusing their leaves (values out)",
                "aggregate_note": "sum of the ranks' instances x N x S / the slowest rank's epoch seconds"})
    batcher = None
    if rank == 0 and world == 1 and args.config == "c2" and not args.no_batcher:
        wd.enter("batcher sweep", 600)
        batcher = batcher_sweep(cpu)
    ranks, skew = rank_timing(rdz, me, elapsed, args.steps, stage_ms)
    line = {
        **head,
        **rep, **checks, "cpu_baseline": cpu, "pcie_inclusive": pcie, "ranks": ranks, "rank_skew": skew,
        **({"value_row_view": second} if args.join else {"value_joined": second}), "batcher": batcher,
    }
    ok = all(checks[c] for c in ("values_ok", "oracle_sample_ok", "gather_ok")) and checks["decoded_ok"] == total
    if pcie is not None:  # every rank's host-fed verdicts, values and roots
        ok = ok and pcie["ok"]
    if batcher and "skipped" not in batcher:  # the drop-in path's own checks (verdicts, values, rows, roots)
        ok = ok and batcher["failures"] == 0 and batcher["epoch"]["failures"] == 0 and batcher["rc"] == 0
    if second and "value" in second:  # the second leg's last batch passes the same value check
        ok = ok and second["values_ok"] and second["decoded_ok"] == I
    wd.leave()
    if not ok:
        print(json.dumps({"error": "correctness check failed", **checks, "library": line["library"]}),
              file=sys.stderr, flush=True)
        rdz.close()
        return 3
    if rank == 0:
        print(json.dumps(line), file=out, flush=True)
    rdz.barrier()
    rdz.close()
    return 0


DUMP_ELEMS = {"value": 6 << 20, "shards": 4 << 20, "valid": 2 << 20, "branches": 1 << 20}  # float32 each: < 64 MB


def dump_outputs(path, I, n, k, d, B, S, spitch, opitch, join, commit, cur_set, cur, prev):
    """--dump-outputs: what the last timed step left on the device, as
    float32 .npy files of byte values (status: the int32 codes).  roots,
    digests and status hold every instance; the large arrays a seeded sample
    whose indices are written beside them, the same from run to run:
      commit_roots [I,32], commit_branches [instances,N,depth,32],
      commit_shards [rows,S] (rows of commit_shards_index: instance, shard)
                       -- the step's commit (batch t)
      receive_valid [instances,N], receive_value [instances,B]
                       -- its ECHO verdicts and decoded values (batch t-1)
      receive_digests [I,32], receive_status [I]
                       -- its root recheck and digest (batch t-2)
    Under the serial schedule all three are the one batch of the step."""
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(SEED + 3)
    dd = max(d, 1)

    def pick(count, limit):
        return np.sort(rng.choice(count, size=max(1, min(count, limit)), replace=False))

    def save(name, a):
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))

    save("commit_roots", commit["roots"].download(I * 32).reshape(I, 32))
    save("receive_digests", prev["digests"].download(I * 32).reshape(I, 32))
    save("receive_status", prev["status"].download(I * 4).view(np.int32))
    ib = pick(I, DUMP_ELEMS["branches"] // (n * dd * 32))
    save("commit_branches_index", ib)
    save("commit_branches", np.stack([commit["branches"].download(n * dd * 32, int(i) * n * dd * 32)
                                      for i in ib]).reshape(len(ib), n, dd, 32))
    rows = pick(I * n, min(2048, DUMP_ELEMS["shards"] // S))
    save("commit_shards_index", np.stack([rows // n, rows % n], axis=1))
    save("commit_shards", np.stack([commit["shards"].download(S, int(r) * spitch) for r in rows]))
    iv = pick(I, DUMP_ELEMS["valid"] // n)
    save("receive_valid_index", iv)
    save("receive_valid", cur["valid"].download(I * n).reshape(I, n) if len(iv) == I
         else np.stack([cur["valid"].download(n, int(i) * n) for i in iv]))
    io = pick(I, DUMP_ELEMS["value"] // B)
    save("receive_value_index", io)
    if join:
        vals = [cur["out"].download(B, int(i) * opitch) for i in io]
    else:  # the row view: the k data rows of the batch's shard set, joined here and cut to the value's length
        vals = [cur_set["shards"].download(k * spitch, int(i) * n * spitch).reshape(k, spitch)[:, :S].reshape(-1)[:B]
                for i in io]
    save("receive_value", np.stack(vals))


def _run_key(name):
    """Profile file names carry their run, r<round><letters>: runs of a round
    are lettered a..z, then aa, ab, ... -- so r06ae is newer than r06h."""
    import re
    m = re.search(r"_r(\d+)([a-z]*)", name)
    return (int(m.group(1)), len(m.group(2)), m.group(2), name) if m else (-1, 0, "", name)


def host_fed_aggregate(per, n, S):
    """The ranks' host-fed epochs (tools/host_bench.epoch results, rank
    order) -> the job's figure: every rank's committed shard bytes over the
    slowest rank's epoch (the ranks start together behind a barrier), the
    per-rank rates, the spread, and whether every rank's checks passed."""
    el_max = max(x["seconds"] for x in per)
    rates = [x["GBps"] for x in per]
    return {"aggregate_GBps": round(sum(x["instances"] for x in per) * n * S / el_max / 1e9, 3),
            "ranks": len(per), "per_rank_GBps": rates,
            "slowest_rank": int(np.argmax([x["seconds"] for x in per])),
            "min_over_max": round(min(rates) / max(rates), 4) if max(rates) > 0 else None,
            "ok": all(x["ok"] for x in per), "rank0": per[0]}


FUSED_JOIN_MIN_S = 2048  # csrc/capi.cpp kFusedJoinMinS: the FFT decode joins rows of at least this many bytes
BATCHER_LEVELS = (1024, 8192, 32768, 88064)  # outstanding validates; 88,064 = one C2 epoch (1,024 x 86 ECHOs)
EPOCH_WINDOW = 64  # instances each of the 16 client threads keeps in flight: all 1,024 at once, one goroutine per instance (8: 15-19 GB/s and noisy, profiles/r06z)


def batcher_sweep(cpu):
    """The drop-in path the unchanged Go handlers use: validateMessage
    (rbc/rbc.go:92-95) once per ECHO through the batcher's validate lane
    (tools/batcher_bench validate-sweep: 16 client threads, each with a
    sliding window of outstanding requests, C2 messages from host memory,
    every verdict checked).  Host memory in, verdicts out: PCIe-inclusive,
    never `value`.  The host's own SHA-NI verify of the same message shape
    (cpu_baseline leg) sits beside it."""
    import subprocess
    exe = os.path.join(ROOT, "tools", "batcher_bench")
    if not os.path.exists(exe):
        return {"skipped": "tools/batcher_bench is not built"}
    r = subprocess.run([exe, "validate-sweep", "256", "16", "200"] + [str(x) for x in BATCHER_LEVELS],
                       capture_output=True, text=True, timeout=500)
    rows = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    sweep = [x for x in rows if x.get("phase") == "validate"]
    out = {"unit": "GB/s of ECHO shard bytes (S per message), host memory in, verdicts out",
           "sweep": [{kk: x[kk] for kk in ("outstanding", "window", "messages", "seconds", "GBps", "msg_per_s", "launches",
                                            "msgs_per_launch", "failed")} for x in sweep],
           "failures": next((x["failures"] for x in rows if x.get("phase") == "check"), None), "rc": r.returncode,
           "tool": "tools/batcher_bench validate-sweep (C2: N=128, f=42, 1 MiB values, S=23,832; 16 client threads)"}
    # the whole drop-in epoch: 1,024 shard + 88,064 validate + 1,024 interpolate
    # requests from 16 client threads at once, timed with the validate lane's leaves reused by
    # interpolate, again with the full rehash, and with the validated rows kept on the device
    # (rbc_batcher_set_keep); the tool checks every verdict, value, row and root
    r = subprocess.run([exe, "epoch", "1024", "16", str(EPOCH_WINDOW), "200"], capture_output=True, text=True,
                       timeout=300)
    rows = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    ep = {x["interpolate"].split()[0]: x for x in rows if x.get("phase") == "epoch"}
    chk = next((x for x in rows if x.get("phase") == "check"), {})
    out["epoch"] = {"unit": "GB/s of committed shard bytes (N*S per instance), host memory in and out",
                    "GBps": ep.get("verified", {}).get("GBps"), "GBps_full_rehash": ep.get("full", {}).get("GBps"),
                    # ABI 7: the same calls with rbc_batcher_set_keep (the ECHO rows cross PCIe once)
                    "GBps_kept": ep.get("kept", {}).get("GBps"),
                    "keep": next(({kk: v for kk, v in x.items() if kk != "phase"} for x in rows
                                  if x.get("phase") == "keep"), None),
                    "seconds": ep.get("verified", {}).get("seconds"), "requests": ep.get("verified", {}).get("requests"),
                    "launches": ep.get("verified", {}).get("launches"), "window_per_thread": EPOCH_WINDOW,
                    "failures": chk.get("failures"), "verified_equals_full": chk.get("verified_equals_full"),
                    "rc": r.returncode,
                    "tool": "tools/batcher_bench epoch (C2, 1,024 instances: shard + 86 validateMessage + interpolate "
                            "each, 10% with one corrupted ECHO, 16 client threads)"}
    if cpu and cpu.get("validate"):
        out["host_sha_ni"] = cpu["validate"]
        best = max((x["GBps"] for x in sweep), default=0)
        out["gpu_over_host_at_epoch"] = round(sweep[-1]["GBps"] / cpu["validate"]["GBps"], 2) if sweep else None
        out["best_GBps"] = best
    return out


def rank_timing(rdz, me, elapsed, steps, stage_ms):
    """Every rank's record (device, bus, NUMA node, RCCL ranks) with its own
    timed wall time, ms per step and stage spans, gathered to all ranks, and
    the skew between the slowest and the fastest rank: a slow or mis-placed
    rank of a multi-GPU run shows by name, not only in the max."""
    me = dict(me, elapsed_s=round(elapsed, 6), ms_per_step=round(elapsed * 1000.0 / steps, 4),
              stage_ms={kk: round(v, 4) for kk, v in stage_ms.items()})
    ranks = rdz.allgather(me)
    el = [r["elapsed_s"] for r in ranks]
    skew = {"elapsed_min_s": min(el), "elapsed_max_s": max(el), "slowest_rank": ranks[int(np.argmax(el))]["rank"],
            "fastest_rank": ranks[int(np.argmin(el))]["rank"],
            "max_over_min": round(max(el) / min(el), 4) if min(el) > 0 else None}
    return ranks, skew


def spans(ev_sets, faults_on, pverify=False):
    """Average event spans (ms) per stage over the given steps (faults_on None:
    the serial schedule); each span is taken on the stream its kernels run on
    (under the pipeline it also holds the other stream's concurrent work)."""
    pairs = {"enc": ("t0", "enc"), "leaf": ("enc", "leaf"), "tree": ("leaf", "tree")}
    if faults_on is None:
        pairs.update(fault=("tree", "pf"), verify=("pf", "hashed"), interp=("hashed", "rend"),
                     gather=("rend", "gather"))
    else:
        # verify = compaction + the row-hashing launch + (C4) the shared-path verify; verify_rows and
        # verify_path are the two launches alone (rbc_rx_marks hash_begin / rows_hashed, ABI 4)
        pairs.update(fault=("r0", "rf") if faults_on == "receiver" else ("tree", "pf"), verify=("rf", "hashed"),
                     verify_rows=("hb", "rh"), verify_path=("rh", "hashed"),
                     check=("hashed", "dbeg"), decode=("dbeg", "ddone"), interp=("hashed", "rend"),
                     gather=("rend", "gather"))
        if pverify:  # the verify runs on P after the commit; R's hashing launch is prev's regen rows alone
            pairs.update(verify=("pf", "pv"), regen_rows=("hb", "rh"))
            del pairs["verify_rows"], pairs["verify_path"]
    return {nm: sum(ev[a].elapsed_ms(ev[b]) for ev in ev_sets) / len(ev_sets) for nm, (a, b) in pairs.items()}


def decode_bytes(n, k, S, present, corrupt):
    """Algorithmic HBM bytes of interpolate's decode kernels for one batch:
    missing-data GF reads the k used rows and writes the m_d missing data rows
    (nothing when m_d = 0); the FFT re-encode reads the k data rows and, per
    parity position, writes a missing one or reads a valid-but-unused one for
    the compare (the m_d used parity rows are skipped); prepare reads the
    valid mask and writes the m_d x k decode matrix and N class bytes."""
    valid = present.astype(bool).copy()
    bad = corrupt >= 0
    valid[np.flatnonzero(bad), corrupt[bad]] = False
    md = (k - valid[:, :k].sum(axis=1)).astype(np.int64)
    gf = int(np.where(md > 0, (k + md) * S, 0).sum())
    fft = int(((k + (n - k - md)) * S).sum())
    return gf + fft + int(len(md) * 2 * n + (md * k).sum())


def report(args, ctx, I, n, k, d, S, present_h, corrupt_h, stage_ms, iso, elapsed_max):
    """roofline (dominant kernel), roofline_encode / roofline_decode (north_star:
    encode / decode against the HBM peak), sha256_chip, commit_only /
    receive_only (BASELINE configs[1] / [2] stages alone), phases."""
    bps = (S + 9 + 63) // 64  # compressions per shard
    R = int(present_h.sum())  # received ECHO shards
    regen = int(I * n - R + (corrupt_h >= 0).sum())
    enc_kernel = "rs_fft_kernel<encode>" if ctx.codec == "fft" else "gf_rows_kernel<encode>"
    pipe = "decode" in stage_ms
    path = ctx.verify_form(S) == "shared_path"  # rbc_ctx_verify_form: C4's leaves + merkle_path_kernel
    kern = {  # name: (stage, algorithmic HBM bytes per launch, SHA-256 compressions per launch)
        enc_kernel: ("enc", I * (k * S + n * S), 0),
        "sha_rows_kernel<leaves>": ("leaf", I * (n * S + n * 32), I * n * bps),
    }
    # the received ECHO rows (R) are read once; a walk also reads each row's d branch entries and the
    # instance's root and writes its valid byte; the shared-path verify reads the leaves and branches
    # of the received rows, the roots and present masks, and writes valid for every row
    path_bytes = R * (32 * d + 32) + I * (32 + 2 * n)
    if pipe and "regen_rows" in stage_ms:  # verify on the proposer's stream; R hashes the regen rows alone
        if path:
            kern["verify: sha_rows_kernel<leaves> + merkle_path_kernel<4>"] = ("verify", R * (S + 32) + path_bytes,
                                                                              R * bps)
        else:
            kern["sha_rows_kernel<verify>"] = ("verify", R * (S + 32 * d + 32 + 1) + I * 32, R * (bps + 2 * d))
        kern["sha_rx_kernel<regen>"] = ("regen_rows", regen * (S + 32), regen * bps)
    elif pipe:  # the receive step's row-hashing launch: ECHO rows of t + the regenerated rows of t-1
        if path:
            kern["sha_rx_kernel<leaves+regen>"] = ("verify_rows", (R + regen) * (S + 32), (R + regen) * bps)
            kern["merkle_path_kernel<4>"] = ("verify_path", path_bytes, 0)
        else:
            kern["sha_rx_kernel<verify+regen>"] = ("verify_rows", R * (S + 32 * d + 32 + 1) + I * 32 + regen * (S + 32),
                                                   R * (bps + 2 * d) + regen * bps)
    elif path:  # serial: rbc_dev_verify = leaves of the received rows, then merkle_path_kernel
        kern["verify: sha_rows_kernel<leaves> + merkle_path_kernel<4>"] = ("verify", R * (S + 32) + path_bytes, R * bps)
    else:
        kern["sha_rows_kernel<verify>"] = ("verify", R * (S + 32 * d + 32 + 1) + I * 32, R * (bps + 2 * d))
    if pipe:
        # + the joined value the FFT re-encode writes from the data rows it loads (k*S per instance), for
        # rows of >= FUSED_JOIN_MIN_S bytes; shorter rows are joined by join_kernel on the aux stream
        kern["decode: prepare + gf_regen_kernel + rs_fft_kernel<decode>"] = (
            "decode", decode_bytes(n, k, S, present_h, corrupt_h) + (I * k * S if args.join and S >= FUSED_JOIN_MIN_S
                                                                     else 0), 0)
    pm, pmc_path = {}, None
    want_form = "joined" if args.join else "row view"
    cands = []
    for cand in sorted((x for x in os.listdir(os.path.join(ROOT, "profiles")) if x.startswith("pmc_traffic_r")),
                       key=_run_key, reverse=True):
        try:
            c = json.load(open(os.path.join(ROOT, "profiles", cand)))
        except (OSError, ValueError):
            continue
        if c.get("config") == args.config and c.get("instances", 1024) == I:
            # rank: the timed value form stated in the file, then the other form stated (the SHA and
            # encode kernels are the same in both), then a file from before the form was recorded
            form = c.get("value_form")
            cands.append((0 if form == want_form else (1 if form else 2), cand, c))
    if cands:  # newest first within a rank (the names sort by round)
        _, cand, pm = min(cands, key=lambda x: x[0])
        pmc_path = os.path.join("profiles", cand)
    # the loaded clock per kernel, each kernel alone (serial schedule; tools/clock_summary.py)
    clk, clk_path = {}, None
    for cand in sorted((x for x in os.listdir(os.path.join(ROOT, "profiles")) if x.startswith("valu_clock_r")),
                       key=_run_key, reverse=True):
        try:
            c = json.load(open(os.path.join(ROOT, "profiles", cand)))
        except (OSError, ValueError):
            continue
        if c.get("config") == args.config and c.get("instances", 1024) == I:
            clk, clk_path = c, os.path.join("profiles", cand)
            break
    clock_ghz = clk.get("clock_ghz_weighted")
    mix_path = os.path.join("profiles", "isa_mix_r05.json")
    try:
        mix = json.load(open(os.path.join(ROOT, mix_path)))["kernels"]
    except (OSError, ValueError, KeyError):
        mix = {}
    lg = max(d, 1)

    def cpi(role):
        """SIMD clk per wave64 VALU instruction of a kernel role: SHA-256 kernels at the probe's
        dependency-limited rate at 4 waves per SIMD (issue_priced uses their static mix instead),
        every other kernel at its static ISA mix priced per opcode (tools/isa_mix.py)."""
        sym = {"rs_fft_kernel<encode>": f"rs_fft_kernel<{lg}, {k}, {n}, 0>",
               "rs_fft_kernel<decode>": f"rs_fft_kernel<{lg}, {k}, {n}, 1>",
               "sha_rows_kernel<leaves>": "sha_rows_kernel<false>", "sha_rows_kernel<verify>": "sha_rows_kernel<true>",
               "sha_rx_kernel<verify+regen>": "sha_rx_kernel", "sha_rx_kernel<leaves+regen>": "sha_rx_kernel"}.get(
                   role, role)
        m = mix.get(sym)
        if m is None:
            return None, None
        sha = sym.startswith(("sha_", "merkle", "digest"))
        return m["clk_per_instr"], (SHA_CHAIN_CLK_PER_INSTR if sha else m["clk_per_instr"])

    def priced(instr, role, ms):
        c_issue, c_chain = cpi(role)
        if c_issue is None or not clock_ghz:
            return None
        per_simd_ms = lambda c: instr * c / 1024 / (clock_ghz * 1e6)  # noqa: E731
        return {"issue_priced_ms": round(per_simd_ms(c_issue), 4), "chain_priced_ms": round(per_simd_ms(c_chain), 4),
                "issue_frac": round(per_simd_ms(c_issue) / ms, 4), "chain_frac": round(per_simd_ms(c_chain) / ms, 4)}

    def roofline(name, span=None):
        stage, nbytes, ncomp = kern[name]
        ms = stage_ms[stage]
        ach = nbytes / (ms / 1e3) / 1e9
        r = {"bound": "hbm", "kernel": name, "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
             "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None, "algorithmic_bytes_per_launch": int(nbytes),
             "avg_ms": round(ms, 4), "span": span or f"HIP events around the launch on its stream ({stage})"}
        pk = pm.get("kernels", {}).get(name)
        if pk and name.startswith("decode") and pm.get("value_form") != ("joined" if args.join else "row view"):
            pk = None  # the decode writes the joined value in one form and not the other: other traffic
        if pk:
            r["traffic"], r["traffic_source"] = pk["hbm_bytes_per_launch"], pmc_path
        if ncomp:
            cps = ncomp / (ms / 1e3)
            r["bound_note"] = ("SHA-256 is integer-VALU bound: HBM frac is not this kernel's roof (see valu and "
                               "isolated); under the pipeline avg_ms also holds the other stream's kernels")
            r["valu"] = {"achieved": round(cps / 1e9, 3), "peak": round(SHA_PEAK_CPS / 1e9, 2),
                         "unit": "G compressions/s", "frac": round(cps / SHA_PEAK_CPS, 4),
                         "attainable_probe": round(SHA_PROBE_CPS / 1e9, 2),
                         "frac_of_attainable": round(cps / SHA_PROBE_CPS, 4),
                         "model": "4 clk alignbit/add3/perm, 2 clk bitop3/add/shift per wave64 instr; 4484 SIMD "
                                  "clk per wave-compression @2.4 GHz nominal (the chip runs ~2.1 GHz under load)"}
        pr = priced(pk["SQ_INSTS_VALU"], name, ms) if pk and pk.get("SQ_INSTS_VALU") else None
        if pr:
            # the launch's wave64 VALU instructions (PMC) priced per opcode from the probe, over the
            # SIMD time of its live span at the loaded clock (SQ_ACTIVE_INST_VALU only counts
            # instructions on gfx950, so no counter gives busy cycles: tools/clock_summary.py)
            r.setdefault("valu", {})["priced"] = {
                "valu_instr_per_launch": pk["SQ_INSTS_VALU"], "clock_ghz": clock_ghz, **pr,
                "sources": [pmc_path, clk_path, mix_path],
                "note": "issue_priced: static ISA mix x per-opcode issue cost at 4 waves/SIMD (probe); "
                        "chain_priced: SHA-256 kernels at the probe's 6131 SIMD clk per wave-compression "
                        "(dependency-limited, 4 waves/SIMD). Under the pipeline the span also issues the other "
                        "stream's instructions"}
        if iso and iso.get(stage) and not name.startswith("sha_rx"):  # sha_rx runs only under the pipeline
            ms_i = iso[stage]
            r["isolated"] = {"avg_ms": round(ms_i, 4), "achieved": round(nbytes / ms_i / 1e6, 1),
                             "frac": round(nbytes / ms_i / 1e6 / HBM_PEAK_GBS, 4),
                             "note": "same kernel and batch alone on the chip (serial steps before the warmup)"}
            if ncomp:
                r["isolated"]["valu_frac_of_attainable"] = round(ncomp / (ms_i / 1e3) / SHA_PROBE_CPS, 4)
        return r

    dom = max((x for x in kern if not x.startswith("decode")), key=lambda x: stage_ms[kern[x][0]])
    out = {"stage_ms": {kk: round(v, 4) for kk, v in stage_ms.items()}, "roofline": roofline(dom),
           "roofline_encode": roofline(enc_kernel)}
    out["roofline_decode"] = roofline(
        "decode: prepare + gf_regen_kernel + rs_fft_kernel<decode>",
        "receive step's decode_begin -> decoded marks (rbc_rx_marks) on the receiver stream") if pipe else None
    # the receive step's two hashing launches, each over its own span (hash_begin -> rows_hashed ->
    # hashed marks): the row hashing, and at C4 the shared-path verify
    rx = [x for x in kern if kern[x][0] == "verify_rows"]
    sv = [x for x in kern if kern[x][0] == "verify"]  # serial schedule: rbc_dev_verify's launch(es)
    out["roofline_verify"] = roofline(rx[0], "receive step's hash_begin -> rows_hashed marks (rbc_rx_marks)") \
        if rx else (roofline(sv[0]) if sv else None)
    out["roofline_verify_path"] = roofline(
        "merkle_path_kernel<4>", "receive step's rows_hashed -> hashed marks (rbc_rx_marks)") \
        if "merkle_path_kernel<4>" in kern else None
    # the whole step's VALU issue, measured: every data-path kernel's wave64 VALU instructions per
    # launch (PMC, one launch each per step) at the loaded clock, against the chip's SIMD cycles
    util = ("fill_random", "count_mismatch", "poison_rows", "inject_faults", "__amd", "[grid")
    if pm.get("kernels") and clock_ghz:
        vk = {kk: v["SQ_INSTS_VALU"] for kk, v in pm["kernels"].items()
              if v.get("SQ_INSTS_VALU") and not any(u in kk for u in util) and not kk.startswith("decode:")}
        if vk:
            tot = sum(vk.values())
            step_ms = elapsed_max / args.steps * 1e3
            parts = {kk: priced(v, kk, step_ms) for kk, v in vk.items()}
            unpriced = sorted(kk for kk, v in parts.items() if v is None)
            out_valu = {"valu_instr_per_step": int(tot), "clock_ghz": clock_ghz, "kernels": len(vk),
                        "issue_priced_ms": round(sum(v["issue_priced_ms"] for v in parts.values() if v), 4),
                        "chain_priced_ms": round(sum(v["chain_priced_ms"] for v in parts.values() if v), 4),
                        "unpriced_kernels": unpriced, "sources": [pmc_path, clk_path, mix_path],
                        "per_kernel": {kk: v for kk, v in parts.items() if v},
                        "note": "every data-path kernel's wave64 VALU instructions per launch (PMC, one launch "
                                "each per step) priced in SIMD time at the loaded clock over 1024 SIMDs. "
                                "issue_priced: each kernel's static ISA mix at the probe's per-opcode issue cost "
                                "(v_perm / v_alignbit / v_add3 ~4.3-4.8 clk, v_bitop3 / v_xor / v_add / shifts "
                                "~2.4-2.8 clk at 4 waves per SIMD) -- the step if every SIMD issued back to back; "
                                "chain_priced: the SHA-256 kernels at the probe's measured dependency-limited "
                                "throughput instead (6131 clk per wave-compression at 4 waves per SIMD)"}
            out_valu["issue_frac_of_step"] = round(out_valu["issue_priced_ms"] / step_ms, 4)
            out_valu["chain_frac_of_step"] = round(out_valu["chain_priced_ms"] / step_ms, 4)
        else:
            out_valu = None
    else:
        out_valu = None
    step_comp = I * n * bps + R * (bps + 2 * d) + regen * bps
    step_cps = step_comp / (elapsed_max / args.steps)
    out["sha256_chip"] = {"compressions_per_step": int(step_comp), "achieved": round(step_cps / 1e9, 2),
                          "unit": "G compressions/s per GPU", "attainable_probe": round(SHA_PROBE_CPS / 1e9, 2),
                          "frac_of_attainable": round(step_cps / SHA_PROBE_CPS, 3),
                          "note": "leaves (all N rows) + ECHO verify (received rows + branch walk) + interpolate's "
                                  "regenerated rows, per ms_per_step"}
    out["valu_step"] = out_valu
    src = iso if iso is not None else (stage_ms if not pipe else None)
    for key, stages, note in (("commit_only", ("enc", "leaf", "tree"), "RS encode + Merkle build alone "
                               "(BASELINE configs[1]'s stages): encode + leaf hashing + tree spans of serial steps"),
                              ("receive_only", ("verify", "interp"), "ECHO-side Merkle branch verify + RS "
                               "reconstruct / re-encode / root recheck alone (BASELINE configs[2]'s stages): verify "
                               "+ interpolate spans of serial steps")):
        ms = sum(src[s] for s in stages) if src else None
        out[key] = {"GBps": round(I * n * S / ms / 1e6, 2), "ms_per_batch": round(ms, 4),
                    "unit": "GB/s of committed shard bytes (N*S per instance), per rank", "note": note} if ms else None
    enc_ms = stage_ms["enc"] + stage_ms["leaf"] + stage_ms["tree"]
    dec_ms = stage_ms["verify"] + stage_ms["interp"]
    out["phases"] = {"encode_commit": {"gpu_gbs": round(I * n * S / enc_ms / 1e6, 2), "bytes": "N*S per instance"},
                     "verify_decode": {"gpu_gbs": round(I * k * S / dec_ms / 1e6, 2), "bytes": "k*S per instance"}}
    return out


def check_batch(args, ca, dev, stream, I, n, k, B, S, spitch, vpitch, opitch, d_values, sp, rb, d_count, join=None):
    """One received batch on the device: statuses, and every decoded value
    against its input (the joined value, or the row view's k data rows)."""
    stream.sync()
    status = rb["status"].download(I * 4).view(np.int32).copy()
    if args.join if join is None else join:
        ca.rbc.count_mismatch(dev, stream.ptr, rb["out"], opitch, d_values, vpitch, I, B, d_count)
    else:  # the row view: the k data rows of the shard set are the value
        ca.rbc.count_mismatch_rows(dev, stream.ptr, sp["shards"], n * spitch, spitch, k, S, d_values, vpitch, B, I,
                                   d_count)
    stream.sync()
    return {"status": status, "mism": int(d_count.download(4).view(np.uint32)[0]),
            "roots": sp["roots"].download(I * 32).reshape(I, 32),
            "digests": rb["digests"].download(I * 32).reshape(I, 32)}


def check_results(args, synth, acs, rdz, world, first, I, total, slots, n, f, k, B, vpitch, last, timed, d_gather,
                  gather):
    """After the timed loop, the last timed batch: every instance decoded,
    every decoded value equals its input, the gathered records of every rank
    are what that rank holds, and sampled roots / digests equal the C
    oracle's (checker only: nothing here is timed or shipped)."""
    status, roots, digests = timed["status"], timed["roots"], timed["digests"]
    gather_ok = True
    if gather:
        mine = acs.pack_records(roots, digests, slots, status)
        everyone = rdz.allgather_bytes(mine.tobytes())
        g = d_gather.download().reshape(world, slots, 64)
        gather_ok = all(np.array_equal(g[r], np.frombuffer(everyone[r], np.uint8).reshape(slots, 64))
                        for r in range(world))
        gather_ok = rdz.all(gather_ok and [o["instance"] for o in acs.assemble_output_set(g, total, world)]
                            == list(range(total)))
    return {"gather_ok": gather_ok}


def oracle_samples(args, synth, first, I, total, n, f, k, B, vpitch, batches):
    """Evenly spaced global ids, each checked by its owner: the root and the
    digest of every given batch against the C restatement."""
    ok, checked = True, 0
    if args.oracle_samples <= 0:
        return ok, checked
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import rbc_ref
    for g_id in sorted(set(np.linspace(0, total - 1, min(args.oracle_samples, total)).astype(int).tolist())):
        if first <= g_id < first + I:
            i = g_id - first
            _, root, _, leaves = rbc_ref.encode_commit(n, f, synth.row(SEED, g_id, vpitch, B))
            dig = rbc_ref.sha256(np.ascontiguousarray(leaves[:k]).tobytes())
            for b in batches:
                ok = ok and bytes(b["roots"][i]) == root and bytes(b["digests"][i]) == dig and b["status"][i] == 0
            checked += 1
    return ok, checked


def fold_guard(args, synth, rdz, first, I, total, n, f, k, B, vpitch, checks, timed, poisoned):
    """decoded_ok / values_ok / oracle_sample_ok hold for BOTH the last timed
    batch and the poisoned receive (an instance counts as decoded only if it
    decoded in both); each batch's own figures are kept under `guard`."""
    both_ok = (timed["status"] == 0) & (poisoned["status"] == 0)
    sample_ok, checked = oracle_samples(args, synth, first, I, total, n, f, k, B, vpitch, (timed, poisoned))
    out = {"decoded_ok": rdz.sum(int(both_ok.sum())),
           "values_ok": rdz.all(timed["mism"] == 0 and poisoned["mism"] == 0),
           "value_mismatch_chunks": rdz.sum(timed["mism"] + poisoned["mism"]),
           "gather_ok": checks["gather_ok"],
           "oracle_sample_ok": rdz.all(sample_ok), "oracle_samples_checked": rdz.sum(checked)}
    out["guard"] = {
        "timed_batch": {"decoded": rdz.sum(int((timed["status"] == 0).sum())),
                        "value_mismatch_chunks": rdz.sum(timed["mism"])},
        "poisoned_batch": {"decoded": rdz.sum(int((poisoned["status"] == 0).sum())),
                           "value_mismatch_chunks": rdz.sum(poisoned["mism"]),
                           "note": "a fresh commit whose absent and corrupted rows were overwritten with seeded "
                                   "garbage (rbc_dev_poison_rows) before the receive path ran on it"}}
    return out


def cpu_baseline(args, host):
    """The C restatement (oracle/librbc_ref.so: AVX2 split-nibble GF +
    SHA-NI) running the same per-instance pipeline on this box's host cores,
    on bounded samples: the bench config (~6 GB of shard output) and, more
    briefly, every other config."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import rbc_ref

    threads = host["usable_cores"]
    feats = rbc_ref.lib().rbcref_cpu_features()

    def run(cfg, target_bytes, nthreads):
        n, f, B, _, _ = CONFIGS[cfg]
        k = n - 2 * f
        S = (B + k - 1) // k
        count = max(nthreads, int(target_bytes // (n * S)))
        rng = np.random.default_rng(7)
        values = rng.integers(0, 256, size=(min(count, 64), B), dtype=np.uint8)  # instance i uses values[i % 64]
        present = np.zeros((count, n), dtype=np.uint8)
        corrupt = np.full(count, -1, dtype=np.int32)
        for i in range(count):
            pres = rng.permutation(n)[: n - f]
            present[i, pres] = 1
            if rng.random() < 0.10:
                corrupt[i] = int(rng.choice(pres))
        secs, st, es, ds = rbc_ref.pipeline(n, f, count, B, nthreads, values, present, corrupt, phases=True)
        return {"value": round(count * n * S / secs / 1e9, 3), "unit": "GB/s",
                "phases": {"encode_commit": round(count * n * S / (es / nthreads) / 1e9, 3),
                           "verify_decode": round(count * k * S / (ds / nthreads) / 1e9, 3)},
                "sample": f"{count} instances x {B} B (N={n} f={f}), {secs:.2f} s wall on {nthreads} threads",
                "status_sum": st}

    def validate_rate():
        """validateMessage of one C2 epoch's ECHOs (88,064 = 1,024 instances x
        86) on the host's cores, SHA-NI where present: the per-message
        baseline of the batcher's validate lane (key `batcher`)."""
        n, f, B, _, _ = CONFIGS["c2"]
        rng = np.random.default_rng(11)
        com = [rbc_ref.encode_commit(n, f, rng.integers(0, 256, B, dtype=np.uint8)) for _ in range(32)]
        shards = np.stack([c[0] for c in com])
        branches = np.stack([c[2] for c in com])
        roots = np.stack([np.frombuffer(c[1], np.uint8) for c in com])
        m = np.arange(88064)
        inst, j = (m // (n - f)) % len(com), m % (n - f)
        # three passes over the epoch (each ~0.1 s on 16 cores), the median reported: one short pass
        # moved with the shared host's load by ~12 %
        runs = [rbc_ref.verify_many(n, shards, branches, roots, inst, j, threads) for _ in range(3)]
        secs = sorted(r[0] for r in runs)[1]
        ok = np.logical_and.reduce([r[1] for r in runs])
        S = shards.shape[2]
        return {"GBps": round(len(m) * S / secs / 1e9, 3), "msg_per_s": round(len(m) / secs), "cores": threads,
                "all_valid": bool(ok.all()), "kind": "port",
                "runs_GBps": [round(len(m) * S / r[0] / 1e9, 3) for r in runs],
                "sample": f"{len(m)} C2 ECHO messages (S={S}) from {len(com)} committed values, median of 3 "
                          f"passes, {secs:.3f} s"}

    main_cfg = args.config
    res, single = run(main_cfg, 6e9, threads), run(main_cfg, 6e9 / 16, 1)
    per_config, per_config_1 = {}, {}
    for cfg in [c.strip() for c in args.cpu_configs.split(",") if c.strip() in CONFIGS]:
        per_config[cfg] = res if cfg == main_cfg else run(cfg, 1.5e9, threads)
        per_config_1[cfg] = single if cfg == main_cfg else run(cfg, 1.5e9 / 16, 1)  # 1 core too
    return {"value": res["value"], "unit": "GB/s", "cores": threads, "kind": "port",
            "sample": res["sample"] + "; same per-instance pipeline as the GPU step (verified leaves reused)",
            "phases": res["phases"],
            "single_core": {"value": single["value"], "unit": "GB/s", "cores": 1, "phases": single["phases"],
                            "sample": single["sample"]},
            "per_config": {c: {"value": r["value"], "phases": r["phases"], "sample": r["sample"],
                               "single_core": {"value": per_config_1[c]["value"], "phases": per_config_1[c]["phases"]}}
                           for c, r in per_config.items()},
            "validate": validate_rate() if main_cfg == "c2" else None,
            "host": host, "simd": ("avx2 " if feats & 1 else "") + ("sha-ni" if feats & 2 else ""),
            "status_sum": res["status_sum"] + single["status_sum"] + sum(r["status_sum"] for r in per_config.values())
            + sum(r["status_sum"] for c, r in per_config_1.items() if c != main_cfg)}


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
