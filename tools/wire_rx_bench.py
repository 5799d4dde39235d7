#!/usr/bin/env python3
"""One node's C2 epoch of received ECHOs, validated two ways in the same run.

N = 128, f = 42; 1,024 instances x 86 ECHOs of S = 23,832-byte shards arrive as
pb.Message bytes in a pinned ring (a pass-through gRPC codec's view).

  A  the parent's path: rbc_pb_decode_rbc + rbc_json_decode_val on 16 host
     threads into a pinned packed arena (tools/wire_rx_decode.cpp), then
     rbc_validate_packed_keep.
  B  rbc_wire_validate straight from the ring.
  K  the unmarshal kernel alone on a device-resident ring, from events, beside
     its byte floor (bytes read + written over the HBM rate DESIGN.md uses).

  C  today's composition to delivered values: rbc_wire_validate, the host
     reads the verdicts and groups the kept rows by instance, then
     rbc_interpolate_batch_kept.
  R  rbc_wire_receive: the same ring to the same values in one submission.

  H  the epoch's READYs on the host: 1,024 instances x 128 READYs of 65 bytes;
     16 threads run rbc_pb_decode_rbc + rbc_json_decode_ready, a per-sender
     dedupe and the thresholds per instance (tools/wire_rx_decode.cpp).
  Q  rbc_wire_quorum: the same ring to the same bitmap, counts and flags in
     one submission.

Every leg is a child process of its own under its own time limit; the parent
stops at the first one that fails.  Each leg runs --warmup (>= 2) epochs, then
--epochs (>= 5) timed ones, and reports the median and the min-max spread.  The
epoch is seeded, so the legs see the same bytes, and A's and B's verdicts must
be identical (a digest of them is compared), and so must C's and R's statuses
and value bytes.  About 1 % of the messages carry one corrupted shard
character, so both verdict values occur.  H and Q see one READY ring (every
member's READY for every instance, about 1 % with one root character replaced,
so that READY names another root), and their bitmaps, counts, flags and
per-message verdicts must be identical.

--codec json|binary (or both, comma-separated) chooses the payload codec the
epoch is encoded in and the context decodes (include/rbc_protocol.h,
RBC_HAS_WIRE_BINARY).  With both, every leg runs once per codec in the same
invocation, json first, on the same shards with the same messages corrupted;
the verdict and result digests must be identical across the codecs, and each
leg's binary run is called a win or a loss against its json run only where
their min-max ranges do not overlap.  Leg A is the JSON host decoder's.

  python tools/wire_rx_bench.py --legs A,B,K --out profiles/wire_rx/c2.json
  python tools/wire_rx_bench.py --legs C,R --out profiles/wire_rx/c2_receive.json
  python tools/wire_rx_bench.py --legs B,R,K --codec json,binary --out profiles/wire_rx/c2_binary.json
  python tools/wire_rx_bench.py --legs H,Q --out profiles/wire_rx/c2_ready.json
  python tools/wire_rx_bench.py --legs H,Q --n 256 --f 85 --instances 4096 --out profiles/wire_rx/c4_ready.json
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 8e12  # the roofline's HBM rate
THREADS = 16


NAMES = {"A": "A_parent_decode_then_validate_packed_keep", "B": "B_wire_validate", "K": "K_unmarshal_kernel",
         "C": "C_wire_validate_then_interpolate_kept", "R": "R_wire_receive",
         "H": "H_host_ready_decode_and_tally", "Q": "Q_wire_quorum"}
READY_LEGS = ("H", "Q")


def rup(x, a):
    return (x + a - 1) // a * a


def build_epoch(ca, ctx, a):
    """The epoch's messages in a pinned ring: offs, lens, idx, and the commitment geometry."""
    import numpy as np
    n, k, d = ctx.n, ctx.k, ctx.depth
    S = a.shard_len
    rng = np.random.default_rng(a.seed)
    distinct = min(a.distinct, a.instances)
    values = [rng.integers(0, 256, k * S, dtype=np.uint8) for _ in range(distinct)]
    c = ctx.shard_commit_batch(values)
    pitch = rup(S, 64)
    sh = np.zeros((distinct, n, pitch), np.uint8)
    sh[:, :, :S] = c["shards"][:, :, :S]
    out_pitch = rup(ctx.val_message_size(S, 0, 1), 16)
    dsh, dbr, drt = ca.DeviceBuffer(sh.nbytes), ca.DeviceBuffer(distinct * n * d * 32), ca.DeviceBuffer(distinct * 32)
    dout, dol = ca.DeviceBuffer(distinct * n * out_pitch), ca.DeviceBuffer(distinct * n * 4)
    dsh.upload(sh)
    dbr.upload(np.ascontiguousarray(c["branches"]).reshape(-1))
    drt.upload(np.ascontiguousarray(c["roots"]).reshape(-1))
    ctx.dev_marshal_val(None, distinct, 1, dsh, pitch, None, S, dbr, drt, dout, out_pitch, dol)
    ca.rbc.lib.rbc_device_sync(0)
    msgs = dout.download().reshape(distinct * n, out_pitch)
    mlen = int(dol.download().view(np.uint32)[0])
    for b in (dsh, dbr, drt, dout, dol):
        b.free()
    count = a.instances * a.echoes
    slot = rup(mlen, 16)
    ring = ca.pinned_empty(count * slot)
    r2 = ring.reshape(count, slot)
    idx = np.zeros(count, np.uint8)
    for i in range(a.instances):
        senders = np.sort(rng.permutation(n)[:a.echoes])
        idx[i * a.echoes:(i + 1) * a.echoes] = senders
        r2[i * a.echoes:(i + 1) * a.echoes] = msgs[(i % distinct) * n + senders, :slot]
    # ~1 % corrupted: one shard character replaced by another of the alphabet (binary: the first
    # shard byte that character encodes, one bit flipped): the same messages under either codec
    binary = a.codec == "binary"
    blk0 = mlen - 2 - S if binary else mlen - 5 - (S + 2) // 3 * 4  # the ECHO type field (and '"]}') behind the block
    for m in rng.permutation(count)[:max(count // 100, 1)]:
        ch = int(rng.integers(0, S // 3 * 4))
        if binary:
            r2[m, blk0 + ch * 3 // 4] ^= 1
        else:
            r2[m, blk0 + ch] = ord("A") if r2[m, blk0 + ch] != ord("A") else ord("B")
    offs = np.arange(count, dtype=np.uint64) * slot
    lens = np.full(count, mlen, np.uint32)
    inst = np.repeat(np.arange(a.instances, dtype=np.uint32), a.echoes)
    roots = np.ascontiguousarray(c["roots"])[np.arange(a.instances) % distinct]
    return {"ring": ring, "offs": offs, "lens": lens, "idx": idx, "count": count, "S": S, "mlen": mlen,
            "inst": inst, "roots": np.ascontiguousarray(roots), "instances": a.instances,
            "wire_bytes": int(count) * mlen, "shard_bytes": int(count) * S, "ring_bytes": int(ring.nbytes)}


def timed(fn, warmup, epochs):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(epochs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def stats(ts, nbytes):
    med = statistics.median(ts)
    return {"median_s": med, "min_s": min(ts), "max_s": max(ts), "epochs_s": ts,
            "median_GBps": nbytes / med / 1e9, "min_GBps": nbytes / max(ts) / 1e9, "max_GBps": nbytes / min(ts) / 1e9}


def digest(v):
    return hashlib.sha256(bytes(v)).hexdigest()


def leg_a(ca, ctx, e, a):
    import numpy as np
    assert a.codec == "json", "leg A is the JSON host decoder's path"
    so = os.path.join(ROOT, "tools", "libwire_rx_decode.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "libwire_rx_decode.so"], check=True)
    dec = ctypes.CDLL(so).wire_rx_decode_range
    dec.restype = ctypes.c_int
    dec.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_uint32,
                   ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 3
    count, S, d = e["count"], e["S"], ctx.depth
    assert ctx.n % 2 == 0  # no empty level-0 sibling: the flat branch is the device form
    pitch, bslot = rup(S, 64), max(d, 1) * 32
    arena = ca.pinned_empty(count * pitch)
    arena[:] = 0
    aoffs = np.arange(count, dtype=np.uint64) * pitch
    br, roots = ca.pinned_empty((count, bslot)), ca.pinned_empty((count, 32))
    slens, types = np.zeros(count, np.uint32), np.zeros(count, np.uint8)
    keep = ca.DeviceBuffer(arena.nbytes)
    out = {"ok": ca.pinned_empty(count), "leaves": ca.pinned_empty((count, 32))}
    bad = [0] * THREADS
    edges = [count * t // THREADS for t in range(THREADS + 1)]
    host_s = []

    def work(t):
        bad[t] = dec(e["ring"].ctypes.data, e["offs"].ctypes.data, e["lens"].ctypes.data, edges[t], edges[t + 1],
                     arena.ctypes.data, aoffs.ctypes.data, pitch, br.ctypes.data, bslot, roots.ctypes.data,
                     slens.ctypes.data, types.ctypes.data)

    def epoch():
        t0 = time.perf_counter()
        th = [threading.Thread(target=work, args=(t,)) for t in range(THREADS)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        host_s.append(time.perf_counter() - t0)
        assert sum(bad) == 0 and (slens == S).all()
        ctx.validate_packed_submit(arena, aoffs, slens, e["idx"], br, roots, leaves=True, out=out, keep=keep).wait()

    ts = timed(epoch, a.warmup, a.epochs)
    verdict = (out["ok"][:count] != 0).astype(np.uint8)
    r = stats(ts, e["shard_bytes"])
    r.update(host_decode_median_s=statistics.median(host_s[a.warmup:]), verdict_sha256=digest(verdict),
             valid=int(verdict.sum()), h2d_bytes=int(arena.nbytes))
    return r


def leg_b(ca, ctx, e, a):
    count, S = e["count"], e["S"]
    pitch = rup(S, 64)
    rx = ca.WireRx(ctx, count, e["ring"].nbytes, pitch)
    keep = ca.DeviceBuffer(count * pitch)
    got = {}

    def epoch():
        got.update(rx.validate(e["ring"], e["offs"], e["lens"], e["idx"], keep))

    ts = timed(epoch, a.warmup, a.epochs)
    assert (got["verdict"] != 2).all(), "a message of the project's own encoder fell back"
    r = stats(ts, e["shard_bytes"])
    r.update(verdict_sha256=digest(got["verdict"]), valid=int((got["verdict"] == 1).sum()),
             h2d_bytes=int(e["ring"].nbytes))
    rx.close()
    return r


def leg_k(ca, ctx, e, a):
    import numpy as np
    count, S, d = e["count"], e["S"], ctx.depth
    pitch, bslot = rup(S, 64), max(d, 1) * 32
    dring = ca.DeviceBuffer(e["ring"].nbytes)
    dring.upload(e["ring"])
    doffs, dlens, didx = ca.DeviceBuffer(count * 8), ca.DeviceBuffer(count * 4), ca.DeviceBuffer(count)
    doffs.upload(e["offs"])
    dlens.upload(e["lens"])
    didx.upload(e["idx"])
    rows, slens, br = ca.DeviceBuffer(count * pitch), ca.DeviceBuffer(count * 4), ca.DeviceBuffer(count * bslot)
    roots, types, status = ca.DeviceBuffer(count * 32), ca.DeviceBuffer(count), ca.DeviceBuffer(count * 4)
    st = ca.Stream()
    ms = []
    for it in range(a.warmup + a.epochs):
        e0, e1 = ca.Event(), ca.Event()
        e0.record(st)
        ctx.dev_unmarshal_val(st.ptr, count, dring, doffs, dlens, didx, rows, pitch, slens, br, roots, types, status)
        e1.record(st)
        st.sync()
        if it >= a.warmup:
            ms.append(e0.elapsed_ms(e1))
    assert not status.download().view(np.int32).any()
    read = count * (e["mlen"] + 13)                      # the message, offs, lens, idx
    written = count * (pitch + (d * 32) + 32 + 4 + 1 + 4)  # row up to round_up(S, 64), branch, root, S, type, status
    med = statistics.median(ms) / 1e3
    floor = (read + written) / HBM_BPS
    return {"median_s": med, "min_s": min(ms) / 1e3, "max_s": max(ms) / 1e3, "epochs_s": [m / 1e3 for m in ms],
            "bytes_read": read, "bytes_written": written, "floor_s": floor, "floor_over_median": floor / med,
            "achieved_TBps": (read + written) / med / 1e12}


def result_digest(status, values, used):
    """Statuses and the value bytes of the delivered instances."""
    import numpy as np
    h = hashlib.sha256(np.ascontiguousarray(status, np.int32).tobytes())
    for i in np.nonzero(np.asarray(status) == 0)[0]:
        h.update(values[i, :used].tobytes())
    return h.hexdigest()


def leg_c(ca, ctx, e, a):
    import numpy as np
    count, S, I, n, k = e["count"], e["S"], e["instances"], ctx.n, ctx.k
    pitch = rup(S, 64)
    rx = ca.WireRx(ctx, count, e["ring"].nbytes, pitch)
    keep = ca.DeviceBuffer(count * pitch)
    values = ca.pinned_empty((I, k * S))
    addr = np.uint64(keep.value) + np.arange(count, dtype=np.uint64) * np.uint64(pitch)
    inst, idx = e["inst"].astype(np.int64), e["idx"].astype(np.int64)
    got, res, group_s = {}, {}, []

    def epoch():
        got.update(rx.validate(e["ring"], e["offs"], e["lens"], e["idx"], keep))
        t0 = time.perf_counter()  # the host's turn: verdicts -> the [instances][n] table of kept rows
        use = (got["verdict"] == 1) & (got["shard_lens"] == S) & (got["roots"] == e["roots"][inst]).all(axis=1)
        rows = np.zeros((I, n), np.uint64)
        leaves = np.zeros((I, n, 32), np.uint8)
        rows[inst[use], idx[use]] = addr[use]
        leaves[inst[use], idx[use]] = got["leaves"][use]
        group_s.append(time.perf_counter() - t0)
        res.update(ctx.interpolate_kept_submit(rows, [S] * I, e["roots"], leaves=leaves, values_out=values).wait())

    ts = timed(epoch, a.warmup, a.epochs)
    r = stats(ts, e["shard_bytes"])
    r.update(result_sha256=result_digest(res["status"], res["values"], k * S), delivered=int((res["status"] == 0).sum()),
             proven=int((got["verdict"] == 1).sum()), host_grouping_median_s=statistics.median(group_s[a.warmup:]),
             h2d_bytes=int(e["ring"].nbytes))
    rx.close()
    return r


def leg_r(ca, ctx, e, a):
    count, S, I, k = e["count"], e["S"], e["instances"], ctx.k
    rcv = ca.WireReceiver(ctx, I, count, e["ring"].nbytes, rup(S, 64))
    values = ca.pinned_empty((I, k * S))
    got = {}

    def epoch():
        got.update(rcv.receive(e["ring"], e["offs"], e["lens"], e["inst"], e["idx"], e["roots"], [S] * I,
                               values_out=values))

    ts = timed(epoch, a.warmup, a.epochs)
    assert (got["verdict"] < 2).all(), "a message of the project's own encoder fell back"
    r = stats(ts, e["shard_bytes"])
    r.update(result_sha256=result_digest(got["status"], got["values"], k * S),
             delivered=int((got["status"] == 0).sum()), proven=int((got["verdict"] == 1).sum()),
             h2d_bytes=int(e["ring"].nbytes))
    rcv.close()
    return r


def build_ready_epoch(ca, ctx, a):
    """The epoch's READYs in a pinned ring, ordered by instance: every member's READY for every
    instance, ~1 % naming another root; and what the ECHO side knows (valid, status)."""
    import numpy as np
    from cleisthenes_amd import protocol
    n, f, I = ctx.n, a.f, a.instances
    rng = np.random.default_rng(a.seed)
    roots = rng.integers(0, 256, (I, 32), dtype=np.uint8)
    first = np.frombuffer(protocol.pb_encode(protocol.READY, protocol.json_encode_ready(roots[0].tobytes())), np.uint8)
    mlen, slot = len(first), rup(len(first), 16)
    count = I * n
    ring = ca.pinned_empty(count * slot)
    ring[:] = 0
    r2 = ring.reshape(I, n, slot)
    for i in range(I):
        r2[i, :, :mlen] = np.frombuffer(protocol.pb_encode(protocol.READY, protocol.json_encode_ready(roots[i].tobytes())),
                                        np.uint8)
    flat = ring.reshape(count, slot)
    root_at = bytes(first).index(b'":"') + 3  # the root's 44 base64 characters
    for m in rng.permutation(count)[:max(count // 100, 1)]:
        at = root_at + int(rng.integers(0, 40))
        flat[m, at] = ord("A") if flat[m, at] != ord("A") else ord("B")
    # the ECHO side: most instances have their N-f proven ECHOs and a value, some only N-2f, some too few
    ecount = rng.choice([n - f, n - f, n - f, n - 2 * f, n - 2 * f - 1], I)
    valid = np.zeros((I, n), np.uint8)
    for i in range(I):
        valid[i, rng.permutation(n)[:ecount[i]]] = 1
    status = np.where(ecount >= n - 2 * f, 0, -3).astype(np.int32)
    return {"ring": ring, "offs": np.arange(count, dtype=np.uint64) * slot, "lens": np.full(count, mlen, np.uint32),
            "inst": np.repeat(np.arange(I, dtype=np.uint32), n), "idx": np.tile(np.arange(n, dtype=np.uint8), I),
            "msg_first": np.arange(I + 1, dtype=np.uint32) * n, "roots": roots, "valid": valid, "status": status,
            "count": count, "instances": I, "mlen": mlen, "S": 0, "wire_bytes": count * mlen, "shard_bytes": 0,
            "ring_bytes": int(ring.nbytes), "self": 0}


def ready_digest(ready, verdict, ecounts, rcounts, flags):
    import numpy as np
    h = hashlib.sha256()
    for v, t in ((ready, np.uint8), (verdict, np.uint8), (ecounts, np.uint32), (rcounts, np.uint32), (flags, np.uint8)):
        h.update(np.ascontiguousarray(v, t).tobytes())
    return h.hexdigest()


def ready_result(ts, e, ready, verdict, ecounts, rcounts, flags):
    import numpy as np
    r = stats(ts, e["wire_bytes"])
    r.update(result_sha256=ready_digest(ready, verdict, ecounts, rcounts, flags), counted=int((verdict == 0).sum()),
             other_root=int((verdict == 2).sum()), fallback=int((verdict == 1).sum()),
             send_ready=int((np.asarray(flags) & 4 != 0).sum()), deliver=int((np.asarray(flags) & 8 != 0).sum()),
             messages_per_s_median=e["count"] / statistics.median(ts))
    return r


def leg_h(ca, ctx, e, a):
    import numpy as np
    so = os.path.join(ROOT, "tools", "libwire_rx_decode.so")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "libwire_rx_decode.so"], check=True)
    fn = ctypes.CDLL(so).wire_ready_host_range
    fn.restype = None
    fn.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 2 + [ctypes.c_void_p] + [ctypes.c_int] * 3 + \
        [ctypes.c_void_p] * 7
    I, n, count = e["instances"], ctx.n, e["count"]
    ready, verdict = np.zeros((I, n), np.uint8), np.zeros(count, np.uint8)
    ec, rc, fl = np.zeros(I, np.uint32), np.zeros(I, np.uint32), np.zeros(I, np.uint8)
    edges = [I * t // THREADS for t in range(THREADS + 1)]
    p = lambda x: x.ctypes.data  # noqa: E731

    def work(t):
        fn(p(e["ring"]), p(e["offs"]), p(e["lens"]), p(e["idx"]), p(e["msg_first"]), edges[t], edges[t + 1],
           p(e["roots"]), n, a.f, e["self"], p(e["valid"]), p(e["status"]), p(ready), p(verdict), p(ec), p(rc), p(fl))

    def epoch():
        ready[:] = 0
        th = [threading.Thread(target=work, args=(t,)) for t in range(THREADS)]
        for x in th:
            x.start()
        for x in th:
            x.join()

    ts = timed(epoch, a.warmup, a.epochs)
    return ready_result(ts, e, ready, verdict, ec, rc, fl)


def leg_q(ca, ctx, e, a):
    import numpy as np
    I, n = e["instances"], ctx.n
    wq = ca.WireQuorum(ctx, I, e["count"], e["ring"].nbytes)
    ready = np.zeros((I, n), np.uint8)
    got = {}

    def epoch():
        ready[:] = 0
        got.update(wq.quorum(ready, ring=e["ring"], offs=e["offs"], lens=e["lens"], inst=e["inst"], idx=e["idx"],
                             roots=e["roots"], valid=e["valid"], status=e["status"], self_id=e["self"]))

    ts = timed(epoch, a.warmup, a.epochs)
    r = ready_result(ts, e, ready, got["verdict"], got["echo_counts"], got["ready_counts"], got["flags"])
    r.update(h2d_bytes=int(e["ring"].nbytes))
    wq.close()
    return r


def child(a):
    import cleisthenes_amd as ca
    ctx = ca.Context(a.n, a.f)
    if a.codec != "json":  # before the epoch is built: the marshal kernel writes the codec's messages
        ctx.set_wire_codec(a.codec)
    e = build_ready_epoch(ca, ctx, a) if a.leg in READY_LEGS else build_epoch(ca, ctx, a)
    r = {"A": leg_a, "B": leg_b, "K": leg_k, "C": leg_c, "R": leg_r, "H": leg_h, "Q": leg_q}[a.leg](ca, ctx, e, a)
    r.update(leg=a.leg, count=e["count"], shard_len=e["S"], message_len=e["mlen"], wire_bytes=e["wire_bytes"],
             shard_bytes=e["shard_bytes"], ring_bytes=e["ring_bytes"], codec=a.codec, library=os.path.relpath(ca.rbc.library_path(), ROOT))
    print("WIRE_RX_LEG " + json.dumps(r), flush=True)


def run_leg(a, leg, codec):
    """One leg in a child process of its own, under its own time limit."""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--codec", codec] + \
        [x for k in ("n", "f", "instances", "echoes", "shard_len", "distinct", "warmup", "epochs", "seed")
         for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
    env = dict(os.environ, OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", str(THREADS)))
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout, env=env)
    except subprocess.TimeoutExpired:
        sys.exit(f"leg {leg} ({codec}): no result within {a.leg_timeout} s; stopping")
    line = [x for x in r.stdout.splitlines() if x.startswith("WIRE_RX_LEG ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"leg {leg} ({codec}) failed (exit {r.returncode}); stopping")
    res = json.loads(line[-1][len("WIRE_RX_LEG "):])
    print(f"leg {leg} ({codec}): median {res['median_s'] * 1e3:.3f} ms", file=sys.stderr, flush=True)
    return res


def both_codecs(a, want, codecs):
    """Every leg once per codec, the codecs alternating; binary against json by min-max range."""
    res = {"bench": "wire_rx", "geometry": {"n": a.n, "f": a.f, "instances": a.instances, "echoes": a.echoes,
                                            "shard_len": a.shard_len}, "threads": THREADS, "warmup": a.warmup,
           "epochs": a.epochs, "codecs": codecs}
    same = True
    for leg in want:
        runs = {c: run_leg(a, leg, c) for c in codecs}
        j, b = runs["json"], runs["binary"]
        cmp = {"binary_over_json_median": j["median_s"] / b["median_s"],
               "binary_vs_json": "win" if b["max_s"] < j["min_s"] else "loss" if b["min_s"] > j["max_s"] else "tie",
               "ring_bytes_binary_over_json": b["ring_bytes"] / j["ring_bytes"]}
        for key in ("verdict_sha256", "result_sha256"):
            if key in j:
                cmp[key + "_identical"] = j[key] == b[key]
                same = same and cmp[key + "_identical"]
        res[NAMES[leg] + "[binary vs json]"] = cmp
        for c in codecs:
            res[f"{NAMES[leg]}[{c}]"] = runs[c]
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)
    if not same:
        sys.exit("the two codecs gave different verdicts or results")


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, default=128)
    p.add_argument("--f", type=int, default=42)
    p.add_argument("--instances", type=int, default=1024)
    p.add_argument("--echoes", type=int, default=86)
    p.add_argument("--shard-len", type=int, default=23832)
    p.add_argument("--distinct", type=int, default=16, help="distinct proposals behind the epoch's instances")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--epochs", type=int, default=5)
    p.add_argument("--seed", type=int, default=20261019)
    p.add_argument("--leg-timeout", type=int, default=240, help="seconds per leg")
    p.add_argument("--out", default=None)
    p.add_argument("--legs", default="A,B,K", help="comma-separated legs to run, of A B K C R H Q")
    p.add_argument("--codec", default="json", help="payload codec: json, binary, or json,binary for both")
    p.add_argument("--leg", choices=list(NAMES), default=None, help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.warmup < 2 or a.epochs < 5:
        p.error("at least 2 warm-up and 5 timed epochs")
    codecs = [x for x in a.codec.split(",") if x]
    if not codecs or any(x not in ("json", "binary") for x in codecs) or len(set(codecs)) != len(codecs):
        p.error("--codec takes json, binary or json,binary")
    if a.leg:
        return child(a)
    want = [x for x in a.legs.split(",") if x]
    if not want or any(x not in NAMES for x in want):
        p.error("--legs takes a comma-separated list of " + " ".join(NAMES))
    if "A" in want and codecs != ["json"]:
        p.error("leg A is the JSON host decoder's path: run it with --codec json")
    if len(codecs) == 2:
        return both_codecs(a, want, codecs)
    legs = {leg: run_leg(a, leg, codecs[0]) for leg in want}
    res = {"bench": "wire_rx", "geometry": {"n": a.n, "f": a.f, "instances": a.instances, "echoes": a.echoes,
                                            "shard_len": a.shard_len}, "threads": THREADS, "warmup": a.warmup,
           "epochs": a.epochs}
    if codecs != ["json"]:
        res["codec"] = codecs[0]
    same = True
    if "A" in legs and "B" in legs:
        same = legs["A"]["verdict_sha256"] == legs["B"]["verdict_sha256"]
        res.update(verdicts_identical=same, B_over_A_median=legs["A"]["median_s"] / legs["B"]["median_s"])
    if "C" in legs and "R" in legs:
        c, r = legs["C"], legs["R"]
        res.update(results_identical=c["result_sha256"] == r["result_sha256"],
                   R_over_C_median=c["median_s"] / r["median_s"],
                   R_vs_C="win" if r["max_s"] < c["min_s"] else "loss" if r["min_s"] > c["max_s"] else "tie")
        same = same and res["results_identical"]
    if "H" in legs and "Q" in legs:
        h, q = legs["H"], legs["Q"]
        res.update(ready_results_identical=h["result_sha256"] == q["result_sha256"],
                   Q_over_H_median=h["median_s"] / q["median_s"],
                   Q_vs_H="win" if q["max_s"] < h["min_s"] else "loss" if q["min_s"] > h["max_s"] else "tie")
        res["geometry"].update(readies_per_instance=a.n, ready_messages=a.n * a.instances)
        same = same and res["ready_results_identical"]
    for leg in want:
        res[NAMES[leg]] = legs[leg]
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)
    if not same:
        sys.exit("two legs that must agree gave different results")


if __name__ == "__main__":
    main()
