"""ECHOs from wire bytes to delivered values in one call: rbc_dev_unmarshal_echo
(unmarshal_echo_kernel, csrc/wire.hip) and rbc_wire_receive
(csrc/wire_receive.cpp).

* Decode placement: the hostile corpus of tests/test_gpu_wire_rx.py, grouped
  into instances, shuffled, some messages against another root or another
  length; every status equals the oracle's (the documented five-step order over
  the host decoder), every decoded field sits at its slot, and no byte outside
  the slots of the messages sent changes.
* End to end: rbc_wire_receive equals rbc_wire_validate + host grouping +
  rbc_interpolate_batch_kept on the same ring, and the proposer's values.
* A Byzantine proposer (a commitment over a non-codeword): every ECHO proves,
  the status is RBC_ERR_ROOT_MISMATCH.
* A pageable ring gives what the pinned one gives.
* Every argument check rejects before any device work.

The canonicality test of the oracle: the host decoder accepts the bytes and its
fields re-encode to the same bytes -- except the last character in front of the
'=' of a padded base64 run, whose trailing bits the device decoder ignores as
the host decoder (and Go's) does (include/rbc_protocol.h, rbc_dev_unmarshal_val).
"""
import ctypes

import numpy as np
import pytest

from test_gpu_wire_rx import _corpus, _echo_ring, _runs, rup

pytestmark = pytest.mark.gpu

OK, FALLBACK, OTHER_ROOT, OTHER_LEN = 0, 1, 2, 3
RBC_OK, TOO_FEW, ROOT_MISMATCH, INVALID_ARG = 0, -3, -8, -10
CANARY = 0xC7
GUARD = 256


# ---------------------------------------------------------------------------
# the oracle: the five-step status order over the host decoder
# ---------------------------------------------------------------------------
def _vlen(v):
    n = 1
    while v >= 0x80:
        v >>= 7
        n += 1
    return n


def _msg_size(groups, br_len, mtype):
    """Bytes of the canonical message with `groups` base64 quanta of block (the format description)."""
    # {"RootHash":"<44>","Branch":"<b64>","Block":["<b64>"]}  or  ...,"Branch":null,...
    J = (13 + 44 + 12 + (br_len + 2) // 3 * 4 + 12 if br_len else 13 + 44 + 26) + 4 * groups + 3
    R = 1 + _vlen(J) + J + (2 if mtype else 0)
    return 1 + _vlen(R) + R


def _shape(m, idx, n, depth):
    """(S, type) a canonical message of len(m) bytes from leaf idx would have, else None."""
    if idx >= n:
        return None
    br_len = 32 * (depth - (1 if depth > 0 and (idx ^ 1) >= n else 0))
    for mtype in (0, 1):
        g = 1
        while _msg_size(g, br_len, mtype) <= len(m):
            if _msg_size(g, br_len, mtype) == len(m):
                end = len(m) - (2 if mtype else 0) - 3
                pad = (2 if m[end - 2] == 0x3D else 1) if m[end - 1] == 0x3D else 0
                return 3 * g - pad, mtype
            g += 1
    return None


def _host_fields(ca, protocol, orc, m, idx, n):
    """The host decoder's fields of a canonical message, else None."""
    try:
        t, payload = protocol.pb_decode(m)
        req = protocol.json_decode_val(payload)
    except ca.RBCError:
        return None
    blk = req["Block"][0]
    if t not in (protocol.VAL, protocol.ECHO) or not blk or orc.unflatten_branch(req["Branch"], idx, n) is None:
        return None
    again = protocol.pb_encode(t, protocol.json_encode_val(req["RootHash"], req["Branch"], blk))
    if len(again) != len(m):
        return None
    if again != m:
        free = set()  # the last character in front of a run's padding
        for b, e in _runs(again):
            npad = (e - b) - len(again[b:e].rstrip(b"="))
            if npad:
                free.add(e - npad - 1)
        if any(x != y and at not in free for at, (x, y) in enumerate(zip(again, m))):
            return None
    return {"type": t, "root": req["RootHash"], "branch": req["Branch"], "block": blk}


def _oracle(ca, protocol, orc, m, idx, n, depth, root, slen, pitch):
    """(status, host fields or None) of message m from leaf idx for an instance with (root, slen)."""
    sh = _shape(m, idx, n, depth)
    if sh is None or sh[0] > pitch:
        return FALLBACK, None
    if sh[0] != slen:
        return OTHER_LEN, None
    h = _host_fields(ca, protocol, orc, m, idx, n)
    if h is None or h["type"] != sh[1] or len(h["block"]) != sh[0]:
        return FALLBACK, None
    if h["root"] != root:
        return OTHER_ROOT, h
    return OK, h


def _pack(ca, msgs, pinned=True):
    """The messages at 16-byte offsets of one ring: ring, offs, lens."""
    offs = np.zeros(len(msgs), np.uint64)
    at = 0
    for i, m in enumerate(msgs):
        offs[i] = at
        at += rup(max(len(m), 1), 16)
    ring = ca.pinned_empty(at) if pinned else np.empty(at, np.uint8)
    ring[:] = 0
    for m, o in zip(msgs, offs):
        ring[int(o):int(o) + len(m)] = np.frombuffer(m, np.uint8)
    return ring, offs, np.array([len(m) for m in msgs], np.uint32)


# ---------------------------------------------------------------------------
# 1. decode placement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,f", [(4, 1), (5, 1), (7, 2), (16, 5)])
def test_unmarshal_echo_places_every_message_and_follows_the_status_order(gpu, n, f):
    import rbc_oracle as orc
    from cleisthenes_amd import protocol
    ca = gpu
    ctx = ca.Context(n, f)
    try:
        d = ctx.depth
        bslot, pitch = max(d, 1) * 32, 192
        rng = np.random.default_rng(1000 + n)
        corpus = _corpus(protocol, n, d)
        # every message gets an instance setting (root, shard length): its own fields, another
        # instance's root, or another length; messages with one setting share instances, one per leaf
        insts, open_by_key, plan = [], {}, []
        for m, idx, _ in corpus:
            h = _host_fields(ca, protocol, orc, m, idx, n)
            root = h["root"] if h else rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
            slen = len(h["block"]) if h else (5, 64, 100)[int(rng.integers(0, 3))]
            roll = int(rng.integers(0, 10))
            if roll == 0:
                root = insts[int(rng.integers(0, len(insts)))][0] if insts else bytes(32)
            elif roll == 1:
                slen = slen + 1 if slen < pitch else slen - 1
            for i in open_by_key.setdefault((root, slen), []):
                if idx not in insts[i][2]:
                    break
            else:
                i = len(insts)
                insts.append((root, slen, set()))
                open_by_key[(root, slen)].append(i)
            insts[i][2].add(idx)
            plan.append((m, idx, i))
        count = len(insts)
        assert any(len(s) > 1 for _, _, s in insts)  # instances holding several messages
        order = rng.permutation(len(plan))
        plan = [plan[q] for q in order]
        msgs = len(plan)
        ring, offs, lens = _pack(ca, [m for m, _, _ in plan])
        idx = np.array([ix for _, ix, _ in plan], np.uint8)
        inst = np.array([i for _, _, i in plan], np.uint32)
        roots = np.frombuffer(b"".join(r for r, _, _ in insts), np.uint8)
        slens = np.array([s for _, s, _ in insts], np.uint32)

        def dev(a):
            a = np.ascontiguousarray(a)
            b = ca.DeviceBuffer(max(a.nbytes, 16))
            b.upload(a.view(np.uint8).reshape(-1))
            return b
        dring, doffs, dlens, dinst, didx, droots, dslens = (dev(a) for a in (ring, offs, lens, inst, idx, roots, slens))
        sizes = {"shards": count * n * pitch, "branches": count * n * bslot, "present": count * n,
                 "status": msgs * 4, "types": msgs}
        out = {}
        for name, size in sizes.items():
            out[name] = ca.DeviceBuffer(size + GUARD)
            out[name].upload(np.full(size + GUARD, CANARY, np.uint8))
        ctx.dev_unmarshal_echo(None, count, msgs, dring, doffs, dlens, dinst, didx, droots, dslens, 0, out["shards"],
                               pitch, out["branches"], out["present"], out["status"], out["types"])
        ca.rbc.lib.rbc_device_sync(0)
        got = {}
        for name, size in sizes.items():
            raw = out[name].download()
            assert (raw[size:] == CANARY).all(), f"guard after {name} overwritten"
            got[name] = raw[:size]
        status = got["status"].view(np.int32)
        shards = got["shards"].reshape(count * n, pitch)
        branches = got["branches"].reshape(count * n, bslot)
        present = got["present"]
        sent = np.zeros(count * n, bool)
        for q, (m, ix, i) in enumerate(plan):
            r = i * n + ix
            assert not sent[r]
            sent[r] = True
            want, h = _oracle(ca, protocol, orc, m, ix, n, d, insts[i][0], insts[i][1], pitch)
            assert status[q] == want, (q, int(status[q]), want, ix, i, len(m))
            if want == OK:
                blk = h["block"]
                S = len(blk)
                assert present[r] == 1 and got["types"][q] == h["type"], q
                assert bytes(shards[r, :S]) == blk, q
                assert not shards[r, S:rup(S, 64)].any(), q
                assert (shards[r, rup(S, 64):] == CANARY).all(), q
                levels = orc.unflatten_branch(h["branch"], ix, n)
                assert bytes(branches[r]) == b"".join(lv if lv else bytes(32) for lv in levels), q
            else:
                assert present[r] == CANARY, q
            if want == OTHER_LEN:  # the slot is fully intact
                assert (shards[r] == CANARY).all() and (branches[r] == CANARY).all(), q
        # no byte outside the slots of the messages sent changed
        assert (shards[~sent] == CANARY).all() and (branches[~sent] == CANARY).all()
        assert (present[~sent] == CANARY).all()
        assert set(np.unique(status)) == {OK, FALLBACK, OTHER_ROOT, OTHER_LEN}
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# 2. end to end
# ---------------------------------------------------------------------------
_EPOCHS = {}


def _epoch(ca, ctx, n, f):
    """A seeded epoch of six instances (built once per geometry): the ECHOs, what was done to them and
    the oracle's verdicts."""
    if (n, f) in _EPOCHS:
        return _EPOCHS[(n, f)]
    import rbc_oracle as orc
    from cleisthenes_amd import protocol
    k, d = ctx.k, ctx.depth
    rng = np.random.default_rng(100 * n + f)
    # ragged lengths; instances 3 and 4 share S, so that an ECHO of one is "another root" for the other
    vlens = [k * 40 + 1, k * 96, k * 150 - 2, k * 64 - 1, k * 64 - 1, k * 200 - 3]
    values = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in vlens]
    c, slens, echo = _echo_ring(ca, ctx, values)
    count = len(values)
    assert len(set(int(s) for s in slens)) >= 4 and slens[3] == slens[4]
    senders = []
    for i in range(count):
        keep = n - f if i < 4 else (k if i == 4 else k - 1)  # 4: exactly k rows, 5: fewer than k
        senders.append(sorted(int(j) for j in rng.permutation(n)[:keep]))
    absent = [[j for j in range(n) if j not in senders[i]] for i in range(count)]
    plan = {(i, j): echo[i * n + j] for i in range(count) for j in senders[i]}  # (inst, idx) -> bytes
    # instance 0: one in-alphabet corruption of a shard character
    j = senders[0][1]
    m = plan[(0, j)]
    at = _runs(m)[2][0] + 7
    plan[(0, j)] = m[:at] + (b"A" if m[at:at + 1] != b"A" else b"B") + m[at + 1:]
    # instance 0 too, at a leaf nobody sent from: an ECHO of another length (instance 1's)
    plan[(0, absent[0][0])] = echo[1 * n + absent[0][0]]
    # instance 1: one whitespace-padded message
    j = senders[1][0]
    t, payload = protocol.pb_decode(plan[(1, j)])
    plan[(1, j)] = protocol.pb_encode(t, payload.replace(b":", b": ", 1))
    # instance 2: one message under a wrong idx (a leaf nobody sent from, with a branch of the same length)
    j = next(s for s in senders[2] if (s ^ 1) < n)
    j2 = next(a for a in absent[2] if (a ^ 1) < n)
    plan[(2, j2)] = plan.pop((2, j))
    # instance 3: one ECHO carrying instance 4's root (same length)
    j = senders[3][2]
    plan[(3, j)] = echo[4 * n + j]
    keys = list(plan)
    keys = [keys[q] for q in rng.permutation(len(keys))]  # interleaved across the instances
    msgs = [plan[key] for key in keys]
    inst = np.array([i for i, _ in keys], np.uint32)
    idx = np.array([j for _, j in keys], np.uint8)
    pitch = rup(int(slens.max()), 64)
    verdict = np.zeros(len(msgs), np.uint8)
    for q, m in enumerate(msgs):
        i, j = int(inst[q]), int(idx[q])
        st, h = _oracle(ca, protocol, orc, m, j, n, d, bytes(c["roots"][i]), int(slens[i]), pitch)
        if st == OK:
            levels = orc.unflatten_branch(h["branch"], j, n)
            verdict[q] = orc.merkle_verify(n, h["block"], h["root"], levels, j)
        else:
            verdict[q] = {FALLBACK: 2, OTHER_ROOT: 0, OTHER_LEN: 3}[st]
    e = {"values": values, "roots": np.ascontiguousarray(c["roots"]), "slens": slens, "msgs": msgs, "inst": inst,
         "idx": idx, "pitch": pitch, "verdict": verdict, "count": count}
    _EPOCHS[(n, f)] = e
    return e


def _composition(ca, ctx, e, ring, offs, lens):
    """Today's path: rbc_wire_validate, host grouping, rbc_interpolate_batch_kept."""
    n, count, pitch = ctx.n, e["count"], e["pitch"]
    rx = ca.WireRx(ctx, len(offs), ring.nbytes, pitch)
    try:
        keep = ca.DeviceBuffer(len(offs) * pitch)
        got = rx.validate(ring, offs, lens, e["idx"], keep)
        rows = np.zeros((count, n), np.uint64)
        leaves = np.zeros((count, n, 32), np.uint8)
        for q in range(len(offs)):
            i, j = int(e["inst"][q]), int(e["idx"][q])
            if (got["verdict"][q] == 1 and bytes(got["roots"][q]) == bytes(e["roots"][i])
                    and got["shard_lens"][q] == e["slens"][i]):
                rows[i, j] = keep.value + q * pitch
                leaves[i, j] = got["leaves"][q]
        res = ctx.interpolate_kept_submit(rows, [int(s) for s in e["slens"]], e["roots"], leaves=leaves).wait()
        return rows != 0, res
    finally:
        rx.close()


@pytest.mark.parametrize("n,f", [(4, 1), (7, 2), (16, 5), (37, 12), (128, 42)])
def test_wire_receive_equals_the_composition_and_the_oracle(gpu, n, f):
    ca = gpu
    ctx = ca.Context(n, f)
    rcv = None
    try:
        k = ctx.k
        e = _epoch(ca, ctx, n, f)
        count, slens = e["count"], e["slens"]
        ring, offs, lens = _pack(ca, e["msgs"])
        rcv = ca.WireReceiver(ctx, count, len(offs), ring.nbytes, e["pitch"])
        got = rcv.receive(ring, offs, lens, e["inst"], e["idx"], e["roots"], slens)
        assert np.array_equal(got["verdict"], e["verdict"]), np.nonzero(got["verdict"] != e["verdict"])[0][:10]
        assert set(np.unique(got["verdict"])) == {0, 1, 2, 3}
        assert (got["types"][got["verdict"] == 1] == 1).all()  # ECHO
        proven = np.zeros((count, n), np.uint8)
        proven[e["inst"][e["verdict"] == 1], e["idx"][e["verdict"] == 1]] = 1
        assert np.array_equal(got["valid"], proven)
        assert proven[4].sum() == k and proven[5].sum() < k
        want_valid, want = _composition(ca, ctx, e, ring, offs, lens)
        assert np.array_equal(got["valid"] != 0, want_valid)
        assert np.array_equal(got["status"], want["status"])
        assert set(got["status"]) == {RBC_OK, TOO_FEW} and got["status"][4] == RBC_OK and got["status"][5] == TOO_FEW
        for i, v in enumerate(e["values"]):
            used = k * int(slens[i])
            assert not got["values"][i, used:].any(), i  # zeros up to value_pitch
            if got["status"][i] != RBC_OK:
                continue  # values and digests are defined where the status is RBC_OK
            assert np.array_equal(got["values"][i, :used], want["values"][i, :used]), i
            assert np.array_equal(got["digests"][i], want["digests"][i]), i
            assert got["values"][i, :used].tobytes() == v + bytes(used - len(v)), i  # the value plus the Split pad
    finally:
        if rcv is not None:
            rcv.close()
        ctx.close()


# ---------------------------------------------------------------------------
# 3. a Byzantine proposer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,f", [(7, 2), (16, 5)])
def test_wire_receive_reports_a_commitment_over_a_non_codeword(gpu, ref, n, f):
    import rbc_oracle as orc
    from cleisthenes_amd import protocol
    ca = gpu
    ctx = ca.Context(n, f)
    rcv = None
    try:
        k = ctx.k
        rng = np.random.default_rng(7 * n)
        values = [rng.integers(0, 256, k * 70 - 1, dtype=np.uint8) for _ in range(2)]
        S = 70
        pitch = rup(S, 64)
        msgs, inst, idx, roots = [], [], [], []
        shards = np.zeros((2, n, pitch), np.uint8)
        for i, v in enumerate(values):
            sh, _, _, _ = ref.encode_commit(n, f, v)
            if i == 0:
                sh[k + 1, 3] ^= 0x20  # one parity row altered before the Merkle build: not a codeword
            mt = orc.merkle_tree([bytes(r) for r in sh])
            roots.append(mt[1])
            shards[i, :, :S] = sh
            for j in range(n):
                br = orc.flat_branch(orc.merkle_branch(mt, j))
                msgs.append(protocol.pb_encode(protocol.ECHO, protocol.json_encode_val(mt[1], br, bytes(sh[j]))))
                inst.append(i)
                idx.append(j)
        roots = np.frombuffer(b"".join(roots), np.uint8).reshape(2, 32)
        ring, offs, lens = _pack(ca, msgs)
        rcv = ca.WireReceiver(ctx, 2, len(msgs), ring.nbytes, pitch)
        got = rcv.receive(ring, offs, lens, inst, idx, roots, [S, S])
        assert (got["verdict"] == 1).all() and (got["valid"] == 1).all()  # every ECHO proves
        assert list(got["status"]) == [ROOT_MISMATCH, RBC_OK]
        assert got["values"][1, :k * S].tobytes() == values[1].tobytes() + b"\0"
        same = ctx.interpolate_batch(shards, [S, S], np.ones((2, n), np.uint8), roots)
        assert list(same["status"]) == [ROOT_MISMATCH, RBC_OK]
        assert np.array_equal(same["digests"][1], got["digests"][1])
    finally:
        if rcv is not None:
            rcv.close()
        ctx.close()


# ---------------------------------------------------------------------------
# 4. a pageable ring
# ---------------------------------------------------------------------------
def test_wire_receive_from_a_pageable_ring_gives_the_same(gpu):
    ca = gpu
    n, f = 16, 5
    ctx = ca.Context(n, f)
    rcv = None
    try:
        e = _epoch(ca, ctx, n, f)
        ring, offs, lens = _pack(ca, e["msgs"])
        rcv = ca.WireReceiver(ctx, e["count"], len(offs), ring.nbytes, e["pitch"])
        pinned = rcv.receive(ring, offs, lens, e["inst"], e["idx"], e["roots"], e["slens"])
        pageable = rcv.receive(np.array(ring), offs, lens, e["inst"], e["idx"], e["roots"], e["slens"])
        ok = pinned["status"] == RBC_OK
        assert ok.any() and not ok.all()
        for name in ("verdict", "types", "valid", "status"):
            assert np.array_equal(pageable[name], pinned[name]), name
        for name in ("values", "digests"):
            assert np.array_equal(pageable[name][ok], pinned[name][ok]), name
        assert np.array_equal(pinned["verdict"], e["verdict"])
    finally:
        if rcv is not None:
            rcv.close()
        ctx.close()


# ---------------------------------------------------------------------------
# 5. rejections
# ---------------------------------------------------------------------------
def test_wire_receive_rejects_bad_arguments_and_then_still_works(gpu):
    from cleisthenes_amd import _lib, protocol
    ca = gpu
    lib = _lib.lib
    n, f = 4, 1
    ctx = ca.Context(n, f)
    rcv = None
    try:
        k = ctx.k
        rng = np.random.default_rng(44)
        values = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in (k * 50, k * 33 - 1)]
        msgs, inst, idx, roots, slens = [], [], [], [], []
        for i, v in enumerate(values):
            s = ctx.shard(v)
            roots.append(s["root"])
            slens.append(len(s["shards"][0]))
            for j in range(n - f):
                msgs.append(protocol.pb_encode(protocol.ECHO, protocol.json_encode_val(s["root"], s["branches"][j],
                                                                                      bytes(s["shards"][j]))))
                inst.append(i)
                idx.append(j)
        count, nm, pitch = 2, len(msgs), 64
        ring, offs, lens = _pack(ca, msgs)
        rcv = ca.WireReceiver(ctx, count, nm, ring.nbytes, pitch)
        vp = k * max(slens)
        good = {"count": count, "msgs": nm, "ring": ring, "ring_bytes": ring.nbytes, "offs": offs, "lens": lens,
                "inst": np.array(inst, np.uint32), "idx": np.array(idx, np.uint8),
                "roots": np.frombuffer(b"".join(roots), np.uint8).copy(),
                "shard_lens": np.array(slens, np.uint64), "value_pitch": vp}
        outs = {"verdict": np.zeros(nm, np.uint8), "types": np.zeros(nm, np.uint8),
                "valid": np.zeros((count, n), np.uint8), "values": np.zeros((count, vp), np.uint8),
                "digests": np.zeros((count, 32), np.uint8), "status": np.zeros(count, np.int32)}
        ticket = ctypes.c_uint64(0)

        def call(**change):
            a = dict(good, **{name: None for name in ("verdict", "types", "valid", "values", "digests", "status")})
            a.update({name: outs[name] for name in outs})
            a["ticket"] = ctypes.byref(ticket)
            a.update(change)
            p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            sl = a["shard_lens"]
            return lib.rbc_wire_receive(rcv._p, a["count"], a["msgs"], p(a["ring"]), a["ring_bytes"], p(a["offs"]),
                                        p(a["lens"]), p(a["inst"]), p(a["idx"]), p(a["roots"]),
                                        None if sl is None else sl.ctypes.data_as(_lib.szp), p(a["verdict"]),
                                        p(a["types"]), p(a["valid"]), p(a["values"]), a["value_pitch"],
                                        p(a["digests"]), None if a["status"] is None
                                        else a["status"].ctypes.data_as(_lib.i32p), a["ticket"])

        def rejected(**change):
            for o in outs.values():
                o.view(np.uint8)[...] = 0x5B
            ticket.value = 77
            assert call(**change) == INVALID_ARG, change.keys()
            assert ticket.value == 77 and all((o.view(np.uint8) == 0x5B).all() for o in outs.values()), change.keys()

        for name in ("ring", "offs", "lens", "inst", "idx", "roots", "shard_lens", "verdict", "valid", "values",
                     "status", "ticket"):
            rejected(**{name: None})
        more = lambda a, x: np.append(a, np.array([x], a.dtype))  # noqa: E731
        rejected(count=count + 1, roots=np.zeros(96, np.uint8), shard_lens=np.array(slens + [5], np.uint64))
        rejected(msgs=nm + 1, offs=more(offs, 0), lens=more(lens, lens[0]), inst=more(good["inst"], 1),
                 idx=more(good["idx"], n - 1))                                            # msgs > max_msgs
        rejected(ring_bytes=ring.nbytes + 16)                                             # ring_bytes > max_ring_bytes
        rejected(offs=offs + np.array([0, 8] + [0] * (nm - 2), np.uint64))                # misaligned offs
        rejected(ring_bytes=int(offs[-1]) + 16)                                           # a message past ring_bytes
        rejected(inst=np.array([0, 0, 2] + inst[3:], np.uint32))                          # inst >= count
        rejected(count=1)                                                                 # instance 1 of one
        rejected(idx=np.array([0, n, 2] + idx[3:], np.uint8))                             # idx >= n
        rejected(idx=np.array([0, 1, 1] + idx[3:], np.uint8))                             # (0, 1) twice
        rejected(shard_lens=np.array([slens[0], 0], np.uint64))
        rejected(shard_lens=np.array([pitch + 1, slens[1]], np.uint64))
        rejected(value_pitch=vp - 1)                                                      # < k * Smax
        # a good call afterwards returns the right values
        got = rcv.receive(ring, offs, lens, inst, idx, good["roots"], slens)
        assert (got["verdict"] == 1).all() and (got["status"] == RBC_OK).all()
        assert np.array_equal(got["valid"], np.array([[1] * (n - f) + [0] * f] * count, np.uint8))
        for i, v in enumerate(values):
            used = k * slens[i]
            assert got["values"][i, :used].tobytes() == v + bytes(used - len(v)), i
            assert not got["values"][i, used:].any()
    finally:
        if rcv is not None:
            rcv.close()
        ctx.close()
