"""READYs from wire bytes to per-instance quorums: rbc_dev_unmarshal_ready
(unmarshal_ready_kernel), rbc_dev_quorum (quorum_kernel, both csrc/wire.hip) and
rbc_wire_quorum (csrc/wire_ready.cpp).

* Mutation corpus: every single-byte mutation of a canonical READY, its
  truncations and extensions and the 31- / 33-byte roots, about 17 k messages in
  one launch; the statuses equal the Python oracle's (pb_decode / json_decode and
  the re-encode canonicality test), `ready` holds exactly the OK slots on top of
  its 0 / 1 pattern, and the guard behind msg_status is intact.
* Accumulation and duplicates over three calls.
* The quorum kernel against a numpy restatement: random rows and the boundary
  rows of every threshold, with and without `self`.
* Lock step with OracleNode: ECHOs through rbc_wire_receive, READYs through
  rbc_wire_quorum, in three batches.
* rbc_wire_quorum end to end: pinned and pageable rings, a re-tally without
  messages, and equality with the rbc_dev_* pair.

The geometries: (4, 1), (7, 2) and (128, 42) with three instances, (256, 85) with
two -- n = 128 and 256 are where the tally takes more than one wave-wide step
(two and four), and idx reaches 255, the last value its byte holds.

The canonicality test of the oracle: the host decoder accepts the bytes as a
READY and its root re-encodes to the same bytes -- except the last character in
front of the '=', whose trailing bits the device decoder ignores as the host
decoder (and Go's) does (include/rbc_protocol.h).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, FALLBACK, OTHER_ROOT = 0, 1, 2
Q_ECHO, Q_AMPLIFY, Q_SEND_READY, Q_DELIVER = 1, 2, 4, 8
RBC_OK, TOO_FEW, ROOT_MISMATCH = 0, -3, -8
GUARD_BYTE, GUARD = 0xA5, 256
GEOMETRIES = [(4, 1, 3), (7, 2, 3), (128, 42, 3), (256, 85, 2)]


def rup(x, a):
    return (x + a - 1) // a * a


# ---------------------------------------------------------------------------
# the oracle: pb_decode / json_decode and the re-encode canonicality test
# ---------------------------------------------------------------------------
def _ready_msg(po, root):
    return po.pb_encode(po.READY, po.json_encode_ready(root))


def _host(po, m):
    """(accepted root or None, canonical) of message m under the host decoder."""
    dec = po.pb_decode(m)
    req = po.json_decode(dec[1]) if dec is not None and dec[0] == po.READY else None
    if req is None or len(req["root"]) != 32:
        return None, False
    again = _ready_msg(po, req["root"])
    if len(again) != len(m):
        return req["root"], False
    free = again.rindex(b"=") - 1  # the last character in front of the padding
    return req["root"], all(x == y or at == free for at, (x, y) in enumerate(zip(again, m)))


_CORPUS = {}


def _corpus():
    """The messages (built and judged once): [(bytes, root or None, canonical)], and the roots A, B."""
    if _CORPUS:
        return _CORPUS["msgs"], _CORPUS["A"], _CORPUS["B"]
    import rbc_protocol_oracle as po
    rng = np.random.default_rng(20261019)
    A, B = (rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(2))
    canon = _ready_msg(po, A)
    msgs = [canon] * 12
    for at in range(len(canon)):  # every single-byte mutation
        for v in range(256):
            if v != canon[at]:
                msgs.append(canon[:at] + bytes([v]) + canon[at + 1:])
    for d in range(1, 17):  # truncation and extension
        msgs.append(canon[:-d])
        msgs.append(canon + rng.integers(0, 256, d, dtype=np.uint8).tobytes())
    for length in (31, 33):  # as many characters, the same total length
        m = _ready_msg(po, rng.integers(0, 256, length, dtype=np.uint8).tobytes())
        assert len(m) == len(canon) and _host(po, m)[0] is None
        msgs.append(m)
    msgs.append(_ready_msg(po, B))
    msgs.append(b"")
    judged = [(m,) + _host(po, m) for m in msgs]
    assert judged[0][2] and len(judged) > 16000
    _CORPUS.update(msgs=judged, A=A, B=B)
    return judged, A, B


def _pack(ca, msgs, pinned=True):
    """The messages at 16-byte offsets of one ring: ring, offs, lens."""
    lens = np.array([len(m) for m in msgs], np.uint32)
    steps = (np.maximum(lens, 1).astype(np.uint64) + np.uint64(15)) // np.uint64(16) * np.uint64(16)
    offs = np.concatenate(([0], np.cumsum(steps)[:-1])).astype(np.uint64) if len(msgs) else np.zeros(0, np.uint64)
    total = int(steps.sum()) if len(msgs) else 16
    ring = ca.pinned_empty(total) if pinned else np.empty(total, np.uint8)
    ring[:] = 0
    for m, o in zip(msgs, offs):
        ring[int(o):int(o) + len(m)] = np.frombuffer(m, np.uint8)
    return ring, offs, lens


def _dev(ca, a, guard=0):
    """A device buffer holding array a, with `guard` bytes of GUARD_BYTE behind it."""
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    b = ca.DeviceBuffer(max(a.nbytes + guard, 16))
    b.upload(np.concatenate((a, np.full(max(guard, 16 - a.nbytes, 0), GUARD_BYTE, np.uint8))))
    return b


def _sync(ca):
    assert ca.rbc.lib.rbc_device_sync(0) == 0


# ---------------------------------------------------------------------------
# 1. the mutation corpus
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,f,count", GEOMETRIES)
def test_unmarshal_ready_follows_the_host_decoder_over_the_mutation_corpus(gpu, n, f, count):
    ca = gpu
    judged, A, B = _corpus()
    ctx = ca.Context(n, f)
    try:
        rng = np.random.default_rng(n)
        roots = [B] + [A] * (count - 1)  # instance 0 collects READYs for another root
        msgs = [m for m, _, _ in judged]
        q = np.arange(len(msgs))
        inst = (q % count).astype(np.uint32)
        idx = ((q // count) % n).astype(np.uint8)
        want = np.array([FALLBACK if not canonical else OK if root == roots[i] else OTHER_ROOT
                         for (_, root, canonical), i in zip(judged, inst)], np.int32)
        # an instance or a leaf out of range: FALLBACK, nothing written
        extra = [(count, 0), (0xFFFFFFFF, 0)] + ([(1, n), (1, 255)] if n < 256 else [])
        msgs += [judged[0][0]] * len(extra)
        inst = np.concatenate((inst, np.array([e[0] for e in extra], np.uint32)))
        idx = np.concatenate((idx, np.array([e[1] for e in extra], np.uint8)))
        want = np.concatenate((want, np.full(len(extra), FALLBACK, np.int32)))
        ring, offs, lens = _pack(ca, msgs)
        pattern = (rng.integers(0, 4, (count, n)) == 0).astype(np.uint8)  # 0 and 1
        dring, doffs, dlens, dinst, didx = (_dev(ca, a) for a in (ring, offs, lens, inst, idx))
        droots = _dev(ca, np.frombuffer(b"".join(roots), np.uint8))
        dready = _dev(ca, pattern, GUARD)
        dstatus = _dev(ca, np.full(len(msgs) * 4, GUARD_BYTE, np.uint8), GUARD)
        ctx.dev_unmarshal_ready(None, count, len(msgs), dring, doffs, dlens, dinst, didx, droots, dready, dstatus)
        _sync(ca)
        raw = dstatus.download()
        assert (raw[len(msgs) * 4:len(msgs) * 4 + GUARD] == GUARD_BYTE).all(), "guard after msg_status overwritten"
        status = raw[:len(msgs) * 4].view(np.int32)
        bad = np.nonzero(status != want)[0]
        assert not len(bad), [(int(b), int(status[b]), int(want[b]), msgs[b].hex()) for b in bad[:5]]
        assert {OK, FALLBACK, OTHER_ROOT} == set(np.unique(status))
        expect = pattern.copy()
        okq = np.nonzero(want == OK)[0]
        expect[inst[okq], idx[okq]] = 1
        raw = dready.download()
        assert (raw[count * n:count * n + GUARD] == GUARD_BYTE).all(), "guard after ready overwritten"
        assert np.array_equal(raw[:count * n].reshape(count, n), expect)  # the OK slots, and no other byte
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# 2. accumulation and duplicates
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,f,count", GEOMETRIES)
def test_ready_bitmap_accumulates_over_calls_and_ignores_repeats(gpu, n, f, count):
    import rbc_protocol_oracle as po
    ca = gpu
    ctx = ca.Context(n, f)
    try:
        rng = np.random.default_rng(7 * n)
        roots = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(count)]
        ready_msg = [_ready_msg(po, r) for r in roots]
        senders = [rng.permutation(n)[:max(1, (2 * n) // 3)] for _ in range(count)]
        pairs = [(i, int(j)) for i in range(count) for j in senders[i]]
        pairs = [pairs[q] for q in rng.permutation(len(pairs))]
        third = (len(pairs) + 2) // 3
        calls = [pairs[:third], pairs[third:2 * third], pairs[2 * third:]]
        calls[1] = calls[1] + calls[0][:3] + calls[1][:2]  # repeats of an earlier call, and inside one call
        calls[2] = calls[2] + calls[2][-1:] + calls[0][-2:]
        droots = _dev(ca, np.frombuffer(b"".join(roots), np.uint8))
        dready = ca.DeviceBuffer(max(count * n, 16))
        dready.zero()
        union = np.zeros((count, n), np.uint8)
        for call in calls:
            ring, offs, lens = _pack(ca, [ready_msg[i] for i, _ in call])
            inst = np.array([i for i, _ in call], np.uint32)
            idx = np.array([j for _, j in call], np.uint8)
            bufs = [_dev(ca, a) for a in (ring, offs, lens, inst, idx)]
            dstatus = _dev(ca, np.full(len(call) * 4, GUARD_BYTE, np.uint8), GUARD)
            ctx.dev_unmarshal_ready(None, count, len(call), *bufs, droots, dready, dstatus)
            _sync(ca)
            assert (dstatus.download()[:len(call) * 4].view(np.int32) == OK).all()
            union[inst, idx] = 1
            assert np.array_equal(dready.download()[:count * n].reshape(count, n), union)
        ec, rc, fl = (ca.DeviceBuffer(max(count * 4, 16)) for _ in range(3))
        ctx.dev_quorum(None, count, None, dready, None, -1, ec, rc, fl)
        _sync(ca)
        assert np.array_equal(rc.download()[:count * 4].view(np.uint32), [len(s) for s in senders])
        assert not ec.download()[:count * 4].any()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# 3. the quorum kernel against a model
# ---------------------------------------------------------------------------
def _model(n, f, valid, ready, status, self_id):
    """The four lines of include/rbc_protocol.h over numpy rows."""
    count = len(ready)
    E = (valid != 0).sum(1) if valid is not None else np.zeros(count, np.int64)
    R = (ready != 0).sum(1)
    ok = (status == RBC_OK) if status is not None else np.zeros(count, bool)
    have = ok & ((E >= n - f) | ((R >= 2 * f + 1) & (E >= n - 2 * f)))
    amplify = R >= f + 1
    send = amplify | have
    after = ready.copy()
    if self_id >= 0:
        own = send & (ready[:, self_id] == 0)
        after[own, self_id] = 1
        R = R + own
    deliver = ok & (R >= 2 * f + 1) & (E >= n - 2 * f)
    flags = (E >= n - f) * Q_ECHO + amplify * Q_AMPLIFY + send * Q_SEND_READY + deliver * Q_DELIVER
    return E.astype(np.uint32), R.astype(np.uint32), flags.astype(np.uint8), after


def _rows(rng, n, counts):
    """One row of n bytes per count: that many non-zero bytes at random places."""
    out = np.zeros((len(counts), n), np.uint8)
    for r, c in enumerate(counts):
        out[r, rng.permutation(n)[:c]] = rng.integers(1, 256, c)
    return out


@pytest.mark.parametrize("n,f,count", GEOMETRIES)
def test_quorum_kernel_equals_the_model_at_random_and_boundary_rows(gpu, n, f, count):
    ca = gpu
    ctx = ca.Context(n, f)
    try:
        rng = np.random.default_rng(31 * n + f)
        # the boundary rows of every threshold, under each status; then random rows
        Es = [e for e in (n - 2 * f - 1, n - 2 * f, n - f - 1, n - f) if 0 <= e <= n]
        Rs = [r for r in (f, f + 1, 2 * f, 2 * f + 1) if 0 <= r <= n]
        ecs, rcs, sts = [], [], []
        for e in Es:
            for r in Rs:
                for st in (RBC_OK, TOO_FEW, ROOT_MISMATCH):
                    ecs.append(e), rcs.append(r), sts.append(st)
        for _ in range(40 * count):
            ecs.append(int(rng.integers(0, n + 1))), rcs.append(int(rng.integers(0, n + 1)))
            sts.append((RBC_OK, RBC_OK, TOO_FEW, ROOT_MISMATCH)[int(rng.integers(0, 4))])
        rows = len(ecs)
        valid, ready, status = _rows(rng, n, ecs), _rows(rng, n, rcs), np.array(sts, np.int32)
        own_set = int(np.argmax(ready[0] != 0)) if ready[0].any() else 0
        for self_id in (-1, 0, n - 1, own_set):
            for use_valid, use_status in ((True, True), (False, True), (True, False)):
                dvalid, dready, dstatus = _dev(ca, valid), _dev(ca, ready, GUARD), _dev(ca, status)
                ec, rc = (_dev(ca, np.zeros(rows, np.uint32), GUARD) for _ in range(2))
                fl = _dev(ca, np.zeros(rows, np.uint8), GUARD)
                ctx.dev_quorum(None, rows, dvalid if use_valid else None, dready, dstatus if use_status else None,
                               self_id, ec, rc, fl)
                _sync(ca)
                wE, wR, wF, wready = _model(n, f, valid if use_valid else None, ready,
                                            status if use_status else None, self_id)
                key = (self_id, use_valid, use_status)
                assert np.array_equal(ec.download()[:rows * 4].view(np.uint32), wE), key
                assert np.array_equal(rc.download()[:rows * 4].view(np.uint32), wR), key
                got = fl.download()
                assert np.array_equal(got[:rows], wF), (key, np.nonzero(got[:rows] != wF)[0][:5])
                raw = dready.download()
                assert np.array_equal(raw[:rows * n].reshape(rows, n), wready), key  # only the own byte is written
                for b, size in ((dready, rows * n), (ec, rows * 4), (rc, rows * 4), (fl, rows)):
                    assert (b.download()[size:size + GUARD] == GUARD_BYTE).all(), key
                if use_valid and use_status:
                    assert {0, Q_DELIVER} <= {int(x) & Q_DELIVER for x in wF}, key
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# 4. lock step with OracleNode
# ---------------------------------------------------------------------------
def _broadcast(po, n, f, value):
    """An honest proposer 0 broadcasts `value`: the root, every node's VAL and every node's ECHO."""
    p = po.OracleNode(n, f, 0, 0)
    assert p.propose(value) == 0
    p.progress()
    out = p.messages()
    vals = {to: m for to, m in out if to >= 0}
    echo = {0: next(m for to, m in out if to < 0)}
    for j in range(1, n):
        node = po.OracleNode(n, f, j, 0)
        assert node.handle_message(0, vals[j]) == 0
        node.progress()
        echo[j] = next(m for to, m in node.messages() if to < 0)
    root = po.json_decode(po.pb_decode(echo[0])[1])["root"]
    return root, vals, echo


@pytest.mark.parametrize("schedule", ["echo_led", "ready_led"])
@pytest.mark.parametrize("n,f", [(4, 1), (7, 2)])
def test_quorum_flags_follow_the_oracle_node_batch_by_batch(gpu, n, f, schedule):
    import rbc_protocol_oracle as po
    ca = gpu
    ctx = ca.Context(n, f)
    rcv = wq = None
    try:
        rng = np.random.default_rng(1000 * n + len(schedule))
        me, silent, noisy = 1, n - 1, n - 2
        value = rng.integers(0, 256, 700, dtype=np.uint8).tobytes()
        root, vals, echo = _broadcast(po, n, f, value)
        S = len(po.json_decode(po.pb_decode(echo[0])[1])["block"][0])
        good_ready = _ready_msg(po, root)
        other_ready = _ready_msg(po, bytes(32))
        garbage = [rng.integers(0, 256, len(good_ready), dtype=np.uint8).tobytes(), good_ready[:-1],
                   good_ready[:20] + b"=" + good_ready[21:]]
        assert all(po.pb_decode(g) is None or po.json_decode(po.pb_decode(g)[1]) is None
                   or len(po.json_decode(po.pb_decode(g)[1])["root"]) != 32 for g in garbage)
        others = [int(j) for j in rng.permutation([j for j in range(n) if j not in (me, silent)])]
        readers = [int(j) for j in rng.permutation(others)]  # the order the READYs arrive in
        k = n - 2 * f
        if schedule == "echo_led":   # N-f ECHOs first: interpolate, READY; then the READYs
            e_cut = [n - f - 2, n - f - 1, len(others)]  # ECHOs of others, on top of our own
            r_cut = [0, 0, len(readers)]
        else:                        # f+1 READYs first: amplification; the ECHOs last
            e_cut = [max(k - 2, 0), max(k - 2, 0), len(others)]
            r_cut = [f, f + 1, len(readers)]
        oracle = po.OracleNode(n, f, me, 0)
        rcv = ca.WireReceiver(ctx, 1, n, n * rup(len(echo[0]), 16), rup(S, 64))
        wq = ca.WireQuorum(ctx, 1, 2 * n + 8, (2 * n + 8) * rup(len(good_ready), 16))
        ready = np.zeros((1, n), np.uint8)
        echoes_in = [(me, echo[me])]  # our own ECHO: the oracle counts it when the VAL is proven
        roots = np.frombuffer(root, np.uint8).reshape(1, 32)
        seen = []
        for b in range(3):
            batch = []  # (sender, message) in arrival order
            if b == 0:
                batch.append((0, vals[me]))
                batch += [(noisy, g) for g in garbage]
            new_e = others[(e_cut[b - 1] if b else 0):e_cut[b]]
            new_r = readers[(r_cut[b - 1] if b else 0):r_cut[b]]
            batch += [(j, echo[j]) for j in new_e] + [(j, good_ready) for j in new_r]
            batch = [batch[0]] + [batch[q] for q in 1 + rng.permutation(len(batch) - 1)] if b == 0 else \
                [batch[q] for q in rng.permutation(len(batch))]
            if b == 2:  # behind their first READYs: a second READY of a sender, and one naming another root
                batch += [(readers[0], good_ready), (noisy, other_ready)]
            for sender, m in batch:
                oracle.handle_message(sender, m)
            oracle.progress()
            # the device: every ECHO so far through rbc_wire_receive, this batch's READYs through rbc_wire_quorum
            echoes_in += [(s, m) for s, m in batch if po.pb_decode(m) is not None and po.pb_decode(m)[0] == po.ECHO]
            ring, offs, lens = _pack(ca, [m for _, m in echoes_in])
            got = rcv.receive(ring, offs, lens, [0] * len(echoes_in), [s for s, _ in echoes_in], roots, [S])
            assert (got["verdict"] == 1).all()
            readies = [(s, m) for s, m in batch if not (po.pb_decode(m) is not None and po.pb_decode(m)[0] != po.READY)]
            readies = [(s, m) for s, m in readies if m is not vals[me]]
            rring, roffs, rlens = _pack(ca, [m for _, m in readies])
            res = wq.quorum(ready, ring=rring, offs=roffs, lens=rlens, inst=[0] * len(readies),
                            idx=[s for s, _ in readies], roots=roots, valid=got["valid"], status=got["status"],
                            self_id=me)
            st = oracle.roots[root]
            flags = int(res["flags"][0])
            seen.append((bool(flags & Q_SEND_READY), bool(flags & Q_DELIVER)))
            assert bool(flags & Q_SEND_READY) == oracle.ready_sent, (b, flags)
            assert bool(flags & Q_DELIVER) == oracle.delivered, (b, flags)
            assert int(res["ready_counts"][0]) == st.readies and int(res["echo_counts"][0]) == st.echoes, b
            assert np.array_equal(ready[0] != 0, np.array(st.ready)), b
            for (s, m), v in zip(readies, res["verdict"]):
                assert v == (OK if m is good_ready else OTHER_ROOT if m is other_ready else FALLBACK), (b, s)
        assert seen[0] == (False, False) and seen[2] == (True, True), seen
        assert oracle.value() == value
        assert got["values"][0, :k * S].tobytes()[8:8 + len(value)] == value
    finally:
        for h in (rcv, wq):
            if h is not None:
                h.close()
        ctx.close()


# ---------------------------------------------------------------------------
# 5. rbc_wire_quorum end to end
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,f,count", GEOMETRIES)
def test_wire_quorum_equals_the_device_pair_from_pinned_and_pageable_memory(gpu, n, f, count):
    import rbc_protocol_oracle as po
    ca = gpu
    ctx = ca.Context(n, f)
    wq = None
    try:
        rng = np.random.default_rng(5 * n + 1)
        roots = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(count)]
        msgs, inst, idx = [], [], []
        for i in range(count):
            for j in rng.permutation(n)[:int(rng.integers(1, n + 1))]:
                roll = int(rng.integers(0, 8))
                m = _ready_msg(po, roots[i] if roll else roots[(i + 1) % count])   # 1 in 8: another root
                if roll == 1:
                    m = m[:30] + b" " + m[31:]                                       # 1 in 8: not canonical
                msgs.append(m), inst.append(i), idx.append(int(j))
        msgs.append(msgs[0]), inst.append(inst[0]), idx.append(idx[0])               # a repeat
        # one of each kind whatever the dice gave: a good one, another root, not canonical
        msgs.append(_ready_msg(po, roots[0])), inst.append(0), idx.append(0)
        msgs.append(_ready_msg(po, roots[1])), inst.append(0), idx.append(1)
        msgs.append(_ready_msg(po, roots[0])[:-1] + b"\x01"), inst.append(0), idx.append(2)
        inst, idx = np.array(inst, np.uint32), np.array(idx, np.uint8)
        ecounts = [n - f, n - 2 * f, int(rng.integers(0, n + 1))][:count]
        valid = _rows(rng, n, ecounts)
        status = np.array([RBC_OK, RBC_OK, TOO_FEW][:count], np.int32)
        before = (rng.integers(0, 5, (count, n)) == 0).astype(np.uint8)
        self_id = int(rng.integers(0, n))
        # the rbc_dev_* pair
        ring, offs, lens = _pack(ca, msgs)
        bufs = [_dev(ca, a) for a in (ring, offs, lens, inst, idx)]
        droots, dready = _dev(ca, np.frombuffer(b"".join(roots), np.uint8)), _dev(ca, before)
        dstatus = ca.DeviceBuffer(len(msgs) * 4)
        dvalid, dst = _dev(ca, valid), _dev(ca, status)
        ec, rc, fl = (ca.DeviceBuffer(max(count * 4, 16)) for _ in range(3))
        ctx.dev_unmarshal_ready(None, count, len(msgs), *bufs, droots, dready, dstatus)
        ctx.dev_quorum(None, count, dvalid, dready, dst, self_id, ec, rc, fl)
        _sync(ca)
        want = {"verdict": dstatus.download()[:len(msgs) * 4].view(np.int32).astype(np.uint8),
                "ready": dready.download()[:count * n].reshape(count, n),
                "echo_counts": ec.download()[:count * 4].view(np.uint32),
                "ready_counts": rc.download()[:count * 4].view(np.uint32), "flags": fl.download()[:count]}
        assert {OK, FALLBACK, OTHER_ROOT} == set(want["verdict"]) and np.array_equal(want["echo_counts"], ecounts)
        wq = ca.WireQuorum(ctx, count, len(msgs), ring.nbytes)
        for pinned in (True, False):
            r2 = ring if pinned else np.array(ring)
            ready = before.copy()
            got = wq.quorum(ready, ring=r2, offs=offs, lens=lens, inst=inst, idx=idx,
                            roots=np.frombuffer(b"".join(roots), np.uint8), valid=valid, status=status,
                            self_id=self_id)
            for name in want:
                assert np.array_equal(got[name], want[name]), (pinned, name)
            assert np.array_equal(ready, want["ready"])  # updated in place
            # no messages: the same bitmap re-tallied gives the same counts and flags, and changes nothing
            again = wq.quorum(ready, valid=valid, status=status, self_id=self_id)
            assert np.array_equal(again["ready"], want["ready"]) and len(again["verdict"]) == 0
            assert np.array_equal(again["ready_counts"], want["ready_counts"])
            assert np.array_equal(again["echo_counts"], want["echo_counts"])
            # the own bit is in the bitmap now, so the flags only differ where it tipped AMPLIFY
            wE, wR, wF, _ = _model(n, f, valid, ready, status, self_id)
            assert np.array_equal(again["flags"], wF) and np.array_equal(again["ready_counts"], wR)
            # ... and after new ECHO results
            full = wq.quorum(ready, valid=np.ones((count, n), np.uint8), status=np.zeros(count, np.int32),
                             self_id=self_id)
            assert (full["echo_counts"] == n).all() and (full["flags"] & Q_SEND_READY).all()
    finally:
        if wq is not None:
            wq.close()
        ctx.close()
