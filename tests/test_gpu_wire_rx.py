"""Device-side unmarshal of received VAL / ECHO messages (rbc_dev_unmarshal_val,
csrc/wire.hip) and the validate-from-the-wire entry built on it
(rbc_wire_validate, csrc/wire_rx.cpp).

* Round trip: rbc_dev_marshal_val then rbc_dev_unmarshal_val returns the
  marshal's inputs, for every padding count, both types and the geometries
  with an empty level-0 sibling; nothing outside a message's slots is written.
* Hostile bytes: over a seeded corpus of mutated messages, status OK implies
  that the host decoder (rbc_pb_decode_rbc + rbc_json_decode_val) accepts the
  same bytes with byte-equal fields, and every in-alphabet substitution off
  the padding is decoded on the device.
* End to end: ECHOs from a pinned (and a pageable) ring through
  rbc_wire_validate against the oracle's validateMessage, then
  rbc_interpolate_batch_kept over the kept rows.
* Argument errors enqueue nothing.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, FALLBACK = 0, 1
CANARY = 0xC7
GUARD = 256
ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"


def rup(x, a):
    return (x + a - 1) // a * a


class Outputs:
    """The unmarshal's output buffers, canary-filled, each with a guard region behind it."""

    def __init__(self, ca, count, depth, row_pitch):
        self.count, self.row_pitch, self.bslot = count, row_pitch, max(depth, 1) * 32
        self.sizes = {"rows": count * row_pitch, "slens": count * 4, "branches": count * self.bslot,
                      "roots": count * 32, "types": count, "status": count * 4}
        self.dev = {}
        for name, size in self.sizes.items():
            self.dev[name] = ca.DeviceBuffer(size + GUARD)
            self.dev[name].upload(np.full(size + GUARD, CANARY, np.uint8))

    def download(self):
        """status, types, slens, roots, branches, rows; asserts every guard region intact."""
        got = {}
        for name, size in self.sizes.items():
            raw = self.dev[name].download()
            assert (raw[size:] == CANARY).all(), f"guard after {name} overwritten"
            got[name] = raw[:size]
        c = self.count
        return (got["status"].view(np.int32), got["types"], got["slens"].view(np.uint32),
                got["roots"].reshape(c, 32), got["branches"].reshape(c, self.bslot),
                got["rows"].reshape(c, self.row_pitch))


def unmarshal(ca, ctx, outs, dmsgs, offs, lens, idx):
    count = len(offs)
    doffs, dlens, didx = ca.DeviceBuffer(count * 8), ca.DeviceBuffer(count * 4), ca.DeviceBuffer(count)
    doffs.upload(np.ascontiguousarray(offs, np.uint64))
    dlens.upload(np.ascontiguousarray(lens, np.uint32))
    didx.upload(np.ascontiguousarray(idx, np.uint8))
    d = outs.dev
    ctx.dev_unmarshal_val(None, count, dmsgs, doffs, dlens, didx, d["rows"], outs.row_pitch, d["slens"],
                          d["branches"], d["roots"], d["types"], d["status"])
    ca.rbc.lib.rbc_device_sync(0)
    return outs.download()


ROUND_TRIP_S = [1, 2, 3, 4, 15, 16, 17, 47, 48, 49, 63, 64, 65, 1000]


@pytest.mark.parametrize("n,f", [(4, 1), (5, 1), (7, 2), (16, 5)])
@pytest.mark.parametrize("msg_type", [0, 1])
def test_marshal_then_unmarshal_returns_the_inputs(gpu, n, f, msg_type):
    ca = gpu
    ctx = ca.Context(n, f)
    try:
        d = ctx.depth
        rng = np.random.default_rng(100 * n + msg_type)
        slens = np.repeat(np.array(ROUND_TRIP_S, np.uint32), 3)  # three instances of every S
        count = len(slens)
        pitch = rup(int(slens.max()), 64)
        sh = np.zeros((count, n, pitch), np.uint8)
        for i, S in enumerate(slens):
            sh[i, :, :S] = rng.integers(0, 256, (n, S), dtype=np.uint8)
        br = rng.integers(0, 256, (count, n, d, 32), dtype=np.uint8)
        roots = rng.integers(0, 256, (count, 32), dtype=np.uint8)
        out_pitch = rup(max(ctx.val_message_size(int(slens.max()), j, msg_type) for j in (0, n - 1)), 16)
        dsh, dbr, drt = ca.DeviceBuffer(sh.nbytes), ca.DeviceBuffer(br.nbytes), ca.DeviceBuffer(roots.nbytes)
        dln, dout, dol = ca.DeviceBuffer(count * 4), ca.DeviceBuffer(count * n * out_pitch), ca.DeviceBuffer(count * n * 4)
        dsh.upload(sh)
        dbr.upload(br.reshape(-1))
        drt.upload(roots.reshape(-1))
        dln.upload(slens)
        dout.upload(np.full(count * n * out_pitch, 0xEE, np.uint8))
        ctx.dev_marshal_val(None, count, msg_type, dsh, pitch, dln, 0, dbr, drt, dout, out_pitch, dol)
        ca.rbc.lib.rbc_device_sync(0)
        mlens = dol.download().view(np.uint32)
        msgs = count * n
        # a row slot wider than the widest shard: the rest of every slot must stay untouched
        row_pitch = pitch + 64
        outs = Outputs(ca, msgs, d, row_pitch)
        idx = np.tile(np.arange(n, dtype=np.uint8), count)
        status, types, S_out, r_out, b_out, rows = unmarshal(ca, ctx, outs, dout, np.arange(msgs) * out_pitch, mlens,
                                                              idx)
        assert (status == OK).all(), np.nonzero(status)[0][:10]
        assert (types == msg_type).all()
        assert np.array_equal(S_out, np.repeat(slens, n))
        assert np.array_equal(r_out, np.repeat(roots, n, axis=0))
        want_br = br.copy()
        for j in range(n):
            if (j ^ 1) >= n:
                want_br[:, j, 0] = 0  # the empty level-0 sibling: a zero slot
        assert np.array_equal(b_out, want_br.reshape(msgs, d * 32))
        rows = rows.reshape(count, n, row_pitch)
        for i, S in enumerate(slens):
            S = int(S)
            assert np.array_equal(rows[i, :, :S], sh[i, :, :S]), (i, S)
            assert not rows[i, :, S:rup(S, 64)].any(), (i, S)
            assert (rows[i, :, rup(S, 64):] == CANARY).all(), (i, S)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# hostile bytes
# ---------------------------------------------------------------------------
def _varint(v, extra=0):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    for _ in range(extra):  # redundant continuation bytes: not minimal
        out[-1] |= 0x80
        out.append(0)
    return bytes(out)


def _runs(msg):
    """[begin, end) of the three base64 runs of a canonical message (root, branch, block)."""
    q = [i for i, c in enumerate(msg) if c == 0x22]
    assert len(q) == 12
    return [(q[4 * k + 2] + 1, q[4 * k + 3]) for k in range(3)]


def _corpus(protocol, n, depth):
    """(bytes, idx, must_be_ok) of the mutated messages."""
    rng = np.random.default_rng(20261019)
    below = lambda m: int(rng.integers(0, m))  # noqa: E731
    out = []
    for base in range(42):
        S = (5, 64, 100)[base % 3]
        idx = (base // 3) % n
        mtype = (base // 21) % 2
        empty0 = (idx ^ 1) >= n
        root, br, blk = (rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in (32, 32 * (depth - empty0), S))
        json = protocol.json_encode_val(root, br, blk)
        canon = protocol.pb_encode(mtype, json)
        runs = _runs(canon)
        out.append((canon, idx, True))
        for _ in range(6):
            rb, re = runs[below(3)]
            npad = len(canon[rb:re]) - len(canon[rb:re].rstrip(b"="))
            sub = lambda at, c: canon[:at] + bytes([c]) + canon[at + 1:]  # noqa: E731
            ins = lambda at, c: canon[:at] + bytes([c]) + canon[at:]  # noqa: E731
            out.append((sub(rb + below(re - rb - npad), ALPHABET[below(64)]), idx, True))
            out.append((sub(re - npad - 1, ALPHABET[below(64)]), idx, True))  # trailing bits may be anything
            out.append((sub(rb + below(re - rb), b"-_ .,\\\x7f\x80\xff\x00@[`{"[below(14)]), idx, False))
            out.append((sub(rb + below(re - rb - npad), ord("=")), idx, False))
            at = below(len(canon))
            out.append((sub(at, canon[at] ^ (1 << below(8))), idx, False))
            out.append((canon[:below(len(canon))], idx, False))
            out.append((canon + rng.integers(0, 256, 1 + below(5), dtype=np.uint8).tobytes(), idx, False))
            j0 = runs[0][0] - 13
            out.append((ins(j0 + below(len(canon) - j0), b" \t\n\r"[below(4)]), idx, False))
            out.append((ins(rb + below(re - rb), 0x0A), idx, False))
            out.append((canon, (idx + 1 + below(n - 1)) % n, False))
        # the JSON re-wrapped with true lengths: forms the host decoder accepts but that are not canonical
        at = runs[2][0] - (runs[0][0] - 13)
        bpos = json.find(b',"Block":')
        for js in (b" " + json, json + b"\n", json.replace(b"RootHash", b"roothash"), json.replace(b"Block", b"BLOCK"),
                   json[:-1] + b',"Extra":"AAAA"}', b'{"Extra":[1,{"a":null}],' + json[1:],
                   json.replace(b"RootHash", b"Root\\u0048ash"),
                   b"{" + json[bpos + 1:-1] + b"," + json[1:bpos] + b"}",
                   json[:at] + b"\\u%04x" % json[at] + json[at + 1:], json[:at + 4] + b"\\n" + json[at + 4:],
                   json.replace(b":", b": ", 1)):
            out.append((protocol.pb_encode(mtype, js), idx, False))
        tail = bytes([0x10, mtype]) if mtype else b""
        for variant in range(6):
            J = len(json)
            vj = _varint(J + (variant == 2) - (variant == 3), extra=int(variant == 1))
            R = 1 + len(vj) + J + len(tail) + (variant == 4) - (variant == 5)
            out.append((b"\x1a" + _varint(R, extra=int(variant == 0)) + b"\x0a" + vj + json + tail, idx, False))
        if mtype:
            out.append((canon[:-1] + b"\x02", idx, False))  # READY
            out.append((canon[:-1] + b"\x81", idx, False))
    for length in range(0, 120):  # shorter than any canonical message, and random bytes of its size
        m = rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        out.append(((b"\x1a" + m[1:]) if length else m, 0, False))
    return out


def test_unmarshal_agrees_with_the_host_decoder_on_hostile_bytes(gpu):
    import rbc_oracle as orc
    from cleisthenes_amd import protocol
    ca = gpu
    n, f = 7, 2
    ctx = ca.Context(n, f)
    try:
        d = ctx.depth
        corpus = _corpus(protocol, n, d)
        count = len(corpus)
        assert count > 3000
        # lens and offs describe bytes really present: the arena ends with the last message's last chunk
        offs = np.zeros(count, np.uint64)
        at = 0
        for i, (m, _, _) in enumerate(corpus):
            offs[i] = at
            at += rup(max(len(m), 1), 16)
        arena = np.zeros(at, np.uint8)
        for (m, _, _), o in zip(corpus, offs):
            arena[int(o):int(o) + len(m)] = np.frombuffer(m, np.uint8)
        dar = ca.DeviceBuffer(at)
        dar.upload(arena)
        row_pitch = 192
        outs = Outputs(ca, count, d, row_pitch)
        status, types, S_out, r_out, b_out, rows = unmarshal(ca, ctx, outs, dar, offs, [len(m) for m, _, _ in corpus],
                                                              [ix for _, ix, _ in corpus])
        assert set(np.unique(status)) <= {OK, FALLBACK}
        n_ok = 0
        for i, (m, idx, must) in enumerate(corpus):
            if status[i] != OK:
                assert not must, (i, "an in-alphabet substitution (or a canonical message) fell back")
                assert S_out[i] == 0
                continue
            n_ok += 1
            try:  # status OK: the host decoder accepts the same bytes, with the same fields
                t, payload = protocol.pb_decode(m)
                req = protocol.json_decode_val(payload)
            except ca.RBCError:
                raise AssertionError(f"message {i}: decoded on the device, rejected by the host decoder")
            blk = req["Block"][0]
            assert types[i] == t and t in (protocol.VAL, protocol.ECHO), i
            assert bytes(r_out[i]) == req["RootHash"], i
            assert S_out[i] == len(blk) and bytes(rows[i, :len(blk)]) == blk, i
            assert not rows[i, len(blk):rup(len(blk), 64)].any(), i
            assert (rows[i, rup(len(blk), 64):] == CANARY).all(), i
            levels = orc.unflatten_branch(req["Branch"], idx, n)
            assert levels is not None, (i, "a branch of another length decoded")
            assert bytes(b_out[i]) == b"".join(lv if lv else bytes(32) for lv in levels), i
        assert n_ok >= sum(must for _, _, must in corpus) > 500
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# end to end through rbc_wire_validate
# ---------------------------------------------------------------------------
def _echo_ring(ca, ctx, values):
    """shard + commit `values`, marshal every ECHO on the device; returns the commitment and the messages."""
    n, d = ctx.n, ctx.depth
    c = ctx.shard_commit_batch(values)
    count = len(values)
    slens = c["shard_lens"].astype(np.uint32)
    pitch = rup(int(slens.max()), 64)
    sh = np.zeros((count, n, pitch), np.uint8)
    sh[:, :, :c["shards"].shape[2]] = c["shards"]
    br = np.ascontiguousarray(c["branches"]).reshape(count, n, d, 32)
    out_pitch = rup(max(ctx.val_message_size(int(slens.max()), j, 1) for j in (0, n - 1)), 16)
    dsh, dbr, drt = ca.DeviceBuffer(sh.nbytes), ca.DeviceBuffer(br.nbytes), ca.DeviceBuffer(count * 32)
    dln, dout, dol = ca.DeviceBuffer(count * 4), ca.DeviceBuffer(count * n * out_pitch), ca.DeviceBuffer(count * n * 4)
    dsh.upload(sh)
    dbr.upload(br.reshape(-1))
    drt.upload(np.ascontiguousarray(c["roots"]).reshape(-1))
    dln.upload(slens)
    ctx.dev_marshal_val(None, count, 1, dsh, pitch, dln, 0, dbr, drt, dout, out_pitch, dol)
    ca.rbc.lib.rbc_device_sync(0)
    out = dout.download().reshape(count * n, out_pitch)
    ol = dol.download().view(np.uint32)
    return c, slens, [bytes(out[m, :ol[m]]) for m in range(count * n)]


def test_wire_validate_then_interpolate_from_the_kept_rows(gpu):
    import rbc_oracle as orc
    from cleisthenes_amd import protocol
    ca = gpu
    n, f = 16, 5
    ctx = ca.Context(n, f)
    rx = None
    try:
        k = ctx.k
        rng = np.random.default_rng(16)
        values = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in (6 * 333 + 1, 700, 6 * 1024)]
        c, slens, msgs = _echo_ring(ca, ctx, values)
        count = len(values)
        idx = np.tile(np.arange(n, dtype=np.uint8), count)
        # one in-alphabet corruption of a shard character, one whitespace-padded message, one wrong idx
        m = msgs[0 * n + 2]
        at = _runs(m)[2][0] + 7
        msgs[0 * n + 2] = m[:at] + (b"A" if m[at:at + 1] != b"A" else b"B") + m[at + 1:]
        t, payload = protocol.pb_decode(msgs[1 * n + 3])
        msgs[1 * n + 3] = protocol.pb_encode(t, payload.replace(b":", b": ", 1))
        idx[2 * n + 5] = 6
        offs = np.zeros(len(msgs), np.uint64)
        at = 0
        for i, m in enumerate(msgs):
            offs[i] = at
            at += rup(len(m), 16)
        lens = np.array([len(m) for m in msgs], np.uint32)
        ring = ca.pinned_empty(at)
        ring[:] = 0
        for m, o in zip(msgs, offs):
            ring[int(o):int(o) + len(m)] = np.frombuffer(m, np.uint8)
        row_pitch = rup(int(slens.max()), 64)
        rx = ca.WireRx(ctx, len(msgs), at, row_pitch)
        keep = ca.DeviceBuffer(len(msgs) * row_pitch)
        got = rx.validate(ring, offs, lens, idx, keep)
        # the oracle's validateMessage over the host-decoded fields
        want = np.zeros(len(msgs), np.uint8)
        for i, m in enumerate(msgs):
            t, payload = protocol.pb_decode(m)
            req = protocol.json_decode_val(payload)
            if protocol.pb_encode(t, protocol.json_encode_val(req["RootHash"], req["Branch"], req["Block"][0])) != m:
                want[i] = 2  # accepted by the host decoder, but not in the canonical form
                continue
            levels = orc.unflatten_branch(req["Branch"], int(idx[i]), n)
            want[i] = levels is not None and orc.merkle_verify(n, req["Block"][0], req["RootHash"], levels, int(idx[i]))
            assert got["types"][i] == t and bytes(got["roots"][i]) == req["RootHash"], i
            assert got["shard_lens"][i] == len(req["Block"][0]), i
            assert bytes(got["leaves"][i]) == orc.sha256(req["Block"][0]), i
        assert np.array_equal(got["verdict"], want)
        assert want[0 * n + 2] == 0 and want[1 * n + 3] == 2 and want[2 * n + 5] == 0 and (want == 1).sum() == len(msgs) - 3
        # interpolate from the kept rows: the first N - f valid rows of every proposal
        rows = np.zeros((count, n), np.uint64)
        leaves = np.zeros((count, n, 32), np.uint8)
        for i in range(count):
            valid = [j for j in range(n) if got["verdict"][i * n + j] == 1][:n - f]
            assert len(valid) == n - f
            for j in valid:
                rows[i, j] = keep.value + (i * n + j) * row_pitch
                leaves[i, j] = got["leaves"][i * n + j]
        res = ctx.interpolate_kept_submit(rows, [int(s) for s in slens], c["roots"], leaves=leaves).wait()
        assert (res["status"] == 0).all()
        for i, v in enumerate(values):
            S = int(slens[i])
            assert res["values"][i, :k * S].tobytes() == v + bytes(k * S - len(v)), i
        # the same call from a pageable ring
        again = rx.validate(np.array(ring), offs, lens, idx, keep)
        for name in got:
            assert np.array_equal(again[name][want != 2], got[name][want != 2]), name
        assert np.array_equal(again["verdict"], got["verdict"])
    finally:
        if rx is not None:
            rx.close()
        ctx.close()


def test_wire_validate_rejects_bad_arguments_and_then_still_works(gpu):
    from cleisthenes_amd import protocol
    ca = gpu
    n, f = 4, 1
    ctx = ca.Context(n, f)
    rx = None
    try:
        rng = np.random.default_rng(4)
        msgs, comms = [], []
        for j in range(n):
            v = rng.integers(0, 256, 90 + j, dtype=np.uint8).tobytes()
            s = ctx.shard(v)
            comms.append(s)
            msgs.append(protocol.pb_encode(protocol.ECHO, protocol.json_encode_val(s["root"], s["branches"][j],
                                                                                  bytes(s["shards"][j]))))
        offs = np.arange(n, dtype=np.uint64) * 256
        lens = np.array([len(m) for m in msgs], np.uint32)
        assert lens.max() <= 256
        idx = np.arange(n, dtype=np.uint8)
        ring = ca.pinned_empty(n * 256)
        ring[:] = 0
        for m, o in zip(msgs, offs):
            ring[int(o):int(o) + len(m)] = np.frombuffer(m, np.uint8)
        rx = ca.WireRx(ctx, n, ring.nbytes, 64)
        keep = ca.DeviceBuffer(n * 64)
        keep.upload(np.full(n * 64, CANARY, np.uint8))
        small = ca.DeviceBuffer(n * 64 - 64)

        def rejected(*a, **kw):
            with pytest.raises(ca.RBCError) as e:
                rx.validate(*a, **kw)
            assert e.value.code == -10  # RBC_ERR_INVALID_ARG
            assert (keep.download() == CANARY).all()  # nothing was enqueued

        rejected(ring, offs + np.array([0, 8, 0, 0], np.uint64), lens, idx, keep)       # misaligned offs
        rejected(ring, offs, lens, idx, keep, ring_bytes=int(offs[-1]) + 16)            # a message past ring_bytes
        rejected(ring, offs, lens, np.array([0, 1, n, 3], np.uint8), keep)              # idx >= n
        rejected(ring, offs, lens, idx, small)                                          # keep_bytes too small
        rejected(ring, np.append(offs, 0), np.append(lens, lens[0]), np.append(idx, 0), keep)  # count > max_msgs
        got = rx.validate(ring, offs, lens, idx, keep)
        assert (got["verdict"] == 1).all()
        for j in range(n):
            assert bytes(got["roots"][j]) == comms[j]["root"]
            S = len(comms[j]["shards"][j])
            assert bytes(keep.download(S, j * 64)) == bytes(comms[j]["shards"][j])
    finally:
        if rx is not None:
            rx.close()
        ctx.close()
