"""The binary VAL / ECHO payload codec on the device wire path
(RBC_HAS_WIRE_BINARY: marshal_val_bin_kernel, unmarshal_val_bin_kernel and
unmarshal_echo_bin_kernel in csrc/wire.hip, chosen by Context.set_wire_codec).

Expected bytes come from tests/wire_bin.py, a restatement of the format table,
never from the code under test.  Every output buffer is canary-filled with a
guard region behind it.
"""
import numpy as np
import pytest

import wire_bin as wb

pytestmark = pytest.mark.gpu

OK, FALLBACK, OTHER_ROOT, OTHER_LEN = 0, 1, 2, 3
CANARY = 0xC7
GUARD = 256


def rup(x, a):
    return (x + a - 1) // a * a


def dev(ca, a):
    a = np.ascontiguousarray(a)
    b = ca.DeviceBuffer(max(a.nbytes, 16))
    b.upload(a.view(np.uint8).reshape(-1))
    return b


def canaried(ca, size):
    b = ca.DeviceBuffer(size + GUARD)
    b.upload(np.full(size + GUARD, CANARY, np.uint8))
    return b


def checked(buf, size, name):
    raw = buf.download()
    assert (raw[size:] == CANARY).all(), f"guard after {name} overwritten"
    return raw[:size]


def pack(ca, msgs, pinned=True):
    """The messages at 16-byte offsets of one ring that ends with the last one's last chunk."""
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


def flat(n, j, br_dev):
    """Go flat form of leaf j's device-form branch [depth][32]."""
    d = br_dev.shape[0]
    return b"".join(bytes(br_dev[lv]) for lv in range(d) if not (lv == 0 and (j ^ 1) >= n))


def binary_ctx(ca, n, f):
    ctx = ca.Context(n, f)
    assert ctx.wire_codec == "json"  # the default
    ctx.set_wire_codec("binary")
    assert ctx.wire_codec == "binary"
    return ctx


class Outputs:
    """dev_unmarshal_val's output buffers."""

    def __init__(self, ca, count, depth, row_pitch):
        self.count, self.row_pitch, self.bslot = count, row_pitch, max(depth, 1) * 32
        self.sizes = {"rows": count * row_pitch, "slens": count * 4, "branches": count * self.bslot,
                      "roots": count * 32, "types": count, "status": count * 4}
        self.dev = {name: canaried(ca, size) for name, size in self.sizes.items()}

    def download(self):
        got = {name: checked(self.dev[name], size, name) for name, size in self.sizes.items()}
        c = self.count
        return (got["status"].view(np.int32), got["types"], got["slens"].view(np.uint32),
                got["roots"].reshape(c, 32), got["branches"].reshape(c, self.bslot),
                got["rows"].reshape(c, self.row_pitch))


def unmarshal(ca, ctx, outs, dmsgs, offs, lens, idx):
    count = len(offs)
    doffs, dlens, didx = dev(ca, np.asarray(offs, np.uint64)), dev(ca, np.asarray(lens, np.uint32)), \
        dev(ca, np.asarray(idx, np.uint8))
    d = outs.dev
    ctx.dev_unmarshal_val(None, count, dmsgs, doffs, dlens, didx, d["rows"], outs.row_pitch, d["slens"],
                          d["branches"], d["roots"], d["types"], d["status"])
    ca.rbc.lib.rbc_device_sync(0)
    return outs.download()


# ---------------------------------------------------------------------------
# marshal bytes and the round trip
# ---------------------------------------------------------------------------
# every shard phase against the 16-byte chunks, the 64-byte row rounding, more than one lane-step
GRID_S = [1, 2, 3, 15, 16, 17, 47, 48, 49, 63, 64, 65, 1000]
# n = 4: varint(J) and varint(R) grow here, one after the other, and the shard's phase moves
VARINT_S = list(range(20, 26)) + list(range(16274, 16284))


def marshal_and_back(ca, ctx, msg_type, slens, seed):
    """dev_marshal_val of one instance per S against the restatement, then dev_unmarshal_val of its output."""
    n, d = ctx.n, ctx.depth
    rng = np.random.default_rng(seed)
    slens = np.asarray(slens, np.uint32)
    count = len(slens)
    pitch = rup(int(slens.max()), 64)
    sh = np.zeros((count, n, pitch), np.uint8)
    for i, S in enumerate(slens):
        sh[i, :, :S] = rng.integers(0, 256, (n, S), dtype=np.uint8)
    br = rng.integers(0, 256, (count, n, max(d, 1), 32), dtype=np.uint8)[:, :, :d]
    roots = rng.integers(0, 256, (count, 32), dtype=np.uint8)
    need = rup(max(ctx.val_message_size(int(slens.max()), j, msg_type) for j in (0, n - 1)), 16)
    assert need == rup(max(wb.message_size(n, int(slens.max()), j, msg_type) for j in (0, n - 1)), 16)
    out_pitch = need + 32  # room behind the longest message: it must stay untouched
    dsh, dbr, drt, dln = dev(ca, sh), dev(ca, br), dev(ca, roots), dev(ca, slens)
    msgs = count * n
    dout, dol = canaried(ca, msgs * out_pitch), canaried(ca, msgs * 4)
    ctx.dev_marshal_val(None, count, msg_type, dsh, pitch, dln, 0, dbr, drt, dout, out_pitch, dol)
    ca.rbc.lib.rbc_device_sync(0)
    out = checked(dout, msgs * out_pitch, "messages").reshape(msgs, out_pitch)
    mlens = checked(dol, msgs * 4, "message lengths").view(np.uint32)
    for i in range(count):
        S = int(slens[i])
        for j in range(n):
            want = wb.message(msg_type, bytes(roots[i]), flat(n, j, br[i, j]), bytes(sh[i, j, :S]))
            q = i * n + j
            assert mlens[q] == len(want), (S, j)
            assert bytes(out[q, :len(want)]) == want, (S, j)
            assert not out[q, len(want):rup(len(want), 16)].any(), (S, j)      # zeroed up to the next 16
            assert (out[q, rup(len(want), 16):] == CANARY).all(), (S, j)       # and nothing behind
    # back: a row slot wider than the widest shard, whose rest must stay untouched
    row_pitch = pitch + 64
    outs = Outputs(ca, msgs, d, row_pitch)
    idx = np.tile(np.arange(n, dtype=np.uint8), count)
    status, types, S_out, r_out, b_out, rows = unmarshal(ca, ctx, outs, dout, np.arange(msgs) * out_pitch, mlens, idx)
    assert (status == OK).all(), np.nonzero(status)[0][:10]
    assert (types == msg_type).all()
    assert np.array_equal(S_out, np.repeat(slens, n))
    assert np.array_equal(r_out, np.repeat(roots, n, axis=0))
    want_br = np.zeros((count, n, max(d, 1), 32), np.uint8)
    want_br[:, :, :d] = br
    for j in range(n):
        if d and (j ^ 1) >= n:
            want_br[:, j, 0] = 0  # the empty level-0 sibling: a zero slot
    assert np.array_equal(b_out, want_br.reshape(msgs, -1))
    rows = rows.reshape(count, n, row_pitch)
    for i, S in enumerate(slens):
        S = int(S)
        assert np.array_equal(rows[i, :, :S], sh[i, :, :S]), S
        assert not rows[i, :, S:rup(S, 64)].any(), S
        assert (rows[i, :, rup(S, 64):] == CANARY).all(), S


@pytest.mark.parametrize("n,f", [(4, 1), (5, 1), (7, 2), (16, 5), (256, 85)])
@pytest.mark.parametrize("msg_type", [0, 1])
def test_marshal_equals_the_restatement_and_unmarshal_returns_the_inputs(gpu, n, f, msg_type):
    ctx = binary_ctx(gpu, n, f)
    try:
        marshal_and_back(gpu, ctx, msg_type, GRID_S + (VARINT_S if n == 4 else []), 100 * n + msg_type)
    finally:
        ctx.close()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_marshal_where_the_varint_grows_to_four_bytes(gpu, delta):
    ctx = binary_ctx(gpu, 4, 1)
    try:
        S = 2 ** 21 - 104 + delta
        assert len(wb.varint(40 + 64 + S)) == (3 if delta < 0 else 4)
        marshal_and_back(gpu, ctx, 0, [S], 21 + delta)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# one total, two types; totals nobody has
# ---------------------------------------------------------------------------
def test_a_total_shared_by_val_and_echo_decodes_by_its_header(gpu):
    ca = gpu
    n = 4
    ctx = binary_ctx(ca, n, 1)
    try:
        rng = np.random.default_rng(2)
        root, br = rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
        S = 50
        val = wb.message(wb.VAL, root, br, rng.integers(0, 256, S - 2, dtype=np.uint8).tobytes() + b"\x10\x01")
        echo = wb.message(wb.ECHO, root, br, rng.integers(0, 256, S - 2, dtype=np.uint8).tobytes())
        assert len(val) == len(echo)
        # 130 at n = 4 and 16387 anywhere: a varint grows there, no (S, type) has that total
        assert wb.unreachable_totals(n, 0, 0, 200) == [130] and wb.unreachable_totals(n, 0, 16300, 16500) == [16387]
        odd = [wb.message(wb.VAL, root, br, bytes(200))[:130], wb.message(wb.ECHO, root, br, bytes(16400))[:16387]]
        msgs = [val, echo] + odd
        ring, offs, lens = pack(ca, msgs)
        outs = Outputs(ca, len(msgs), ctx.depth, 16448)
        status, types, S_out, r_out, b_out, rows = unmarshal(ca, ctx, outs, dev(ca, ring), offs, lens, [0, 1, 2, 3])
        assert list(status) == [OK, OK, FALLBACK, FALLBACK]
        assert list(types[:2]) == [wb.VAL, wb.ECHO] and list(S_out) == [S, S - 2, 0, 0]
        assert bytes(rows[0, :S]) == val[-S:] and bytes(rows[1, :S - 2]) == echo[-S:-2]
        assert not rows[0, S:64].any() and not rows[1, S - 2:64].any()
        assert (rows[:2, 64:] == CANARY).all() and (rows[2:] == CANARY).all()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# hostile bytes
# ---------------------------------------------------------------------------
def hostile_corpus(protocol, n):
    """(bytes, idx): valid messages and their mutants, as the CPU fuzz program builds them."""
    rng = np.random.default_rng(20261019)
    rnd = lambda L: rng.integers(0, 256, L, dtype=np.uint8).tobytes()  # noqa: E731
    out = []
    bases = []
    for S, idx, t in ((5, 0, wb.VAL), (70, n - 1, wb.ECHO), (64, 3, wb.ECHO), (128, 2, wb.VAL)):
        root, br, blk = rnd(32), rnd(32 * wb.flat_len(n, idx)), rnd(S)
        m = wb.message(t, root, br, blk)
        bases.append((m, idx, root, br, blk, t))
        out.append((m, idx))
    for m, idx, root, br, blk, t in bases[:3]:
        hdr = wb.header_len(m)
        for at in list(range(hdr + 40)) + list(range(len(m) - 4, len(m))):  # every single-byte substitution
            out.extend((m[:at] + bytes([v]) + m[at + 1:], idx) for v in range(256) if v != m[at])
        for k in (1, 2, 3):  # the length off by a little
            out.append((m[:-k], idx))
            out.append((m + rnd(k), idx))
            out.append((m + bytes(k), idx))
        out.extend((m, j) for j in range(n) if j != idx)  # another leaf
        out.append((protocol.pb_encode(t, protocol.json_encode_val(root, br, blk)), idx))  # the JSON form
        out.append((wb.wrap(t, wb.payload(root, br, b"")), idx))  # S = 0: the host takes it, the device does not
        out.append((wb.wrap(2, wb.payload(root, br, blk)), idx))  # READY
        out.append((wb.wrap(t, wb.payload(root, br, blk) + b"\x00"), idx))  # a byte behind the shard
    for total in (130, 16387, 0, 1, 40, 50, 60):  # totals nobody has, or below the smallest message
        out.append((b"\x1a" + rnd(max(total - 1, 0)) if total else b"", 0))
    return out


def test_unmarshal_agrees_with_the_host_decoder_on_hostile_bytes(gpu):
    from cleisthenes_amd import protocol
    ca = gpu
    n = 7
    ctx = binary_ctx(ca, n, 2)
    try:
        corpus = hostile_corpus(protocol, n)
        assert len(corpus) > 30000
        ring, offs, lens = pack(ca, [m for m, _ in corpus])
        row_pitch = 128  # the S = 128 base fills its row; a 16387-byte message cannot fit
        outs = Outputs(ca, len(corpus), ctx.depth, row_pitch)
        status, types, S_out, r_out, b_out, rows = unmarshal(ca, ctx, outs, dev(ca, ring), offs, lens,
                                                              [ix for _, ix in corpus])
        assert set(np.unique(status)) == {OK, FALLBACK}
        n_ok = 0
        for i, (m, idx) in enumerate(corpus):
            want = wb.canonical(m, n, idx, row_pitch)
            # both ways: OK only for canonical bytes, and every canonical message is OK
            assert (status[i] == OK) == (want is not None), (i, len(m), idx)
            if want is None:
                assert S_out[i] == 0
                continue
            n_ok += 1
            t, pl = protocol.pb_decode(m)  # status OK: the host decoder accepts it, with the same fields
            req = protocol.bin_decode_val(pl)
            assert (t, req["RootHash"], req["Branch"], req["Block"][0]) == want, i
            blk = want[3]
            assert types[i] == t and bytes(r_out[i]) == want[1] and S_out[i] == len(blk), i
            assert bytes(rows[i, :len(blk)]) == blk and not rows[i, len(blk):rup(len(blk), 64)].any(), i
            assert (rows[i, rup(len(blk), 64):] == CANARY).all(), i
            assert bytes(b_out[i]) == wb.device_branch(n, idx, want[2]), i
        assert n_ok > 20000  # substitutions in the root are any bytes: still canonical
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# the receiver's layout
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,f", [(4, 1), (7, 2)])
def test_unmarshal_echo_places_every_message_and_follows_the_status_order(gpu, n, f):
    ca = gpu
    ctx = binary_ctx(ca, n, f)
    try:
        d, pitch = ctx.depth, 192
        bslot = max(d, 1) * 32
        rng = np.random.default_rng(77 + n)
        rnd = lambda L: rng.integers(0, 256, L, dtype=np.uint8).tobytes()  # noqa: E731
        slens = [5, 64, 65, 130]
        count = len(slens)
        roots = [rnd(32) for _ in range(count)]
        plan = []  # (bytes, inst, idx, status, fields)
        for i, S in enumerate(slens):
            leaves = [int(j) for j in rng.permutation(n)]
            mk = lambda j, t, root, s: (t, root, rnd(32 * wb.flat_len(n, j)), rnd(s))  # noqa: E731
            j = leaves[0]
            fl = mk(j, wb.ECHO, roots[i], S)
            plan.append((wb.message(*fl), i, j, OK, fl))
            j = leaves[1]
            fl = mk(j, wb.ECHO, rnd(32), S)
            plan.append((wb.message(*fl), i, j, OTHER_ROOT, None))
            j = leaves[2]
            fl = mk(j, wb.ECHO, roots[i], S + 1)
            m = wb.message(*fl)
            # decided from the length alone, before any byte: a ruined header changes nothing
            plan.append((b"\xff" * 12 + m[12:] if i % 2 else m, i, j, OTHER_LEN, None))
            j = leaves[3]
            fl = mk(j, wb.VAL if i % 2 else wb.ECHO, roots[i], S)
            m = wb.message(*fl)
            at = wb.header_len(m) + (i % 4)  # magic, version, L or the reserved byte
            plan.append((m[:at] + bytes([m[at] ^ 0x40]) + m[at + 1:], i, j, FALLBACK, None))
        # a VAL of the instance's length is placed too; a total nobody has is a fallback before any byte
        if n > 4:
            j = [x for x in range(n) if x not in [p[2] for p in plan if p[1] == 0]][0]
            fl = (wb.VAL, roots[0], rnd(32 * wb.flat_len(n, j)), rnd(slens[0]))
            plan.append((wb.message(*fl), 0, j, OK, fl))
            j2 = [x for x in range(n) if x not in [p[2] for p in plan if p[1] == 1]][0]
            z = 16387  # for every L: varint(R) grows to three bytes there
            assert all(wb.message_size(n, s, j2, t) != z for t in (0, 1) for s in range(z - 300, z))
            plan.append((b"\x1a" + rnd(z - 1), 1, j2, FALLBACK, None))
        plan = [plan[q] for q in rng.permutation(len(plan))]
        msgs = len(plan)
        ring, offs, lens = pack(ca, [p[0] for p in plan])
        inst = np.array([p[1] for p in plan], np.uint32)
        idx = np.array([p[2] for p in plan], np.uint8)
        sizes = {"shards": count * n * pitch, "branches": count * n * bslot, "present": count * n,
                 "status": msgs * 4, "types": msgs}
        out = {name: canaried(ca, size) for name, size in sizes.items()}
        ctx.dev_unmarshal_echo(None, count, msgs, dev(ca, ring), dev(ca, offs), dev(ca, lens), dev(ca, inst),
                               dev(ca, idx), dev(ca, np.frombuffer(b"".join(roots), np.uint8)),
                               dev(ca, np.array(slens, np.uint32)), 0, out["shards"], pitch, out["branches"],
                               out["present"], out["status"], out["types"])
        ca.rbc.lib.rbc_device_sync(0)
        got = {name: checked(out[name], size, name) for name, size in sizes.items()}
        status = got["status"].view(np.int32)
        shards = got["shards"].reshape(count * n, pitch)
        branches = got["branches"].reshape(count * n, bslot)
        present = got["present"]
        sent = np.zeros(count * n, bool)
        for q, (m, i, j, want, fl) in enumerate(plan):
            r = i * n + j
            sent[r] = True
            assert status[q] == want, (q, int(status[q]), want)
            if want == OK:
                S = len(fl[3])
                assert present[r] == 1 and got["types"][q] == fl[0], q
                assert bytes(shards[r, :S]) == fl[3] and not shards[r, S:rup(S, 64)].any(), q
                assert (shards[r, rup(S, 64):] == CANARY).all(), q
                assert bytes(branches[r]) == wb.device_branch(n, j, fl[2]), q
            else:
                assert present[r] == CANARY, q  # present is set only for OK
            if want == OTHER_LEN:  # the slot is fully intact
                assert (shards[r] == CANARY).all() and (branches[r] == CANARY).all(), q
        assert (shards[~sent] == CANARY).all() and (branches[~sent] == CANARY).all() and (present[~sent] == CANARY).all()
        assert set(status) == {OK, FALLBACK, OTHER_ROOT, OTHER_LEN}
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# the one-call paths: binary mode returns what JSON mode returns for the same fields
# ---------------------------------------------------------------------------
def one_call_epoch(ca, ref, n, f):
    """Nine ragged instances as fields (root, flat branches, shards) and the ECHOs received of each:
    instance 7 commits to a non-codeword, instance 8 has fewer than k ECHOs."""
    import rbc_oracle as orc
    k = n - 2 * f
    rng = np.random.default_rng(9)
    values = [rng.integers(0, 256, k * (20 + 23 * i) - i, dtype=np.uint8) for i in range(9)]
    fields, plan = [], []
    for i, v in enumerate(values):
        sh, _, _, _ = ref.encode_commit(n, f, v)
        sh = np.array(sh, np.uint8)
        if i == 7:
            sh[k + 1, 3] ^= 0x20  # altered before the Merkle build: every ECHO proves, the decode does not
        mt = orc.merkle_tree([bytes(r) for r in sh])
        brs = [orc.flat_branch(orc.merkle_branch(mt, j)) for j in range(n)]
        fields.append((mt[1], brs, [bytes(r) for r in sh]))
        senders = sorted(int(j) for j in rng.permutation(n)[:(k - 1 if i == 8 else n - f)])
        plan += [(i, j) for j in senders]
    plan = [plan[q] for q in rng.permutation(len(plan))]
    return values, fields, plan


def echoes(protocol, fields, plan, codec):
    out = []
    for i, j in plan:
        root, brs, shs = fields[i]
        out.append(wb.message(wb.ECHO, root, brs[j], shs[j]) if codec == "binary" else
                   protocol.pb_encode(protocol.ECHO, protocol.json_encode_val(root, brs[j], shs[j])))
    return out


def test_the_one_call_paths_return_what_json_mode_returns(gpu, ref):
    from cleisthenes_amd import protocol
    ca = gpu
    n, f = 7, 2
    ctx = ca.Context(n, f)
    rx = rcv = None
    try:
        k = ctx.k
        values, fields, plan = one_call_epoch(ca, ref, n, f)
        count = len(values)
        slens = [len(fl[2][0]) for fl in fields]
        assert len(set(slens)) == count  # ragged
        pitch = rup(max(slens), 64)
        roots = np.frombuffer(b"".join(fl[0] for fl in fields), np.uint8).reshape(count, 32)
        inst = np.array([i for i, _ in plan], np.uint32)
        idx = np.array([j for _, j in plan], np.uint8)
        rings = {c: echoes(protocol, fields, plan, c) for c in ("json", "binary")}
        assert sum(map(len, rings["binary"])) < 0.8 * sum(map(len, rings["json"]))
        rx = ca.WireRx(ctx, len(plan), sum(rup(len(m), 16) for m in rings["json"]), pitch)
        rcv = ca.WireReceiver(ctx, count, len(plan), sum(rup(len(m), 16) for m in rings["json"]), pitch)
        keep = ca.DeviceBuffer(len(plan) * pitch)
        got = {}
        for codec in ("json", "binary"):
            ctx.set_wire_codec(codec)
            for pinned in (True, False):
                ring, offs, lens = pack(ca, rings[codec], pinned)
                keep.upload(np.zeros(len(plan) * pitch, np.uint8))
                v = rx.validate(ring, offs, lens, idx, keep)
                v["rows"] = keep.download().reshape(len(plan), pitch)
                r = rcv.receive(ring, offs, lens, inst, idx, roots, slens)
                got[(codec, pinned)] = (v, r)
            # the other codec's ring: nothing canonical in it
            other = "binary" if codec == "json" else "json"
            ring, offs, lens = pack(ca, rings[other])
            assert (rx.validate(ring, offs, lens, idx, keep)["verdict"] == 2).all()
            # (the receiver settles "another length" on the total alone, before any byte: 2 or 3, the
            # host decoder's business either way)
            assert np.isin(rcv.receive(ring, offs, lens, inst, idx, roots, slens)["verdict"], (2, 3)).all()
        base_v, base_r = got[("json", True)]
        assert (base_v["verdict"] == 1).all() and (base_r["verdict"] == 1).all()
        assert list(base_r["status"][:7]) == [0] * 7 and base_r["status"][7] == -8 and base_r["status"][8] == -3
        for i in range(7):
            assert base_r["values"][i, :len(values[i])].tobytes() == values[i].tobytes(), i
        for q, (i, j) in enumerate(plan):
            assert bytes(base_v["rows"][q, :slens[i]]) == fields[i][2][j], q
        for key, (v, r) in got.items():
            for name in ("verdict", "types", "roots", "shard_lens", "leaves", "rows"):
                assert np.array_equal(v[name], base_v[name]), (key, name)
            for name in ("verdict", "types", "valid", "status"):
                assert np.array_equal(r[name], base_r[name]), (key, name)
            ok = base_r["status"] == 0
            assert np.array_equal(r["values"][ok], base_r["values"][ok]), key
            assert np.array_equal(r["digests"][ok], base_r["digests"][ok]), key
        # the send side: the same roots, and the bytes of the restatement
        ctx.set_wire_codec("json")
        js = ctx.shard_commit_val([v.tobytes() for v in values])
        ctx.set_wire_codec("binary")
        bn = ctx.shard_commit_val([v.tobytes() for v in values])
        assert np.array_equal(js["roots"], bn["roots"])
        for i in range(count):
            if i == 7:
                continue  # the altered instance is not what an honest commit gives
            assert bytes(bn["roots"][i]) == fields[i][0], i
            for j in range(n):
                want = wb.message(wb.VAL, fields[i][0], fields[i][1][j], fields[i][2][j])
                assert bn["lens"][i, j] == len(want) and bn["message"](i, j) == want, (i, j)
                t, pl = protocol.pb_decode(js["message"](i, j))
                req = protocol.json_decode_val(pl)
                assert (req["RootHash"], req["Branch"], req["Block"][0]) == (fields[i][0], fields[i][1][j],
                                                                            fields[i][2][j]), (i, j)
        assert bn["msgs"].shape[2] < js["msgs"].shape[2]
    finally:
        for x in (rx, rcv):
            if x is not None:
                x.close()
        ctx.close()


# ---------------------------------------------------------------------------
# the state machine
# ---------------------------------------------------------------------------
def run_nodes(ca, protocol, codecs, value):
    """One broadcast of node 0 among len(codecs) nodes; returns the nodes and every message sent."""
    n, f = len(codecs), (len(codecs) - 1) // 3
    ctx = ca.Context(n, f)
    bt = ca.Batcher(ctx, max_batch=64, max_wait_us=200)
    nodes = [protocol.Node(bt, n, f, i, 0) for i in range(n)]
    for nd, c in zip(nodes, codecs):
        nd.set_wire_codec(c)
    nodes[0].propose(value)
    sent = []
    for _ in range(200):
        moved = False
        for i, nd in enumerate(nodes):
            nd.progress(wait=True)
            for to, msg in nd.messages():
                moved = True
                sent.append((i, msg))
                for dst in (range(n) if to < 0 else [to]):
                    if dst != i:
                        nodes[dst].handle_message(i, msg)
        if not moved:
            break
    return ctx, bt, nodes, sent


def test_binary_nodes_deliver_and_emit_binary_payloads(gpu):
    from cleisthenes_amd import protocol
    ca = gpu
    value = np.random.default_rng(5).integers(0, 256, 1024, dtype=np.uint8).tobytes()
    ctx, bt, nodes, sent = run_nodes(ca, protocol, ["binary"] * 4, value)
    try:
        assert all(nd.value() == value for nd in nodes)
        kinds = set()
        for _, msg in sent:
            t, pl = protocol.pb_decode(msg)
            kinds.add(t)
            if t == protocol.READY:
                protocol.json_decode_ready(pl)  # READY keeps its JSON payload
                continue
            req = protocol.bin_decode_val(pl)
            assert pl[0] == 0xB1 and wb.parse_payload(pl) == (req["RootHash"], req["Branch"], req["Block"][0])
            assert protocol.payload_decode_val(pl) == req
        assert kinds == {protocol.VAL, protocol.ECHO, protocol.READY}
        assert all(nd.stats()["rejected"] == 0 for nd in nodes)
    finally:
        for nd in nodes:
            nd.close()
        bt.close()
        ctx.close()


def test_binary_nodes_deliver_beside_a_json_node_that_rejects_their_vals(gpu):
    from cleisthenes_amd import protocol
    ca = gpu
    value = np.random.default_rng(6).integers(0, 256, 1024, dtype=np.uint8).tobytes()
    ctx, bt, nodes, sent = run_nodes(ca, protocol, ["binary", "binary", "json", "binary"], value)
    try:
        for i in (0, 1, 3):  # n - f = 3 binary nodes carry the broadcast
            assert nodes[i].value() == value, i
        assert nodes[2].stats()["rejected"] > 0  # binary VAL / ECHO are malformed to a JSON node
    finally:
        for nd in nodes:
            nd.close()
        bt.close()
        ctx.close()


def test_a_fresh_context_speaks_json(gpu):
    ctx = gpu.Context(4, 1)
    try:
        assert ctx.wire_codec == "json"
        assert ctx.val_message_size(100, 0, 1) == gpu.rbc.lib.rbc_val_message_size(4, 100, 0, 1)
        with pytest.raises(ValueError):
            ctx.set_wire_codec("xml")
    finally:
        ctx.close()
