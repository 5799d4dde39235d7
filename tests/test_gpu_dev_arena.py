"""Every device stage with all of its buffers carved from one guarded arena
(tests/dev_arena.py): the outputs against the C oracle as elsewhere, and
arena.check() -- no byte outside the outputs changed, every const input intact.

With one allocation per buffer, a store one lane, one 16-byte chunk, one column
tile or one row past the last instance's output lands in the allocator's slack,
and inside a batch in the next instance's slot, which that instance then
repairs.  Here it lands in a guard of seeded random bytes.

* commit side: rbc_dev_encode + rbc_dev_leaves + rbc_dev_merkle_build,
  rbc_dev_shard_commit, rbc_dev_shard_commit_parity (data rows and the dense
  parity arena as two regions);
* receive side: rbc_dev_verify; rbc_dev_interpolate alone with leaves_verified
  1 (joined, value pitch round_up(k*S, 16) + 16; and the row view) and 0
  (joined, a value pitch >= k*S + 256: join_kernel on both codecs);
  rbc_dev_receive_step over three batches whose buffers are interleaved in the
  arena (cur.shards, prev.shards, next.shards, cur.branches, ...): a store into
  the other batch hits a guard or that batch's oracle check;
* the wire kernels: rbc_dev_marshal_val, rbc_dev_unmarshal_echo,
  rbc_dev_unmarshal_ready + rbc_dev_quorum under both payload codecs, against
  the same call on separate allocations (the wire tests hold their oracles).

Geometries: the five FFT ones, and (7,2), (37,12), (200,66) and (128,42) on the
matrix codec.  Shard lengths 1, 5, 63, 64, 65, 257, 763, 2049, uniform (count
5: no multiple of a block's instances, the XCD remap's remainder) and as one
ragged batch.  One packed case per Merkle mechanism (launch_rules.PACKED_CASES:
G = 8 and G = 64), and two verifies of 262144 rows (the second, a 256 MiB
arena, is the smallest batch that reaches sha_rows2_kernel).  Receiver batches mix the
patterns worst, corrupt_data, byzantine and a too-few instance, whose value and
digest keep the arena's random prefill byte for byte; a second batch is
byzantine_data_gone throughout."""
import numpy as np
import pytest

import dev_arena as da
import launch_rules as lr
import rbc_ref
import rx_cases as rc

pytestmark = pytest.mark.gpu

GEOMS = [(4, 1, "fft"), (16, 5, "fft"), (64, 21, "fft"), (128, 42, "fft"), (256, 85, "fft"),
         (7, 2, "matrix"), (37, 12, "matrix"), (200, 66, "matrix"), (128, 42, "matrix")]
GEOM_IDS = [f"n{n}-{codec}" for n, _, codec in GEOMS]
COUNT = 5
RAGGED = (2049, 1, 5, 63, 64, 65, 257, 763, 4)
LENGTHS = {f"S{S}": (S,) * COUNT for S in (1, 5, 63, 64, 65, 257, 763, 2049)}
LENGTHS["ragged"] = RAGGED


def rup(x, a):
    return (x + a - 1) // a * a


def sync(gpu):
    gpu.rbc.lib.rbc_device_sync(0)


@pytest.fixture(scope="module")
def ctxs(gpu):
    made = {}

    def get(n, f, codec):
        if (n, f, codec) not in made:
            c = gpu.Context(n, f)
            if codec == "matrix":
                c.set_codec("matrix")
            assert c.codec == codec
            made[(n, f, codec)] = c
        return made[(n, f, codec)]
    return get


# ---- the harness sees device writes ----------------------------------------------
def test_the_arena_sees_a_device_write_inside_a_guard(gpu):
    arena, at = da.make(gpu, [("a", 1000, "out"), ("b", 64, "in")], seed=3)
    assert at["a"] % 256 == 0 and at["b"] % 256 == 0
    arena.put("b", np.arange(64, dtype=np.uint8))
    assert np.array_equal(arena.get("b"), np.arange(64, dtype=np.uint8))
    gpu.rbc.check(gpu.rbc.lib.rbc_dev_memset(at["a"] + 999, 0, 1), "memset")  # the last byte of the output
    sync(gpu)
    assert arena.check()["a"][999] == 0
    spot = 1000 + 300  # inside the guard behind "a": the arena's own allocation
    value = int(arena.before[arena.regions["a"][0] + spot]) ^ 0xFF
    gpu.rbc.check(gpu.rbc.lib.rbc_dev_memset(at["a"] + spot, value, 1), "memset")
    sync(gpu)
    with pytest.raises(AssertionError, match=r"301 byte\(s\) past the end of region 'a'"):
        arena.check()
    arena, at = da.make(gpu, [("a", 1000, "out"), ("b", 64, "in")], seed=4)
    gpu.rbc.check(gpu.rbc.lib.rbc_dev_memset(at["b"] + 7, int(arena.before[arena.regions["b"][0] + 7]) ^ 1, 1), "memset")
    sync(gpu)
    with pytest.raises(AssertionError, match="'in' region 'b' changed at byte offset 7"):
        arena.check()


# ---- commit side -----------------------------------------------------------------
_commits = {}


def _commit_ref(n, f, lens):
    """Values and the oracle's commitment of one batch, built once per (n, lens)."""
    if (n, lens) not in _commits:
        k = n - 2 * f
        rng = np.random.default_rng(4100 + n + sum(lens))
        Smax = max(lens)
        vpitch = rup(k * Smax, 16) + 16
        values = rng.integers(0, 256, (len(lens), vpitch), dtype=np.uint8)  # random past B_i too: ignored
        vlens = np.array([k * S - min(3, k - 1) for S in lens], np.uint32)
        want = [rbc_ref.encode_commit(n, f, values[i, : vlens[i]]) for i in range(len(lens))]
        for S, w in zip(lens, want):
            assert w[0].shape[1] == S
        _commits[(n, lens)] = (values, vlens, vpitch, want)
    return _commits[(n, lens)]


def _check_commit(n, k, lens, spitch, want, rows, leaves, roots, branches, what):
    """rows [I][n][spitch] (for the parity form: data rows and arena rows side by side)."""
    for i, (w_sh, w_root, w_br, w_lv) in enumerate(want):
        S = lens[i]
        assert np.array_equal(rows[i, :, :S], w_sh), (what, i, np.flatnonzero((rows[i, :, :S] != w_sh).any(axis=1))[:8])
        assert not rows[i, :, S:].any(), (what, "bytes past S must be zero", i)
        assert np.array_equal(leaves[i], w_lv), (what, "leaves", i)
        assert bytes(roots[i]) == w_root, (what, "root", i)
        assert np.array_equal(branches[i], w_br), (what, "branches", i)


def _run_commit(gpu, ctx, lens, form, seed):
    n, k, p, d = ctx.n, ctx.k, ctx.p, ctx.depth
    I = len(lens)
    values, vlens, vpitch, want = _commit_ref(n, ctx.f, lens)
    ragged = len(set(lens)) > 1
    spitch = rup(max(lens), 64)
    specs = [("values", I * vpitch, "in")]
    if ragged:
        specs += [("value_lens", I * 4, "in"), ("shard_lens", I * 4, "in")]
    if form == "parity":
        specs += [("data_rows", I * k * spitch, "out"), ("parity", I * p * spitch, "out")]
    else:
        specs += [("shards", I * n * spitch, "out")]
    specs += [("leaves", I * n * 32, "out"), ("roots", I * 32, "out"), ("branches", I * n * d * 32, "out")]
    arena, at = da.make(gpu, specs, seed=seed, row_pitch=spitch)
    arena.put("values", values)
    if ragged:
        arena.put("value_lens", vlens)
        arena.put("shard_lens", np.array(lens, np.uint32))
    vl, sl = (at["value_lens"], at["shard_lens"]) if ragged else (None, None)
    ub, us = (0, 0) if ragged else (int(vlens[0]), lens[0])
    if form == "stages":
        ctx.dev_encode(None, I, at["values"], vpitch, vl, ub, at["shards"], spitch)
        ctx.dev_leaves(None, I, at["shards"], spitch, sl, us, at["leaves"])
        ctx.dev_merkle_build(None, I, at["leaves"], at["roots"], at["branches"])
    elif form == "commit":
        ctx.dev_shard_commit(None, I, at["values"], vpitch, vl, ub, at["shards"], spitch, sl, at["leaves"],
                             at["roots"], at["branches"])
    else:
        ctx.dev_shard_commit_parity(None, I, at["values"], vpitch, vl, ub, at["data_rows"], at["parity"], spitch, sl,
                                    at["leaves"], at["roots"], at["branches"])
    sync(gpu)
    out = arena.check()
    if form == "parity":
        rows = np.concatenate([out["data_rows"].reshape(I, k, spitch), out["parity"].reshape(I, p, spitch)], axis=1)
    else:
        rows = out["shards"].reshape(I, n, spitch)
    _check_commit(n, k, lens, spitch, want, rows, out["leaves"].reshape(I, n, 32), out["roots"].reshape(I, 32),
                  out["branches"].reshape(I, n, d, 32), form)


@pytest.mark.parametrize("lens", list(LENGTHS), ids=list(LENGTHS))
@pytest.mark.parametrize("n,f,codec", GEOMS, ids=GEOM_IDS)
def test_commit_stages_write_only_their_outputs(gpu, ctxs, n, f, codec, lens):
    ctx = ctxs(n, f, codec)
    for q, form in enumerate(("stages", "commit", "parity")):
        _run_commit(gpu, ctx, LENGTHS[lens], form, seed=100 * n + q)


@pytest.mark.parametrize("n,count", [(7, 4096 + 3), (4, 32768 + 37)], ids=["n7-G8", "n4-G64"])
def test_packed_commit_writes_only_its_outputs(gpu, ctxs, n, count):
    """merkle_kernel with G trees per block, the last block partly filled."""
    assert (n, count) in lr.PACKED_CASES and lr.packed_g(n, count) == (8 if n == 7 else 64)
    f = (n - 1) // 3
    ctx = ctxs(n, f, "fft" if n == 4 else "matrix")
    _run_commit(gpu, ctx, (5,) * count, "commit", seed=count)


# ---- receive side ----------------------------------------------------------------
_rx = {}


def _rx_cases(n, f, lens_id):
    """Two batches per (geometry, lengths): worst + corrupt_data + byzantine (a
    random commitment and a codeword with an altered parity row) + too few; and
    byzantine_data_gone throughout."""
    if (n, lens_id) not in _rx:
        lens = LENGTHS[lens_id]
        kw = dict(lens=lens) if lens_id == "ragged" else {}
        S, count = (None, None) if lens_id == "ragged" else (lens[0], COUNT)
        seed = 5200 + 31 * n + sum(lens)
        mixed = rc.Case(n, f, S, count, "worst", seed, corrupt={0}, byz={1, 2}, too_few={3}, **kw)
        gone = rc.Case(n, f, S, count, "byzantine_data_gone", seed + 1, **kw)
        assert sorted(set(mixed.want_status)) == [-8, -3, 0] and (gone.want_status == -8).all()
        _rx[(n, lens_id)] = (mixed, gone)
    return _rx[(n, lens_id)]


def _held_leaves(case):
    """SHA-256 of every received row as the receiver holds it: what rbc_dev_verify leaves."""
    if not hasattr(case, "_held_leaves"):
        held = case.receiver_rows()
        out = np.zeros((case.count, case.n, 32), np.uint8)
        for i, j in zip(*np.nonzero(case.present)):
            out[i, j] = np.frombuffer(rbc_ref.sha256(held[i, j, : case.lens[i]]), np.uint8)
        case._held_leaves = out
    return case._held_leaves


def _wide_vpitch(case):
    return rup(case.k * case.S + 256, 16)  # too wide a tail for the fused join: join_kernel on the FFT codec too


def _verify_alone(gpu, ctx, case, seed):
    kinds = dict(shards="in", values="in", digests="in", status="in")
    arena, _ = da.make(gpu, da.rx_specs(case, kinds=kinds), seed=seed, row_pitch=case.spitch)
    dev = da.RxRegions(arena, case)
    dev.verify(ctx)
    sync(gpu)
    out = arena.check()
    got_valid = out["valid"].reshape(case.count, case.n)
    assert np.array_equal(got_valid, case.want_valid)
    rec = case.present == 1
    assert np.array_equal(out["leaves"].reshape(case.count, case.n, 32)[rec], _held_leaves(case)[rec])


def _interpolate_alone(gpu, ctx, case, seed, leaves_verified, joined, vpitch=None):
    kinds = dict(valid="in", leaves="inout")
    if not joined:
        kinds["values"] = "in"  # the row view writes no value
    arena, _ = da.make(gpu, da.rx_specs(case, vpitch=vpitch, kinds=kinds), seed=seed, row_pitch=case.spitch)
    dev = da.RxRegions(arena, case, vpitch=vpitch)
    arena.put("valid", case.want_valid)
    leaves = arena.prefill("leaves").reshape(case.count, case.n, 32)
    # verify's leaves of the valid rows; an instance with too few shards is
    # skipped after the prepare, so its received rows' leaves are the caller's
    keep = (case.want_valid == 1) if leaves_verified else np.zeros_like(case.present, bool)
    for i in case.too_few:
        keep[i] = case.present[i] == 1
    leaves[keep] = _held_leaves(case)[keep]
    arena.put("leaves", leaves)
    dev.interpolate(ctx, joined=joined, leaves_verified=leaves_verified)
    sync(gpu)
    got = dev.read({**arena.check(), "valid": case.want_valid.reshape(-1),
                    **({} if joined else {"values": arena.prefill("values")})})
    rc.check_against_oracle(case, got, joined=joined, prefill=dev.prefill())


@pytest.mark.parametrize("lens", list(LENGTHS), ids=list(LENGTHS))
@pytest.mark.parametrize("n,f,codec", GEOMS, ids=GEOM_IDS)
def test_verify_and_interpolate_write_only_their_outputs(gpu, ctxs, n, f, codec, lens):
    ctx = ctxs(n, f, codec)
    for q, case in enumerate(_rx_cases(n, f, lens)):
        seed = 1000 * n + 10 * q
        _verify_alone(gpu, ctx, case, seed)
        _interpolate_alone(gpu, ctx, case, seed + 1, leaves_verified=1, joined=True)
        _interpolate_alone(gpu, ctx, case, seed + 2, leaves_verified=0, joined=True, vpitch=_wide_vpitch(case))
        _interpolate_alone(gpu, ctx, case, seed + 3, leaves_verified=1, joined=False)


def _step_three_batches(gpu, ctx, cases, vpitches, seed):
    tags = ("a.", "b.", "c.")
    specs = da.interleave(*(da.rx_specs(c, tag=t, vpitch=v) for c, t, v in zip(cases, tags, vpitches)))
    arena, _ = da.make(gpu, specs, seed=seed, row_pitch=max(c.spitch for c in cases))
    names = list(arena.regions)
    assert names[:6] == ["a.shards", "b.shards", "c.shards", "a.branches", "b.branches", "c.branches"]
    devs = [da.RxRegions(arena, c, tag=t, vpitch=v) for c, t, v in zip(cases, tags, vpitches)]
    bs = [d.rx_batch(ctx) for d in devs]
    ctx.dev_receive_step(None, bs[0], None)
    ctx.dev_receive_step(None, bs[1], bs[0])
    ctx.dev_receive_step(None, bs[2], bs[1])
    ctx.dev_receive_step(None, None, bs[2])
    sync(gpu)
    out = arena.check()
    for c, d in zip(cases, devs):
        rc.check_against_oracle(c, d.read(out), prefill=d.prefill())


@pytest.mark.parametrize("lens", list(LENGTHS), ids=list(LENGTHS))
@pytest.mark.parametrize("n,f,codec", GEOMS, ids=GEOM_IDS)
def test_receive_step_rotation_writes_only_its_own_batches(gpu, ctxs, n, f, codec, lens):
    mixed, gone = _rx_cases(n, f, lens)
    _step_three_batches(gpu, ctxs(n, f, codec), (mixed, gone, mixed),
                        (mixed.vpitch, _wide_vpitch(gone), mixed.vpitch), seed=7000 + n)


_packed = {}


@pytest.mark.parametrize("n,count", [(7, 4096 + 3), (4, 32768 + 37)], ids=["n7-G8", "n4-G64"])
def test_packed_recheck_in_the_receive_step(gpu, ctxs, n, count):
    """merkle_recheck_kernel (and the verify / decode of a batch of thousands)
    with G instances per block, the last block partly filled."""
    assert (n, count) in lr.PACKED_CASES and lr.packed_g(n, count) == (8 if n == 7 else 64)
    f = (n - 1) // 3
    if n not in _packed:
        _packed[n] = rc.Case(n, f, 5, count, "worst", 8800 + n, corrupt={0, count - 1}, byz={1, 2, count - 2},
                             too_few={3, count - 3})
    case = _packed[n]
    ctx = ctxs(n, f, "fft" if n == 4 else "matrix")
    arena, _ = da.make(gpu, da.rx_specs(case), seed=count, row_pitch=case.spitch)
    dev = da.RxRegions(arena, case)
    b = dev.rx_batch(ctx)
    ctx.dev_receive_step(None, b, None)
    ctx.dev_receive_step(None, None, b)
    sync(gpu)
    rc.check_against_oracle(case, dev.read(arena.check()), prefill=dev.prefill())


@pytest.mark.parametrize("n,f,S,form", [(64, 21, 187, "shared_path"), (2, 0, 1021, "walk")], ids=["n64-S187", "n2-S1021"])
def test_verify_of_262144_rows_writes_only_valid_and_leaves(gpu, n, f, S, form):
    """count * n = 4 * 64 * 1024 rows, every ECHO received (present = NULL): the
    grid size from which rbc_launch_sha_rows hands a per-leaf-walk verify to
    sha_rows2_kernel, two rows per lane.  At (64,21), S = 187, rows this short
    take the shared-path form (sha_rows_kernel + merkle_path_kernel; the walk
    form needs rows of 6136 bytes at depth 6, 1.6 GB of them).  The smallest
    batch that does reach sha_rows2_kernel is (2,0) with rows of 17 SHA blocks:
    S = 1021, 131072 instances, a 256 MiB arena.  One row of every other
    instance is corrupted."""
    count = 4 * 64 * 1024 // n
    ctx = gpu.Context(n, f)
    assert ctx.verify_form(S) == form and ctx.depth >= 1 and n % 2 == 0
    base = rc.Case(n, f, S, 8, "none", 9900 + n)
    rng = np.random.default_rng(9901)
    pick = rng.integers(0, 8, count)
    rows = np.zeros((count, n, base.spitch), np.uint8)
    rows[:, :, :S] = base.rows_in[pick]
    bad = rng.integers(0, n, count)
    hit = np.arange(0, count, 2)
    rows[hit, bad[hit], rng.integers(0, S, len(hit))] ^= 0x10
    specs = [("shards", rows.nbytes, "in"), ("branches", count * n * base.depth * 32, "in"), ("roots", count * 32, "in"),
             ("valid", count * n, "out"), ("leaves", count * n * 32, "out")]
    arena, at = da.make(gpu, specs, seed=99, row_pitch=base.spitch)
    arena.put("shards", rows)
    arena.put("branches", base.branches[pick])
    arena.put("roots", base.roots[pick])
    ctx.dev_verify(None, count, at["shards"], base.spitch, None, S, at["branches"], at["roots"], None, at["valid"],
                   at["leaves"])
    sync(gpu)
    out = arena.check()
    want_valid = np.ones((count, n), np.uint8)
    want_valid[hit, bad[hit]] = 0
    assert np.array_equal(out["valid"].reshape(count, n), want_valid)
    leaves = out["leaves"].reshape(count, n, 32)
    good = want_valid == 1
    assert np.array_equal(leaves[good], base.want_leaves()[pick][good])
    for i in rng.permutation(hit)[:64]:
        assert bytes(leaves[i, bad[i]]) == rbc_ref.sha256(rows[i, bad[i], :S]), i


# ---- the wire kernels ------------------------------------------------------------
# Their bytes are pinned by the wire tests; here each call runs on regions of one
# arena and on separate allocations with the same contents, and must leave the
# same bytes in every output, the guards and the inputs intact.
WIRE_CODECS = ("json", "binary")
WIRE_OK, WIRE_FALLBACK, WIRE_OTHER_ROOT, WIRE_OTHER_LEN = 0, 1, 2, 3


@pytest.fixture(scope="module")
def wire_ctxs(gpu):
    made = {}

    def get(n, f, codec):
        if (n, f) not in made:
            made[(n, f)] = gpu.Context(n, f)
        made[(n, f)].set_wire_codec(codec)
        assert made[(n, f)].wire_codec == codec
        return made[(n, f)]
    return get


def _both_ways(gpu, specs, inputs, call, seed, row_pitch=0):
    """call(addresses) on the arena's regions, then on one allocation per
    buffer holding what the region held -> (arena, the arena's outputs)."""
    arena, at = da.make(gpu, specs, seed=seed, row_pitch=row_pitch)
    for name, a in inputs.items():
        arena.put(name, a)
    call(at)
    sync(gpu)
    out = arena.check()
    bufs = {name: gpu.DeviceBuffer(max(nbytes, 16)) for name, nbytes, _ in specs}
    for name, buf in bufs.items():
        buf.upload(arena.prefill(name))
    call({name: buf.value for name, buf in bufs.items()})
    sync(gpu)
    for name, region in out.items():
        assert np.array_equal(region, bufs[name].download(len(region))), name
    return arena, out


def _ring(msgs):
    """The messages at 16-byte offsets of one ring that ends with the last one's last chunk."""
    lens = np.array([len(m) for m in msgs], np.uint32)
    steps = [rup(max(len(m), 1), 16) for m in msgs]
    offs = np.concatenate(([0], np.cumsum(steps)[:-1])).astype(np.uint64)
    ring = np.zeros(sum(steps), np.uint8)
    for m, o in zip(msgs, offs):
        ring[int(o): int(o) + len(m)] = np.frombuffer(m, np.uint8)
    return ring, offs, lens


def _val_message(protocol, codec, msg_type, root, branch, block):
    enc = protocol.json_encode_val if codec == "json" else protocol.bin_encode_val
    return protocol.pb_encode(msg_type, enc(root, branch, block))


WIRE_LENS = (1, 5, 63, 64, 65, 257)


@pytest.mark.parametrize("msg_type", [0, 1], ids=["val", "echo"])
@pytest.mark.parametrize("codec", WIRE_CODECS)
@pytest.mark.parametrize("n,f", [(7, 2), (16, 5)])
def test_marshal_val_writes_only_its_messages(gpu, wire_ctxs, n, f, codec, msg_type):
    import wire_bin as wb
    from cleisthenes_amd import protocol
    ctx = wire_ctxs(n, f, codec)
    d = ctx.depth
    rng = np.random.default_rng(300 + n + msg_type)
    slens = np.array(WIRE_LENS, np.uint32)
    count, pitch = len(slens), rup(int(slens.max()), 64)
    sh = rng.integers(0, 256, (count, n, pitch), dtype=np.uint8)  # dirty pads: only S_i bytes are the shard
    br = rng.integers(0, 256, (count, n, d, 32), dtype=np.uint8)
    roots = rng.integers(0, 256, (count, 32), dtype=np.uint8)
    out_pitch = rup(max(ctx.val_message_size(int(slens.max()), j, msg_type) for j in (0, n - 1)), 16)
    msgs = count * n
    specs = [("shards", sh.nbytes, "in"), ("shard_lens", count * 4, "in"), ("branches", br.nbytes, "in"),
             ("roots", roots.nbytes, "in"), ("out", msgs * out_pitch, "out"), ("out_lens", msgs * 4, "out")]

    def call(at):
        ctx.dev_marshal_val(None, count, msg_type, at["shards"], pitch, at["shard_lens"], 0, at["branches"],
                            at["roots"], at["out"], out_pitch, at["out_lens"])
    arena, out = _both_ways(gpu, specs, dict(shards=sh, shard_lens=slens, branches=br, roots=roots), call,
                            seed=n + msg_type, row_pitch=out_pitch)
    got, mlens = out["out"].reshape(msgs, out_pitch), out["out_lens"].view(np.uint32)
    before = arena.prefill("out").reshape(msgs, out_pitch)
    for i in range(count):
        for j in range(n):
            flat = b"".join(bytes(br[i, j, lv]) for lv in range(d) if not (lv == 0 and (j ^ 1) >= n))
            assert len(flat) == 32 * wb.flat_len(n, j)
            want = _val_message(protocol, codec, msg_type, bytes(roots[i]), flat, bytes(sh[i, j, : slens[i]]))
            q = i * n + j
            assert mlens[q] == len(want) and bytes(got[q, : len(want)]) == want, (i, j)
            end = rup(len(want), 16)  # zeroed up to the next 16 bytes, nothing behind
            assert not got[q, len(want): end].any() and np.array_equal(got[q, end:], before[q, end:]), (i, j)


def _unmarshal_echo(gpu, wire_ctxs, n, f, codec):
    """Per instance one message of another length, one of another root and one
    non-canonical one (the wrapper's first tag, or a byte inside the payload,
    changed) beside the accepted ones, in the arena and on separate allocations.  Checks the statuses and
    every accepted slot -> [(status, slot bytes changed, present byte changed)]
    of the rejected messages."""
    import wire_bin as wb
    from cleisthenes_amd import protocol
    ctx = wire_ctxs(n, f, codec)
    d = ctx.depth
    bslot = max(d, 1) * 32
    rng = np.random.default_rng(500 + n)
    rnd = lambda L: rng.integers(0, 256, L, dtype=np.uint8).tobytes()  # noqa: E731
    slens = np.array((5, 64, 65, 257, 763), np.uint32)
    count, pitch = len(slens), 768
    roots = [rnd(32) for _ in range(count)]
    plan = []  # (bytes, instance, leaf, status, (type, flat branch, block))
    for i, S in enumerate(int(s) for s in slens):
        leaves = [int(j) for j in rng.permutation(n)]
        mk = lambda j, t, root, s: (t, root, rnd(32 * wb.flat_len(n, j)), rnd(s))  # noqa: E731
        kinds = [WIRE_OTHER_LEN, WIRE_OTHER_ROOT, WIRE_FALLBACK] + [WIRE_OK] * (n - 3)
        for j, kind in zip(leaves, kinds):
            t = protocol.VAL if (i + j) % 3 == 0 else protocol.ECHO
            fl = mk(j, t, rnd(32) if kind == WIRE_OTHER_ROOT else roots[i], S + 1 if kind == WIRE_OTHER_LEN else S)
            m = _val_message(protocol, codec, *fl)
            if kind == WIRE_FALLBACK:
                # the wrapper's first tag, or a byte the decode meets late: the first
                # character of the block's base64 run / the binary header's reserved byte
                at = 0 if i % 2 == 0 else m.index(b'"Block":["') + 10 if codec == "json" else wb.header_len(m) + 3
                m = m[:at] + (b"!" if codec == "json" and at else bytes([m[at] ^ 0x40])) + m[at + 1:]
            plan.append((m, i, j, kind, (fl[0], fl[2], fl[3])))
    plan = [plan[q] for q in rng.permutation(len(plan))]
    msgs = len(plan)
    ring, offs, lens = _ring([p[0] for p in plan])
    inst = np.array([p[1] for p in plan], np.uint32)
    idx = np.array([p[2] for p in plan], np.uint8)
    specs = [("ring", ring.nbytes, "in"), ("offs", msgs * 8, "in"), ("lens", msgs * 4, "in"), ("inst", msgs * 4, "in"),
             ("idx", msgs, "in"), ("roots", count * 32, "in"), ("shard_lens", count * 4, "in"),
             ("shards", count * n * pitch, "out"), ("branches", count * n * bslot, "out"),
             ("present", count * n, "out"), ("status", msgs * 4, "out"), ("types", msgs, "out")]

    def call(at):
        ctx.dev_unmarshal_echo(None, count, msgs, at["ring"], at["offs"], at["lens"], at["inst"], at["idx"],
                               at["roots"], at["shard_lens"], 0, at["shards"], pitch, at["branches"], at["present"],
                               at["status"], at["types"])
    inputs = dict(ring=ring, offs=offs, lens=lens, inst=inst, idx=idx, roots=np.frombuffer(b"".join(roots), np.uint8),
                  shard_lens=slens)
    arena, out = _both_ways(gpu, specs, inputs, call, seed=n, row_pitch=pitch)
    status = out["status"].view(np.int32)
    shards, b_shards = out["shards"].reshape(count * n, pitch), arena.prefill("shards").reshape(count * n, pitch)
    branches, b_branches = out["branches"].reshape(count * n, bslot), arena.prefill("branches").reshape(-1, bslot)
    present, b_present = out["present"], arena.prefill("present")
    assert [int(s) for s in status] == [p[3] for p in plan]
    assert set(status) == {WIRE_OK, WIRE_FALLBACK, WIRE_OTHER_ROOT, WIRE_OTHER_LEN}
    rejected = []
    sent = np.zeros(count * n, bool)
    for q, (m, i, j, kind, (t, flat, blk)) in enumerate(plan):
        r = i * n + j
        sent[r] = True
        if kind == WIRE_OK:
            S = len(blk)
            assert present[r] == 1 and out["types"][q] == t, q
            assert bytes(shards[r, :S]) == blk and not shards[r, S: rup(S, 64)].any(), q
            assert np.array_equal(shards[r, rup(S, 64):], b_shards[r, rup(S, 64):]), q
            assert bytes(branches[r]) == wb.device_branch(n, j, flat), q
        else:
            changed = int((shards[r] != b_shards[r]).sum() + (branches[r] != b_branches[r]).sum())
            rejected.append((kind, changed, int(present[r] != b_present[r])))
    # no slot of a leaf that sent nothing changed
    assert np.array_equal(shards[~sent], b_shards[~sent]) and np.array_equal(branches[~sent], b_branches[~sent])
    assert np.array_equal(present[~sent], b_present[~sent])
    return rejected


ECHO_GEOMS = [(4, 1), (7, 2)]


@pytest.mark.parametrize("codec", WIRE_CODECS)
@pytest.mark.parametrize("n,f", ECHO_GEOMS)
def test_unmarshal_echo_rejected_messages_keep_their_whole_slot(gpu, wire_ctxs, n, f, codec):
    """Guards, inputs and the slots of silent leaves intact; an accepted message
    fills its slot; every rejected message -- another length, another root, not
    canonical -- leaves its row, its branch slot and its present byte as they
    were (include/rbc_protocol.h, statuses 1 to 3 of rbc_dev_unmarshal_echo)."""
    rejected = _unmarshal_echo(gpu, wire_ctxs, n, f, codec)
    assert {k for k, _, _ in rejected} == {WIRE_FALLBACK, WIRE_OTHER_ROOT, WIRE_OTHER_LEN}
    assert not any(c or p for _, c, p in rejected), rejected


@pytest.mark.parametrize("codec", WIRE_CODECS)
@pytest.mark.parametrize("n,f", [(7, 2), (16, 5)])
def test_unmarshal_ready_and_quorum_write_only_their_outputs(gpu, wire_ctxs, n, f, codec):
    from cleisthenes_amd import protocol
    ctx = wire_ctxs(n, f, codec)
    rng = np.random.default_rng(700 + n)
    rnd = lambda L: rng.integers(0, 256, L, dtype=np.uint8).tobytes()  # noqa: E731
    count, self_id = 5, 2
    roots = [rnd(32) for _ in range(count)]
    plan = []  # (bytes, instance, sender, status)
    for i in range(count):
        senders = [int(j) for j in rng.permutation(n)[: (i + 1) * n // count]]
        for q, j in enumerate(senders):
            kind = (WIRE_OTHER_ROOT, WIRE_FALLBACK)[q] if q < 2 and len(senders) > 3 else WIRE_OK
            m = protocol.pb_encode(protocol.READY, protocol.json_encode_ready(rnd(32) if kind == WIRE_OTHER_ROOT
                                                                              else roots[i]))
            if kind == WIRE_FALLBACK:
                m = m[:5] + bytes([m[5] ^ 0x01]) + m[6:]
            plan.append((m, i, j, kind))
    plan = [plan[q] for q in rng.permutation(len(plan))]
    msgs = len(plan)
    ring, offs, lens = _ring([p[0] for p in plan])
    inst = np.array([p[1] for p in plan], np.uint32)
    idx = np.array([p[2] for p in plan], np.uint8)
    ready0 = (rng.integers(0, 5, (count, n)) == 0).astype(np.uint8)  # the bitmap so far: 0 and 1
    ready0[:, self_id] = 0
    valid = (rng.integers(0, 4, (count, n)) != 0).astype(np.uint8)
    valid[0] = 1
    st = np.array([0, 0, -3, -8, 0], np.int32)
    specs = [("ring", ring.nbytes, "in"), ("offs", msgs * 8, "in"), ("lens", msgs * 4, "in"), ("inst", msgs * 4, "in"),
             ("idx", msgs, "in"), ("roots", count * 32, "in"), ("ready", count * n, "inout"),
             ("msg_status", msgs * 4, "out"), ("valid", count * n, "in"), ("status", count * 4, "in"),
             ("echo_counts", count * 4, "out"), ("ready_counts", count * 4, "out"), ("flags", count, "out")]

    def call(at):
        ctx.dev_unmarshal_ready(None, count, msgs, at["ring"], at["offs"], at["lens"], at["inst"], at["idx"],
                                at["roots"], at["ready"], at["msg_status"])
        ctx.dev_quorum(None, count, at["valid"], at["ready"], at["status"], self_id, at["echo_counts"],
                       at["ready_counts"], at["flags"])
    inputs = dict(ring=ring, offs=offs, lens=lens, inst=inst, idx=idx, roots=np.frombuffer(b"".join(roots), np.uint8),
                  ready=ready0, valid=valid, status=st)
    arena, out = _both_ways(gpu, specs, inputs, call, seed=n)
    assert [int(s) for s in out["msg_status"].view(np.int32)] == [p[3] for p in plan]
    assert {p[3] for p in plan} == {WIRE_OK, WIRE_FALLBACK, WIRE_OTHER_ROOT}
    # rbc_protocol.h's rules over counts
    ready = ready0.copy()
    for m, i, j, kind in plan:
        if kind == WIRE_OK:
            ready[i, j] = 1
    E, R = valid.sum(axis=1), ready.sum(axis=1)
    have = (st == 0) & ((E >= n - f) | ((R >= 2 * f + 1) & (E >= n - 2 * f)))
    send = (R >= f + 1) | have
    flags = 1 * (E >= n - f) + 2 * (R >= f + 1) + 4 * send
    ready[send, self_id] = 1
    R = ready.sum(axis=1)
    flags += 8 * ((st == 0) & (R >= 2 * f + 1) & (E >= n - 2 * f))
    assert np.array_equal(out["ready"].reshape(count, n), ready)
    assert np.array_equal(out["echo_counts"].view(np.uint32), E) and np.array_equal(out["ready_counts"].view(np.uint32), R)
    assert np.array_equal(out["flags"], flags.astype(np.uint8))
