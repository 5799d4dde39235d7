"""Parity-only shard commit on the GPU (rbc_shard_commit_parity,
rbc_dev_shard_commit_parity, rbc_shard_parity): the encoder writes the p = N-k
parity rows to a dense arena [count][p][pitch] that leaves the device in one
linear copy, the data rows stay with the caller as slices of its value
(klauspost Split / Encode, rbc/rbc.go:97-100; split_rows).

Every expected byte comes from the C oracle (oracle/rbc_ref.encode_commit),
computed once per (N, f, B); all comparisons are bit-exact."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (N, f, forced codec): the five specialised FFT geometries, an unspecialised odd
# N (matrix codec, empty level-0 sibling), and C2's geometry on the matrix codec
GEOMS = [(4, 1, "auto"), (16, 5, "auto"), (64, 21, "auto"), (128, 42, "auto"), (256, 85, "auto"),
         (37, 12, "auto"), (128, 42, "matrix")]


def rup(x, a):
    return (x + a - 1) // a * a


def ragged_lens(k):
    """S = 1 with all data rows but the first pure pad; k and k + 1; S = 601
    (not a multiple of 4, three 256-B column tiles); k KiB."""
    return [1, k, k + 1, k * 600 + 7, k * 1024]


@functools.lru_cache(maxsize=None)
def _value(n, f, B):
    rng = np.random.default_rng([20261019, n, f, B])
    v = rng.integers(0, 256, B, dtype=np.uint8)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _oracle(n, f, B):
    import rbc_ref
    shards, root, br, leaves = rbc_ref.encode_commit(n, f, _value(n, f, B))
    for a in (shards, br, leaves):
        a.setflags(write=False)
    return shards, root, br, leaves


def _ctx(gpu, n, f, codec="auto"):
    ctx = gpu.Context(n, f)
    ctx.set_codec(codec)
    assert ctx.codec == ("fft" if codec == "auto" and n != 37 and n != 7 else "matrix")
    return ctx


def _check_batch(ctx, n, f, lens, out, key="parity", first=None):
    """out of shard_commit_parity_* (or, key "shards" and first 0, shard_commit_*): the rows
    `first` .. n-1, lengths, roots and branches against the oracle."""
    first = ctx.k if first is None else first
    for i, B in enumerate(lens):
        shards, root, br, _ = _oracle(n, f, B)
        S = shards.shape[1]
        assert out["shard_lens"][i] == S
        assert np.array_equal(out[key][i, :, :S], shards[first:]), (n, f, B)
        assert bytes(out["roots"][i]) == root, (n, f, B)
        assert np.array_equal(out["branches"][i], br), (n, f, B)


# ---- 1. bit-exact parity, roots and branches


@pytest.mark.parametrize("n,f,codec", GEOMS, ids=[f"{n}-{f}-{c}" for n, f, c in GEOMS])
def test_parity_rows_roots_and_branches_equal_the_oracle(gpu, n, f, codec):
    ctx = _ctx(gpu, n, f, codec)
    lens = ragged_lens(ctx.k)  # 5 instances: the tile total is no multiple of 8 (the XCD remap's remainder)
    values = [_value(n, f, B) for B in lens]
    out = ctx.shard_commit_parity_batch(values)
    assert out["parity"].shape == (5, ctx.p, (max(lens) + ctx.k - 1) // ctx.k)
    _check_batch(ctx, n, f, lens, out)
    for i, B in enumerate(lens):  # pageable output: Smax bytes per row, zero past S_i
        assert not out["parity"][i, :, (B + ctx.k - 1) // ctx.k:].any()
    full = ctx.shard_commit_batch(values)
    assert np.array_equal(out["roots"], full["roots"])
    assert np.array_equal(out["branches"], full["branches"])
    assert np.array_equal(out["shard_lens"], full["shard_lens"])
    assert np.array_equal(out["parity"], full["shards"][:, ctx.k:])


# ---- 2. the three output forms


# both commits share one output plan: the parity-only one keeps its case names
FORM_CASES = [(entry, n, f, form) for entry in ("parity", "shards") for n, f in [(128, 42), (37, 12)]
              for form in ["pinned_flat", "pinned_odd_pitch", "pageable"]]


@pytest.mark.parametrize("entry,n,f,form", FORM_CASES,
                         ids=[("" if e == "parity" else "full-") + f"{n}-{f}-{form}" for e, n, f, form in FORM_CASES])
def test_output_forms_and_nothing_written_past_the_output(gpu, entry, n, f, form):
    ctx = _ctx(gpu, n, f)
    k, d = ctx.k, ctx.depth
    rows, first = (ctx.p, k) if entry == "parity" else (n, 0)  # the rows handed back: shards first .. n-1
    lens = ragged_lens(k)
    count, Smax = len(lens), max((B + k - 1) // k for B in lens)
    pitch = {"pinned_flat": rup(Smax, 64), "pinned_odd_pitch": Smax + 3, "pageable": Smax}[form]
    alloc = (lambda shape: np.empty(shape, np.uint8)) if form == "pageable" else gpu.pinned_empty
    raw = alloc(count * rows * pitch + 64)
    raw[:] = 0xA5
    out = {entry: raw[: count * rows * pitch].reshape(count, rows, pitch), "roots": alloc((count, 32)),
           "branches": alloc((count, n, d, 32))}
    submit = ctx.shard_commit_parity_submit if entry == "parity" else ctx.shard_commit_submit
    res = submit([_value(n, f, B) for B in lens], out=out).wait()
    _check_batch(ctx, n, f, lens, res, entry, first)
    assert (raw[count * rows * pitch:] == 0xA5).all(), "sentinel after the output overwritten"
    got = out[entry]
    for i, B in enumerate(lens):
        S = (B + k - 1) // k
        if form == "pinned_flat":  # ONE linear copy: whole rows, bytes [S_i, pitch) zero
            assert not got[i, :, S:].any()
        else:  # Smax bytes per row (zero past S_i); the bytes of the pitch beyond Smax are not touched
            assert not got[i, :, S:Smax].any()
            assert (got[i, :, Smax:] == 0xA5).all()
        if entry == "parity" and S >= 16:  # data rows appear nowhere in the output
            data = {bytes(r) for r in _oracle(n, f, B)[0][:k]}
            assert not any(bytes(got[i, r, :S]) in data for r in range(rows))


# ---- 3. reassembly and round trip


@pytest.mark.parametrize("n,f", [(4, 1), (128, 42), (37, 12), (7, 1)])  # (7, 1): k = 5 > p = 2
def test_split_rows_plus_parity_reassemble_every_shard(gpu, n, f):
    ctx = _ctx(gpu, n, f)
    k, p = ctx.k, ctx.p
    B = k * 600 + 7
    value = _value(n, f, B)
    par = ctx.shard_commit_parity_batch([value])
    full = ctx.shard_commit_batch([value])
    S = int(par["shard_lens"][0])
    rows = ctx.split_rows(value)
    assert len(rows) == k and sum(np.shares_memory(r, value) for r in rows) == B // S
    shards = [np.array(r) for r in rows] + [par["parity"][0, r, :S] for r in range(p)]
    assert all(np.array_equal(shards[j], full["shards"][0, j, :S]) for j in range(n))
    assert all(np.array_equal(shards[j], _oracle(n, f, B)[0][j]) for j in range(n))
    root = bytes(par["roots"][0])
    for j in range(n):
        flat = b"".join(bytes(par["branches"][0, j, lvl]) for lvl in range(ctx.depth)
                        if not (lvl == 0 and (j ^ 1) >= n))
        assert ctx.validate_message(root, flat, shards[j], j), j
    # interpolate from the parity rows alone, or (p < k) the parity rows plus the last k - p data rows
    given = [None] * n
    for j in list(range(k, n)) + list(range(k - max(k - p, 0), k)):
        given[j] = shards[j]
    assert sum(g is not None for g in given) == max(p, k)
    got = ctx.interpolate(root, given)["value"]
    assert got[:B] == value.tobytes() and not any(got[B:]) and len(got) == k * S


# ---- 4. device form


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "per_instance"])
@pytest.mark.parametrize("n,f", [(4, 1), (128, 42)])
def test_device_form_data_rows_arena_and_leaves(gpu, n, f, uniform):
    ctx = _ctx(gpu, n, f)
    k, p, d = ctx.k, ctx.p, ctx.depth
    # uniform: three different values of one length; else the lengths differ too
    lens = [k * 600 + 7] * 3 if uniform else [k + 1, k * 600 + 7, 1]
    vals = [_value(n, f, B) for B in lens] if not uniform else [
        np.roll(_value(n, f, lens[0]), s) for s in (0, 1, 2)]
    I = len(lens)
    Ss = [(B + k - 1) // k for B in lens]
    pitch, vpitch = rup(max(Ss), 64), rup(k * max(Ss) + 32, 64)
    hv = np.zeros((I, vpitch), np.uint8)
    for i, v in enumerate(vals):
        hv[i, : len(v)] = v
        hv[i, len(v):] = 0x3C  # bytes past B_i are ignored (the Split pad is produced by masking)
    mb = gpu.DeviceBuffer
    b = dict(values=mb(hv.nbytes), data=mb(I * k * pitch), arena=mb(I * p * pitch), leaves=mb(I * n * 32),
             roots=mb(I * 32), branches=mb(I * n * d * 32), vlens=mb(I * 4), slens=mb(I * 4))
    b["values"].upload(hv)
    for name in ("data", "arena"):  # every byte of both buffers must be written (zero past S_i)
        b[name].upload(np.full(b[name].nbytes, 0xCC, np.uint8))
    b["vlens"].upload(np.array(lens, np.uint32))
    b["slens"].upload(np.array(Ss, np.uint32))
    ctx.dev_shard_commit_parity(None, I, b["values"], vpitch, None if uniform else b["vlens"],
                                lens[0] if uniform else 0, b["data"], b["arena"], pitch,
                                None if uniform else b["slens"], b["leaves"], b["roots"], b["branches"])
    gpu.rbc.lib.rbc_device_sync(0)
    data = b["data"].download().reshape(I, k, pitch)
    arena = b["arena"].download().reshape(I, p, pitch)
    leaves = b["leaves"].download().reshape(I, n, 32)
    roots = b["roots"].download().reshape(I, 32)
    branches = b["branches"].download().reshape(I, n, d, 32)
    import rbc_ref
    for i, v in enumerate(vals):
        shards, root, br, lv = _oracle(n, f, lens[i]) if not uniform or i == 0 else rbc_ref.encode_commit(n, f, v)
        S = Ss[i]
        assert np.array_equal(data[i, :, :S], shards[:k]) and not data[i, :, S:].any(), i
        assert np.array_equal(arena[i, :, :S], shards[k:]) and not arena[i, :, S:].any(), i
        assert np.array_equal(leaves[i], lv), i
        assert bytes(roots[i]) == root and np.array_equal(branches[i], br), i


# ---- 5. the one-call form


@pytest.mark.parametrize("B", [1024, 1])
def test_shard_parity_one_call_form(gpu, B):
    n, f = 4, 1
    ctx = _ctx(gpu, n, f)
    value = _value(n, f, B)
    shards, root, br, _ = _oracle(n, f, B)
    got = ctx.shard_parity(value)
    want = ctx.shard(value)
    assert got["shard_len"] == shards.shape[1] == want["shard_len"]
    assert len(got["parity"]) == ctx.p
    assert all(np.array_equal(got["parity"][r], shards[ctx.k + r]) for r in range(ctx.p))
    assert got["root"] == root == want["root"]
    assert got["branches"] == want["branches"]
    assert got["branches"] == [b"".join(bytes(br[j, lvl]) for lvl in range(ctx.depth)) for j in range(n)]
