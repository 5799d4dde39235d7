"""GPU tests of the run-time-geometry additive-FFT codec (csrc/rs_fft_any.hip,
RBC_CODEC_FFT_GENERIC / RBC_HAS_FFT_ANY): codec selection, encode against the
oracle on ragged batches, the whole receive path against the matrix codec at
geometries that take every case of the transform's solve at every level, the
generic form against the specialised one, Byzantine non-codewords, dirty pads
with a skipped instance, and the host path.  All comparisons are bit-exact."""
import numpy as np
import pytest

import rbc_oracle  # noqa: F401  (conftest puts oracle/ on the path; test_gpu_parity imports it)
from test_gpu_parity import Pipeline, rup

pytestmark = pytest.mark.gpu

# k = 1, k = n, k = W/2 and W/2 +- 1, n = W/2 + 1, n = W and n = W - 1 at both widths W
GEOMS = [(33, 10), (33, 16), (33, 0), (48, 8), (49, 8), (47, 8), (63, 20), (64, 20), (64, 1), (63, 31),
         (65, 21), (100, 33), (100, 18), (101, 18), (99, 18), (127, 42), (128, 30), (128, 0), (127, 63)]
# The W = 256 kernel is not built (it does not fit the register file without
# scratch): there the generic form must keep being refused.
W256 = [(129, 42), (200, 66), (200, 36), (201, 36), (199, 36), (255, 84), (256, 64), (256, 1), (255, 127)]
GEOM_IDS = [f"n{n}f{f}" for n, f in GEOMS]
RX_GEOMS = [(n, f) for n, f in GEOMS if f > 0]  # k < n: there is something to receive
RX_IDS = [f"n{n}f{f}" for n, f in RX_GEOMS]

TOO_FEW, ROOT_MISMATCH = -3, -8


def generic(gpu, n, f):
    ctx = gpu.Context(n, f)
    ctx.set_codec("fft_generic")
    assert (ctx.codec, ctx.fft_form) == ("fft", "generic")
    return ctx


# ---- 1. selection ----------------------------------------------------------------
def test_codec_selection(gpu):
    ctx = gpu.Context(100, 33)
    assert (ctx.codec, ctx.fft_form) == ("matrix", "none")  # a new context is AUTO
    ctx.set_codec("fft")
    assert (ctx.codec, ctx.fft_form) == ("fft", "generic")
    ctx.set_codec("auto")
    assert (ctx.codec, ctx.fft_form) == ("matrix", "none")
    ctx.set_codec("fft_generic")
    assert (ctx.codec, ctx.fft_form) == ("fft", "generic")
    ctx.set_codec("matrix")
    assert (ctx.codec, ctx.fft_form) == ("matrix", "none")

    ctx = gpu.Context(128, 42)
    assert (ctx.codec, ctx.fft_form) == ("fft", "specialised")
    for codec, form in (("fft", "specialised"), ("fft_generic", "generic"), ("auto", "specialised")):
        ctx.set_codec(codec)
        assert (ctx.codec, ctx.fft_form) == ("fft", form), codec

    ctx = gpu.Context(20, 6)
    for codec in ("fft", "fft_generic"):
        with pytest.raises(gpu.RBCError) as ei:
            ctx.set_codec(codec)
        assert ei.value.code == -10
        assert (ctx.codec, ctx.fft_form) == ("matrix", "none")


@pytest.mark.parametrize("n,f", W256 + [(256, 85)], ids=[f"n{n}f{f}" for n, f in W256 + [(256, 85)]])
def test_generic_form_is_refused_above_128(gpu, n, f):
    ctx = gpu.Context(n, f)
    before = (ctx.codec, ctx.fft_form)
    assert before == (("fft", "specialised") if (n, f) == (256, 85) else ("matrix", "none"))
    for codec in ("fft_generic",) if (n, f) == (256, 85) else ("fft", "fft_generic"):
        with pytest.raises(gpu.RBCError) as ei:
            ctx.set_codec(codec)
        assert ei.value.code == -10
        assert (ctx.codec, ctx.fft_form) == before


# ---- 2. encode against the oracle ------------------------------------------------
SHARD_LENS = (1, 3, 61, 260, 517)  # 517: three column tiles, S % 4 == 1; 260: S % 4 == 0


@pytest.mark.parametrize("n,f", GEOMS, ids=GEOM_IDS)
def test_encode_ragged_batch_equals_the_oracle(gpu, ref, n, f):
    ctx = generic(gpu, n, f)
    k, p, d, I = ctx.k, ctx.p, ctx.depth, len(SHARD_LENS)
    spitch = rup(max(SHARD_LENS), 64)
    vpitch = rup(k * max(SHARD_LENS), 16) + 16
    rng = np.random.default_rng(5100 + 7 * n + f)
    values = rng.integers(0, 256, (I, vpitch), dtype=np.uint8)  # random past B_i too: ignored
    # B_i a little short of k * S_i: the last rows carry Split's zero pad; S = 1: whole rows are pad
    vlens = np.array([k * S - min(3, k - 1) for S in SHARD_LENS], np.uint32)
    assert all((int(B) + k - 1) // k == S for B, S in zip(vlens, SHARD_LENS)) and (k < 4 or vlens[0] < k)
    want = [ref.encode_commit(n, f, values[i, : vlens[i]]) for i in range(I)]

    mb = gpu.DeviceBuffer
    b = dict(values=mb(I * vpitch), vlens=mb(I * 4), slens=mb(I * 4), shards=mb(I * n * spitch),
             data=mb(I * k * spitch), parity=mb(max(I * p * spitch, 64)), leaves=mb(I * n * 32), roots=mb(I * 32),
             branches=mb(I * n * max(d, 1) * 32))
    b["values"].upload(values)
    b["vlens"].upload(vlens)
    b["slens"].upload(np.array(SHARD_LENS, np.uint32))
    for name in ("shards", "data", "parity"):  # nothing stale may survive
        b[name].upload(np.full(b[name].nbytes, 0xA5, np.uint8))

    ctx.dev_encode(None, I, b["values"], vpitch, b["vlens"], 0, b["shards"], spitch)
    gpu.rbc.lib.rbc_device_sync(0)
    rows = b["shards"].download().reshape(I, n, spitch)
    for i, S in enumerate(SHARD_LENS):
        bad = np.flatnonzero((rows[i, :, :S] != want[i][0]).any(axis=1))
        assert bad.size == 0, (i, S, bad[:8])
        assert not rows[i, :, S:].any(), ("bytes past S must be zero", i)

    ctx.dev_shard_commit_parity(None, I, b["values"], vpitch, b["vlens"], 0, b["data"], b["parity"], spitch,
                                b["slens"], b["leaves"], b["roots"], b["branches"])
    gpu.rbc.lib.rbc_device_sync(0)
    data = b["data"].download().reshape(I, k, spitch)
    assert np.array_equal(data, rows[:, :k])
    if p:
        parity = b["parity"].download()[: I * p * spitch].reshape(I, p, spitch)
        assert np.array_equal(parity, rows[:, k:])
    roots = b["roots"].download().reshape(I, 32)
    for i in range(I):
        assert bytes(roots[i]) == want[i][1], i


# ---- 3. the whole receive path against the matrix codec --------------------------
def _receive(gpu, n, f, B, I, codec, form, step):
    """test_fft_codec_matches_matrix_codec's scenario: random n-f present with 30 %
    corrupted ECHOs, parity first, data only, exactly k random."""
    pl = Pipeline(gpu, n, f, B, I, seed=n * 7 + B, corrupt_frac=0.3, codec=codec)
    assert pl.ctx.fft_form == form
    k = pl.k
    for i in range(I):
        if i % 4 == 1:
            pl.present[i] = 0
            pl.present[i, k:] = 1
            if n - k < k:
                pl.present[i, :k - (n - k)] = 1
        elif i % 4 == 2:
            pl.present[i] = 0
            pl.present[i, :k] = 1
            pl.corrupt[i] = -1
        elif i % 4 == 3:
            pl.present[i] = 0
            pl.present[i, np.random.default_rng(i).permutation(n)[:k]] = 1
            pl.corrupt[i] = -1
    pl.b["present"].upload(pl.present)
    pl.b["corrupt"].upload(pl.corrupt)
    pl.commit()
    enc = pl.shards().copy()
    (pl.receive_step if step else pl.receive)()
    return dict(enc=enc, dec=pl.shards(), status=pl.arr("status", np.int32).copy(),
                out=pl.arr("out", shape=(I, pl.opitch)).copy(), digests=pl.arr("digests", shape=(I, 32)).copy(),
                values=pl.values)


def _same_receive(a, b, k, B):
    S = (B + k - 1) // k
    assert np.array_equal(a["enc"], b["enc"])
    assert np.array_equal(a["status"], b["status"])
    ok = a["status"] == 0
    assert ok.sum() >= len(ok) // 2  # the data-only and exactly-k instances at least
    assert np.array_equal(a["out"][ok][:, :k * S], b["out"][ok][:, :k * S])
    assert np.array_equal(a["digests"][ok], b["digests"][ok])
    for i in np.flatnonzero(ok):
        assert b["out"][i, :B].tobytes() == b["values"][i, :B].tobytes()
    assert np.array_equal(a["dec"][ok], a["enc"][ok])  # the regenerated codeword is the encoding, in place
    assert np.array_equal(b["dec"][ok], b["enc"][ok])


@pytest.mark.parametrize("step", [False, True], ids=["receive", "receive_step"])
@pytest.mark.parametrize("n,f", RX_GEOMS, ids=RX_IDS)
def test_receive_path_equals_the_matrix_codec(gpu, n, f, step):
    k = n - 2 * f
    B = 61 * k - min(3, k - 1)
    a = _receive(gpu, n, f, B, 8, "matrix", "none", step)
    b = _receive(gpu, n, f, B, 8, "fft", "generic", step)
    _same_receive(a, b, k, B)


# ---- 4. generic against specialised ----------------------------------------------
def _noncodeword(gpu, n, f, codec, form, row, I=8):
    """test_fft_codec_rejects_noncodeword's scenario: the proposer commits to a
    tampered parity row, valid in half of the instances and absent in the others."""
    k = n - 2 * f
    pl = Pipeline(gpu, n, f, k * 61, I, seed=11, corrupt_frac=0.0, codec=codec)
    assert pl.ctx.fft_form == form
    c, b = pl.ctx, pl.b
    c.dev_encode(None, I, b["values"], pl.vpitch, None, pl.B, b["shards"], pl.spitch)
    sh = pl.shards().copy()
    sh[:, row, 5] ^= 0x21
    b["shards"].upload(sh)
    c.dev_leaves(None, I, b["shards"], pl.spitch, None, pl.S, b["leaves"])
    c.dev_merkle_build(None, I, b["leaves"], b["roots"], b["branches"])
    rng = np.random.default_rng(1)
    for i in range(I):
        pl.present[i] = 0
        pl.present[i, rng.permutation(n)[: n - f]] = 1
        pl.present[i, row] = 1 if i % 2 else 0
    b["present"].upload(pl.present)
    c.dev_verify(None, I, b["shards"], pl.spitch, None, pl.S, b["branches"], b["roots"], b["present"], b["valid"],
                 b["leaves_r"])
    c.dev_interpolate(None, I, b["shards"], pl.spitch, None, pl.S, b["valid"], b["leaves_r"], 1, b["roots"],
                      b["out"], pl.opitch, b["digests"], b["status"])
    return pl.arr("status", np.int32).copy(), pl.arr("digests", shape=(I, 32)).copy(), pl.shards()


@pytest.mark.parametrize("n,f,S", [(64, 21, 61), (64, 21, 2100), (128, 42, 61)])
def test_generic_form_equals_the_specialised_one(gpu, n, f, S):
    """S = 2100: rows long enough for the specialised decode's fused join, which
    the generic form leaves to join_kernel; the values must not differ."""
    k = n - 2 * f
    B = S * k - 3
    for step in (False, True):
        a = _receive(gpu, n, f, B, 8, "fft", "specialised", step)
        b = _receive(gpu, n, f, B, 8, "fft_generic", "generic", step)
        _same_receive(a, b, k, B)
    # a Byzantine row that verifies: the compare class, the flag and the re-hash list
    row = k + (n - k) // 2
    sa, da, ra = _noncodeword(gpu, n, f, "fft", "specialised", row)
    sb, db, rb = _noncodeword(gpu, n, f, "fft_generic", "generic", row)
    assert (sa == ROOT_MISMATCH).all() and np.array_equal(sa, sb)
    assert np.array_equal(da, db) and np.array_equal(ra, rb)


# ---- 5. non-codeword -------------------------------------------------------------
@pytest.mark.parametrize("n,f,row", [(100, 33, 80), (64, 20, 50)])  # (200, 66): refused, see above
def test_generic_form_rejects_a_noncodeword(gpu, n, f, row):
    assert row >= n - 2 * f
    status, _, _ = _noncodeword(gpu, n, f, "fft", "generic", row)
    assert (status == ROOT_MISMATCH).all()


# ---- 6. dirty pads, and an instance the transform must skip ----------------------
def test_dirty_pads_and_a_skipped_instance(gpu):
    n, f, I = 100, 33, 3
    k = n - 2 * f
    pl = Pipeline(gpu, n, f, 61 * k - 3, I, seed=77, corrupt_frac=0.0, codec="fft")
    assert pl.ctx.fft_form == "generic"
    S, sp = pl.S, pl.spitch
    rng = np.random.default_rng(78)
    pl.present[:] = 0
    pl.present[0, rng.permutation(n)[: n - f]] = 1
    pl.present[1, rng.permutation(n)[: k - 1]] = 1  # too few
    pl.present[2, rng.permutation(n)[:k]] = 1
    pl.b["present"].upload(pl.present)
    pl.commit()
    enc = pl.shards().copy()
    assert not enc[:, :, S:].any()
    pl.poison()  # the absent rows, over the whole pitch
    sh = pl.shards().copy()
    sh[:, :, S:] = rng.integers(1, 256, (I, n, sp - S), dtype=np.uint8)  # received rows carry garbage past S
    pl.b["shards"].upload(sh)
    pl.receive(poison=False)
    now, status = pl.shards(), pl.arr("status", np.int32)
    assert list(status) == [0, TOO_FEW, 0]
    assert np.array_equal(now[1], sh[1])  # untouched, pads and poison included
    out = pl.arr("out", shape=(I, pl.opitch))
    for i in (0, 2):
        assert np.array_equal(now[i, :, :S], enc[i, :, :S]), i
        gone = pl.present[i] == 0
        assert not now[i, gone, S:].any(), i  # every written row: zeros past S
        assert out[i, : pl.B].tobytes() == pl.values[i, : pl.B].tobytes()


# ---- 7. host path ----------------------------------------------------------------
def test_host_commit_and_receive_round_trip(gpu, ref):
    n, f = 100, 33
    ctx = generic(gpu, n, f)
    k = ctx.k
    rng = np.random.default_rng(79)
    values = [rng.integers(0, 256, L, dtype=np.uint8) for L in (1, 61 * k - 3, 517 * k)]
    out = ctx.shard_commit_batch(values)
    for i, v in enumerate(values):
        shards, root, br, _ = ref.encode_commit(n, f, v)
        S = shards.shape[1]
        assert out["shard_lens"][i] == S
        assert np.array_equal(out["shards"][i, :, :S], shards), i
        assert bytes(out["roots"][i]) == root, i
        assert np.array_equal(out["branches"][i], br), i
    present = np.zeros((len(values), n), np.uint8)
    for i in range(len(values)):
        present[i, rng.permutation(n)[: n - f]] = 1
    res = ctx.receive_batch(out["shards"] * present[:, :, None], out["shard_lens"], present, out["branches"],
                            out["roots"])
    assert (res["status"] == 0).all()
    assert np.array_equal(res["valid"], present)
    for i, v in enumerate(values):
        S = int(out["shard_lens"][i])
        assert res["values"][i, : len(v)].tobytes() == v.tobytes()
        assert not res["values"][i, len(v): k * S].any()
