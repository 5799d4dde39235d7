"""GPU tests of the wide run-time-geometry additive-FFT codec
(csrc/rs_fft_wide.hip, RBC_CODEC_FFT_WIDE / RBC_HAS_FFT_WIDE, 129 <= N <= 256):
codec selection, encode against the oracle on ragged batches, the whole receive
path against the matrix codec at geometries that take both cases of the kernel
(k <= 128, k > 128) and the solve's cases on either coset, the wide form against
the specialised one at (256, 85), Byzantine non-codewords, dirty pads with a
skipped instance, and the host path.  All comparisons are bit-exact."""
import numpy as np
import pytest

import rbc_oracle  # noqa: F401  (conftest puts oracle/ on the path; test_gpu_parity imports it)
from test_gpu_fft_any import (ROOT_MISMATCH, SHARD_LENS, TOO_FEW, _noncodeword, _receive, _same_receive)
from test_gpu_parity import Pipeline, rup

pytestmark = pytest.mark.gpu

# k = 1; k = 127, 128 (the whole lower block known), 129 (tp = 1); the upper solve descending
# (tp = 32), at a half (tp = 64), all but two rows (tp = 126) and the whole block (k = n = 256);
# n = 129 (one row above) and n = 255, 256
GEOMS = [(129, 42), (200, 66), (255, 84), (255, 127), (199, 36), (200, 36), (256, 64), (201, 36), (131, 1),
         (200, 20), (256, 32), (256, 1), (256, 0), (256, 85)]
GEOM_IDS = [f"n{n}f{f}" for n, f in GEOMS]
RX_GEOMS = [(n, f) for n, f in GEOMS if f > 0]  # k < n: there is something to receive
RX_IDS = [f"n{n}f{f}" for n, f in RX_GEOMS]


def wide(gpu, n, f):
    ctx = gpu.Context(n, f)
    ctx.set_codec("fft_wide")
    assert (ctx.codec, ctx.fft_form) == ("fft", "wide")
    return ctx


# ---- 1. selection ----------------------------------------------------------------
@pytest.mark.parametrize("n,f", GEOMS, ids=GEOM_IDS)
def test_wide_form_is_selected_on_request_only(gpu, n, f):
    ctx = gpu.Context(n, f)
    before = (ctx.codec, ctx.fft_form)
    assert before == (("fft", "specialised") if (n, f) == (256, 85) else ("matrix", "none"))  # AUTO
    ctx.set_codec("fft_wide")
    assert (ctx.codec, ctx.fft_form) == ("fft", "wide")
    ctx.set_codec("auto")
    assert (ctx.codec, ctx.fft_form) == before
    ctx.set_codec("fft_wide")
    ctx.set_codec("matrix")
    assert (ctx.codec, ctx.fft_form) == ("matrix", "none")


@pytest.mark.parametrize("n,f", [(100, 33), (128, 42), (20, 6)])
def test_wide_form_is_refused_up_to_128(gpu, n, f):
    ctx = gpu.Context(n, f)
    for codec in ("auto", "matrix") + (("fft_generic",) if n >= 33 else ()):
        ctx.set_codec(codec)
        before = (ctx.codec, ctx.fft_form)
        with pytest.raises(gpu.RBCError) as ei:
            ctx.set_codec("fft_wide")
        assert ei.value.code == -10
        assert (ctx.codec, ctx.fft_form) == before


def test_codec_5_is_refused(gpu):
    ctx = wide(gpu, 200, 66)
    assert gpu.rbc.lib.rbc_ctx_set_codec(ctx._p, 5) == -10
    assert (ctx.codec, ctx.fft_form) == ("fft", "wide")


# ---- 2. encode against the oracle ------------------------------------------------
@pytest.mark.parametrize("n,f", GEOMS, ids=GEOM_IDS)
def test_encode_ragged_batch_equals_the_oracle(gpu, ref, n, f):
    ctx = wide(gpu, n, f)
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
@pytest.mark.parametrize("step", [False, True], ids=["receive", "receive_step"])
@pytest.mark.parametrize("n,f", RX_GEOMS, ids=RX_IDS)
def test_receive_path_equals_the_matrix_codec(gpu, n, f, step):
    k = n - 2 * f
    B = 61 * k - min(3, k - 1)
    a = _receive(gpu, n, f, B, 8, "matrix", "none", step)
    b = _receive(gpu, n, f, B, 8, "fft_wide", "wide", step)
    _same_receive(a, b, k, B)


# ---- 4. wide against specialised -------------------------------------------------
@pytest.mark.parametrize("S", [61, 2100])
def test_wide_form_equals_the_specialised_one(gpu, S):
    """S = 2100: rows long enough for the specialised decode's fused join, which
    the wide form leaves to join_kernel; the values must not differ."""
    n, f = 256, 85
    k = n - 2 * f
    B = S * k - 3
    for step in (False, True):
        a = _receive(gpu, n, f, B, 8, "fft", "specialised", step)
        b = _receive(gpu, n, f, B, 8, "fft_wide", "wide", step)
        _same_receive(a, b, k, B)


def test_wide_form_flags_the_specialised_ones_byzantine_row(gpu):
    """A Byzantine parity row that verifies: the compare class, the flag and the re-hash list."""
    n, f = 256, 85
    k = n - 2 * f
    row = k + (n - k) // 2
    sa, da, ra = _noncodeword(gpu, n, f, "fft", "specialised", row)
    sb, db, rb = _noncodeword(gpu, n, f, "fft_wide", "wide", row)
    assert (sa == ROOT_MISMATCH).all() and np.array_equal(sa, sb)
    assert np.array_equal(da, db) and np.array_equal(ra, rb)


# ---- 5. non-codeword -------------------------------------------------------------
@pytest.mark.parametrize("row", [100, 150])  # a parity row of either half
def test_wide_form_rejects_a_noncodeword(gpu, row):
    n, f = 200, 66
    assert row >= n - 2 * f
    status, _, _ = _noncodeword(gpu, n, f, "fft_wide", "wide", row)
    assert (status == ROOT_MISMATCH).all()


# ---- 6. dirty pads, and an instance the transform must skip ----------------------
def test_dirty_pads_and_a_skipped_instance(gpu):
    n, f, I = 200, 66, 3
    k = n - 2 * f
    pl = Pipeline(gpu, n, f, 61 * k - 3, I, seed=77, corrupt_frac=0.0, codec="fft_wide")
    assert pl.ctx.fft_form == "wide"
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
    n, f = 200, 66
    ctx = wide(gpu, n, f)
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
