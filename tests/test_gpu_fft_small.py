"""GPU tests of the small run-time-geometry additive-FFT codec
(csrc/rs_fft_small.hip, RBC_CODEC_FFT_SMALL / RBC_HAS_FFT_SMALL, 2 <= N <= 32):
codec and lane selection, encode against the oracle on ragged batches, the whole
receive path against the matrix codec at every case of the solve at every width,
the small form against the specialised one at (4, 1) and (16, 5), Byzantine
non-codewords, dirty pads with a skipped instance, every stage inside a guarded
arena with the value ending at its pitch, and the host path.  Every test that
reaches the kernel runs at lane 1 and at the wider lane built for its width.
All comparisons are bit-exact."""
import numpy as np
import pytest

import dev_arena as da
import fft_small_model as fsm
import rbc_oracle  # noqa: F401  (conftest puts oracle/ on the path; test_gpu_parity imports it)
import rx_cases as rc
from test_gpu_fft_any import ROOT_MISMATCH, TOO_FEW, _noncodeword, _receive, _same_receive
from test_gpu_parity import Pipeline, rup

pytestmark = pytest.mark.gpu

# every solve case at every width, as (n, f), k = n - 2f:
# W = 8:  k = 1 (n < W/2); k = 3 = W/2 - 1 at n = W/2 + 1 and at the BFT-maximal 7; k = 5 = W/2 + 1; k = 4 = W/2,
#         k = 6 and k = n = W at n = W
W8 = [(3, 1), (5, 1), (7, 2), (7, 1), (8, 2), (8, 1), (8, 0)]
# W = 16: k = 5 at n = W/2 + 1; the BFT-maximal 10 (k = 4) and 13 (k = 5); k = 1; k = 9 = W/2 + 1; k = 7 = W/2 - 1;
#         k = W/2 and k = n = W at n = W
W16 = [(9, 2), (10, 3), (13, 4), (13, 6), (15, 3), (15, 4), (16, 4), (16, 0)]
# W = 32: n = W/2 + 1 at k = 7 and at k = n; the BFT-maximal 19 (k = 7), 25 (9) and 31 (11); k = 8, one compare
#         group; k = 17 = W/2 + 1, 15 = W/2 - 1 and 1 at n = 31; k = 12, W/2 and n at n = W
W32 = [(17, 5), (17, 0), (19, 6), (20, 6), (25, 8), (31, 10), (31, 7), (31, 8), (31, 15), (32, 10), (32, 8), (32, 0)]
SPECIAL = [(4, 1), (16, 5)]  # the geometries with a specialised transform
GEOMS = W8 + W16 + W32 + SPECIAL
assert all(1 << fsm.width_log2(n) == w for w, gs in ((8, W8), (16, W16), (32, W32)) for n, _ in gs)

# tiles of both lane widths (256 B, 512 B and 1 KiB a wave), S % 4 and S % 16 non-zero, a last tile that holds
# a single dword (260, 1028: one dword past one tile of lane 1 and of lane 4; 517: one past two tiles of lane 1,
# one past one tile of lane 2), the longest last
SHARD_LENS = (1, 3, 13, 61, 260, 517, 1028, 2053)


def _cases(geoms):
    """(n, f, lane) for lane 1 and the wider lane of n's width."""
    return [(n, f, lane) for n, f in geoms for lane in fsm.lane_widths(n)]


def _ids(cases):
    return [f"n{n}f{f}-lane{lane}" for n, f, lane in cases]


ALL = _cases(GEOMS)
RX = _cases([(n, f) for n, f in GEOMS if f > 0])  # k < n: there is something to receive


def small(gpu, n, f, lane):
    ctx = gpu.Context(n, f)
    ctx.set_codec("fft_small")
    ctx.set_fft_lane(lane)
    assert (ctx.codec, ctx.fft_form, ctx.fft_lane) == ("fft", "small", lane)
    return ctx


class Laned:
    """The package with contexts created at a lane width: the helpers shared with the other FFT
    tests make their own contexts.  The setting has no effect on any form but the small one."""

    def __init__(self, gpu, lane):
        self._gpu, self._lane = gpu, lane

    def __getattr__(self, name):
        return getattr(self._gpu, name)

    def Context(self, n, f, **kw):
        ctx = self._gpu.Context(n, f, **kw)
        ctx.set_fft_lane(self._lane)
        return ctx


# ---- 1. selection ----------------------------------------------------------------
def test_small_form_is_selected_on_request_only(gpu):
    for n, f in GEOMS:
        ctx = gpu.Context(n, f)
        before = (ctx.codec, ctx.fft_form)
        assert before == (("fft", "specialised") if (n, f) in SPECIAL else ("matrix", "none"))  # AUTO
        ctx.set_codec("fft_small")
        assert (ctx.codec, ctx.fft_form) == ("fft", "small"), (n, f)
        ctx.set_codec("auto")
        assert (ctx.codec, ctx.fft_form) == before
        ctx.set_codec("matrix")
        ctx.set_codec("fft_small")
        assert (ctx.codec, ctx.fft_form) == ("fft", "small")
        ctx.set_codec("matrix")
        assert (ctx.codec, ctx.fft_form) == ("matrix", "none")
    ctx = gpu.Context(16, 5)
    ctx.set_codec("fft")
    assert (ctx.codec, ctx.fft_form) == ("fft", "specialised")
    ctx.set_codec("fft_small")
    assert (ctx.codec, ctx.fft_form) == ("fft", "small")
    ctx.set_codec("fft")  # FFT keeps meaning the specialised transform there
    assert (ctx.codec, ctx.fft_form) == ("fft", "specialised")


def test_small_form_is_refused_above_32_and_the_others_below(gpu):
    for n, f, others in [(33, 10, ("auto", "matrix", "fft_generic")), (100, 33, ("auto", "matrix", "fft")),
                         (200, 66, ("auto", "matrix", "fft_wide"))]:
        ctx = gpu.Context(n, f)
        for codec in others:
            ctx.set_codec(codec)
            before = (ctx.codec, ctx.fft_form)
            with pytest.raises(gpu.RBCError) as ei:
                ctx.set_codec("fft_small")
            assert ei.value.code == -10
            assert (ctx.codec, ctx.fft_form) == before
    ctx = gpu.Context(20, 6)
    for start in ("auto", "fft_small"):
        ctx.set_codec(start)
        before = (ctx.codec, ctx.fft_form)
        for codec in ("fft", "fft_generic", "fft_wide"):
            with pytest.raises(gpu.RBCError) as ei:
                ctx.set_codec(codec)
            assert ei.value.code == -10
            assert (ctx.codec, ctx.fft_form) == before
        assert gpu.rbc.lib.rbc_ctx_set_codec(ctx._p, 5) == -10  # unassigned
        assert (ctx.codec, ctx.fft_form) == before


def test_lane_values_outside_the_built_set_are_refused(gpu):
    for n, f, built in [(7, 2, (0, 1, 4)), (16, 5, (0, 1, 4)), (17, 5, (0, 1, 2)), (32, 10, (0, 1, 2)),
                        (100, 33, (0, 1))]:
        ctx = gpu.Context(n, f)
        assert ctx.fft_lane == 0  # automatic
        for lane in built:
            ctx.set_fft_lane(lane)
            assert ctx.fft_lane == lane
            for bad in (-1, 2, 3, 4, 5, 8, 16):
                if bad in built:
                    continue
                with pytest.raises(gpu.RBCError) as ei:
                    ctx.set_fft_lane(bad)
                assert ei.value.code == -10
                assert ctx.fft_lane == lane
        assert (ctx.codec, ctx.fft_form) == (("fft", "specialised") if (n, f) == (16, 5) else ("matrix", "none"))


# ---- 2. encode and parity-only commit against the oracle -------------------------
_oracle = {}


def _commit_ref(ref, n, f):
    """Values, lengths and the oracle's commitment of the ragged batch, once per geometry."""
    if (n, f) not in _oracle:
        k = n - 2 * f
        vpitch = rup(k * max(SHARD_LENS), 16) + 16
        rng = np.random.default_rng(5300 + 7 * n + f)
        values = rng.integers(0, 256, (len(SHARD_LENS), vpitch), dtype=np.uint8)  # random past B_i too: ignored
        # B_i a little short of k * S_i: the last rows carry Split's zero pad; S = 1: whole rows are pad
        vlens = np.array([k * S - min(3, k - 1) for S in SHARD_LENS], np.uint32)
        assert all((int(B) + k - 1) // k == S for B, S in zip(vlens, SHARD_LENS)) and (k < 4 or vlens[0] < k)
        want = [ref.encode_commit(n, f, values[i, : vlens[i]]) for i in range(len(SHARD_LENS))]
        values.setflags(write=False)
        _oracle[(n, f)] = (values, vlens, vpitch, want)
    return _oracle[(n, f)]


@pytest.mark.parametrize("n,f,lane", ALL, ids=_ids(ALL))
def test_encode_ragged_batch_equals_the_oracle(gpu, ref, n, f, lane):
    ctx = small(gpu, n, f, lane)
    k, p, d, I = ctx.k, ctx.p, ctx.depth, len(SHARD_LENS)
    values, vlens, vpitch, want = _commit_ref(ref, n, f)
    spitch = rup(max(SHARD_LENS), 64)

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


# ---- 2b. long rows, several waves to a SIMD ---------------------------------------
_long = {}


def _long_encode(gpu, n, f, codec, lane):
    """48 instances of rows of 64 KiB: 3,072 lane-4 waves, several to a SIMD.  (With 16-byte
    stores the wider lane stored a later value of a data register there, and nowhere at 8 KiB.)"""
    k, I = n - 2 * f, 48
    S = 65536
    B = k * S - min(2, k - 1)
    sp, vp = rup(S, 64), rup(k * S + 32, 64)
    if (n, f) not in _long:
        values = np.random.default_rng(5600 + n).integers(0, 256, (I, vp), dtype=np.uint8)
        values.setflags(write=False)
        _long[(n, f)] = values
    ctx = gpu.Context(n, f)
    ctx.set_codec(codec)
    ctx.set_fft_lane(lane)
    bv, bs = gpu.DeviceBuffer(I * vp), gpu.DeviceBuffer(I * n * sp)
    bv.upload(_long[(n, f)])
    bs.upload(np.full(I * n * sp, 0xA5, np.uint8))
    ctx.dev_encode(None, I, bv, vp, None, B, bs, sp)
    gpu.rbc.lib.rbc_device_sync(0)
    return bs.download().reshape(I, n, sp)


@pytest.mark.parametrize("n,f", [(7, 2), (13, 4), (20, 6)])
def test_long_rows_equal_the_matrix_codec_at_every_lane(gpu, n, f):
    want = _long_encode(gpu, n, f, "matrix", 0)
    for lane in fsm.lane_widths(n):
        got = _long_encode(gpu, n, f, "fft_small", lane)
        bad = np.flatnonzero((got != want).any(axis=(1, 2)))
        assert bad.size == 0, (lane, bad[:8], int((got != want).sum()))


# ---- 3. the whole receive path against the matrix codec --------------------------
_matrix_rx = {}


def _matrix_receive(gpu, n, f, B, step):
    if (n, f, B, step) not in _matrix_rx:
        _matrix_rx[(n, f, B, step)] = _receive(gpu, n, f, B, 8, "matrix", "none", step)
    return _matrix_rx[(n, f, B, step)]


@pytest.mark.parametrize("step", [False, True], ids=["receive", "receive_step"])
@pytest.mark.parametrize("n,f,lane", RX, ids=_ids(RX))
def test_receive_path_equals_the_matrix_codec(gpu, n, f, lane, step):
    k = n - 2 * f
    B = 61 * k - min(3, k - 1)
    a = _matrix_receive(gpu, n, f, B, step)
    b = _receive(Laned(gpu, lane), n, f, B, 8, "fft_small", "small", step)
    _same_receive(a, b, k, B)


# ---- 4. small against specialised ------------------------------------------------
@pytest.mark.parametrize("S", [61, 2100])
@pytest.mark.parametrize("n,f,lane", _cases(SPECIAL), ids=_ids(_cases(SPECIAL)))
def test_small_form_equals_the_specialised_one(gpu, n, f, lane, S):
    """S = 2100: rows long enough for the specialised decode's fused join, which
    the small form leaves to join_kernel; the values must not differ."""
    k = n - 2 * f
    B = S * k - min(3, k - 1)
    for step in (False, True):
        a = _receive(gpu, n, f, B, 8, "fft", "specialised", step)
        b = _receive(Laned(gpu, lane), n, f, B, 8, "fft_small", "small", step)
        _same_receive(a, b, k, B)


@pytest.mark.parametrize("n,f,lane", _cases(SPECIAL), ids=_ids(_cases(SPECIAL)))
def test_small_form_flags_the_specialised_ones_byzantine_row(gpu, n, f, lane):
    """A Byzantine parity row that verifies: the compare class, the flag and the re-hash list."""
    k = n - 2 * f
    row = k + (n - k) // 2
    sa, da_, ra = _noncodeword(gpu, n, f, "fft", "specialised", row)
    sb, db, rb = _noncodeword(Laned(gpu, lane), n, f, "fft_small", "small", row)
    assert (sa == ROOT_MISMATCH).all() and np.array_equal(sa, sb)
    assert np.array_equal(da_, db) and np.array_equal(ra, rb)


# ---- 5. non-codeword -------------------------------------------------------------
NONCODE = [(n, f, row, lane) for n, f, row in [(10, 3, 7), (20, 6, 14), (31, 10, 30)] for lane in fsm.lane_widths(n)]


@pytest.mark.parametrize("n,f,row,lane", NONCODE, ids=[f"n{n}f{f}-lane{lane}" for n, f, _, lane in NONCODE])
def test_small_form_rejects_a_noncodeword(gpu, n, f, row, lane):
    assert n - 2 * f <= row < n
    status, _, _ = _noncodeword(Laned(gpu, lane), n, f, "fft_small", "small", row)
    assert (status == ROOT_MISMATCH).all()


# ---- 6. dirty pads, and an instance the transform must skip ----------------------
DIRTY = _cases([(7, 2), (13, 4), (20, 6)])


@pytest.mark.parametrize("n,f,lane", DIRTY, ids=_ids(DIRTY))
def test_dirty_pads_and_a_skipped_instance(gpu, n, f, lane):
    I = 3
    k = n - 2 * f
    pl = Pipeline(Laned(gpu, lane), n, f, 61 * k - min(3, k - 1), I, seed=77, corrupt_frac=0.0, codec="fft_small")
    assert (pl.ctx.fft_form, pl.ctx.fft_lane) == ("small", lane)
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


# ---- 7. every stage inside a guarded arena ---------------------------------------
ARENA = _cases([(20, 6), (7, 2)])
_tight = {}


def _tight_ref(ref, n, f):
    """The ragged batch with the values packed at a pitch that is no multiple of 16 and ends at
    most 2 bytes past the last (and longest) value: the last dwords a lane reads of it reach the
    end of the value buffer."""
    if (n, f) not in _tight:
        k = n - 2 * f
        vlens = np.array([k * S - min(3, k - 1) for S in SHARD_LENS], np.uint32)
        assert vlens[-1] == vlens.max()
        vpitch = int(vlens[-1]) + 1
        if vpitch % 16 == 0:
            vpitch += 1
        assert vpitch % 16 and vpitch - int(vlens[-1]) <= 3
        rng = np.random.default_rng(5400 + 7 * n + f)
        values = rng.integers(1, 256, (len(SHARD_LENS), vpitch), dtype=np.uint8)
        want = [ref.encode_commit(n, f, values[i, : vlens[i]]) for i in range(len(SHARD_LENS))]
        values.setflags(write=False)
        _tight[(n, f)] = (values, vlens, vpitch, want)
    return _tight[(n, f)]


@pytest.mark.parametrize("form", ["encode", "parity"])
@pytest.mark.parametrize("n,f,lane", ARENA, ids=_ids(ARENA))
def test_encode_and_commit_write_only_their_outputs(gpu, ref, n, f, lane, form):
    ctx = small(gpu, n, f, lane)
    k, p, d, I = ctx.k, ctx.p, ctx.depth, len(SHARD_LENS)
    values, vlens, vpitch, want = _tight_ref(ref, n, f)
    spitch = rup(max(SHARD_LENS), 64)
    assert spitch % 64 == 0 and spitch % 1024
    specs = [("values", I * vpitch, "in"), ("value_lens", I * 4, "in"), ("shard_lens", I * 4, "in")]
    if form == "parity":
        specs += [("data_rows", I * k * spitch, "out"), ("parity", I * p * spitch, "out"),
                  ("leaves", I * n * 32, "out"), ("roots", I * 32, "out"), ("branches", I * n * d * 32, "out")]
    else:
        specs += [("shards", I * n * spitch, "out")]
    arena, at = da.make(gpu, specs, seed=900 + n + lane, row_pitch=spitch)
    arena.put("values", values)
    arena.put("value_lens", vlens)
    arena.put("shard_lens", np.array(SHARD_LENS, np.uint32))
    if form == "encode":
        ctx.dev_encode(None, I, at["values"], vpitch, at["value_lens"], 0, at["shards"], spitch)
    else:
        ctx.dev_shard_commit_parity(None, I, at["values"], vpitch, at["value_lens"], 0, at["data_rows"], at["parity"],
                                    spitch, at["shard_lens"], at["leaves"], at["roots"], at["branches"])
    gpu.rbc.lib.rbc_device_sync(0)
    out = arena.check()
    if form == "parity":
        rows = np.concatenate([out["data_rows"].reshape(I, k, spitch), out["parity"].reshape(I, p, spitch)], axis=1)
        roots = out["roots"].reshape(I, 32)
    else:
        rows = out["shards"].reshape(I, n, spitch)
    for i, S in enumerate(SHARD_LENS):
        assert np.array_equal(rows[i, :, :S], want[i][0]), (i, S)
        assert not rows[i, :, S:].any(), ("bytes past S must be zero", i)
        if form == "parity":
            assert bytes(roots[i]) == want[i][1], i


_rx_arena = {}


def _rx_case(n, f):
    if (n, f) not in _rx_arena:
        case = rc.Case(n, f, None, None, "worst", 5500 + n, corrupt={0, 5}, byz={2, 7}, too_few={3}, lens=SHARD_LENS)
        assert sorted(set(case.want_status)) == [-8, -3, 0]
        _rx_arena[(n, f)] = case
    return _rx_arena[(n, f)]


@pytest.mark.parametrize("n,f,lane", ARENA, ids=_ids(ARENA))
def test_decode_writes_only_its_outputs(gpu, n, f, lane):
    """rbc_dev_verify + rbc_dev_interpolate on a ragged batch: honest, corrupted, Byzantine (the
    compare, the flags and the re-hash list: random rows at S = 13, one altered parity row at
    S = 2053) and too-few instances."""
    ctx = small(gpu, n, f, lane)
    case = _rx_case(n, f)
    assert case.spitch % 64 == 0 and case.spitch % 1024
    arena, _ = da.make(gpu, da.rx_specs(case), seed=950 + n + lane, row_pitch=case.spitch)
    dev = da.RxRegions(arena, case)
    dev.verify(ctx)
    dev.interpolate(ctx, joined=True, leaves_verified=1)
    gpu.rbc.lib.rbc_device_sync(0)
    got = dev.read(arena.check())
    rc.check_against_oracle(case, got, joined=True, prefill=dev.prefill())


# ---- 8. host path ----------------------------------------------------------------
@pytest.mark.parametrize("lane", fsm.lane_widths(19))
def test_host_commit_and_receive_round_trip(gpu, ref, lane):
    n, f = 19, 6
    ctx = small(gpu, n, f, lane)
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
