"""The receive side (rbc_dev_verify + rbc_dev_interpolate, the row view, and
rbc_dev_receive_step) outside the envelope of uniform, full, zero-padded,
honest-or-data-complete batches, against the oracle:

* ragged shard lengths at (128,42) -- per-instance S in the prefetch decode,
  join_kernel instead of the fused join, 11 instances x 9 column tiles (the
  remainder of the XCD tile remap with more than one tile per instance), SHA
  tails on both sides of the one-block / two-block padding boundary -- and a
  smaller ragged list at the other FFT geometries;
* instances with k-1 ECHOs (status -3) first, in the middle and last in a
  batch whose other instances decode: every kernel after the prepare skips
  them, also the ones the next receive step launches for prev;
* non-zero bytes in [S, pitch) of every received row (a reused wire ring):
  every specified output byte equals the zero-padded run's;
* non-codewords whose k-th valid row sits at a chosen index, around every wave
  boundary of decode_prepare_fft_kernel's ballot ranks, on both codecs;
* more than 65535 instances on the FFT launch's gridDim.y.

Every case is one of rx_cases.CONTRACT; test_rx_cases_host.py checks the same
cases' references against each other without a device."""
import numpy as np
import pytest

import rbc_ref
import rx_cases as rc

pytestmark = pytest.mark.gpu

KEYS = ("rows", "valid", "leaves", "status", "digests", "values")


@pytest.fixture(scope="module")
def ctxs(gpu):
    made = {}

    def get(n, f, codec="auto"):
        if (n, f, codec) not in made:
            c = gpu.Context(n, f)
            if codec != "auto":
                c.set_codec(codec)
            made[(n, f, codec)] = c
        return made[(n, f, codec)]
    return get


def _same(case, a, b, what, joined=True):
    x, y = rc.specified(case, a, joined), rc.specified(case, b, joined)
    for key in KEYS:
        assert np.array_equal(x[key], y[key]), (what, key)


def _forms(gpu, ctx, case):
    """The three forms on fresh copies of one case: each against the oracle,
    and every specified byte the same in all of them.  -> the serial form's."""
    dev = rc.DevCase(gpu, case)
    sync = gpu.rbc.lib.rbc_device_sync
    dev.serial(ctx)
    sync(0)
    serial = dev.read()
    rc.check_against_oracle(case, serial)
    dev.reset()
    dev.serial(ctx, joined=False)
    sync(0)
    view = dev.read()
    rc.check_against_oracle(case, view, joined=False)
    assert (view["values"] == rc.VALUE_FILL).all()
    _same(case, serial, view, "row view", joined=False)
    dev.reset()
    b = dev.rx_batch(ctx)
    ctx.dev_receive_step(None, b, None)
    ctx.dev_receive_step(None, None, b)
    sync(0)
    step = dev.read()
    rc.check_against_oracle(case, step)
    _same(case, serial, step, "receive step")
    return serial


def _both_codecs(gpu, ctxs, case):
    fft, mat = ctxs(case.n, case.f), ctxs(case.n, case.f, "matrix")
    assert fft.codec == "fft" and mat.codec == "matrix"
    a = _forms(gpu, fft, case)
    b = _forms(gpu, mat, case)
    _same(case, a, b, "matrix codec")
    return a


# ---- 1. ragged lengths ---------------------------------------------------------
@pytest.mark.parametrize("pattern", ["worst", "corrupt_data", "byzantine"])
def test_ragged_lengths_n128(gpu, ctxs, pattern):
    case = rc.contract_case(f"ragged-128-{pattern}")
    assert case.count == 11 and case.spitch == 2112 and case.ragged
    _both_codecs(gpu, ctxs, case)


@pytest.mark.parametrize("n", [4, 16, 64, 256])
def test_ragged_lengths_other_geometries(gpu, ctxs, n):
    _both_codecs(gpu, ctxs, rc.contract_case(f"ragged-{n}"))


# ---- 2. too few shards inside a batch ------------------------------------------
@pytest.mark.parametrize("shape", ["uniform", "ragged"])
@pytest.mark.parametrize("base", ["worst", "byzantine"])
@pytest.mark.parametrize("n", [128, 64])
def test_too_few_inside_a_batch(gpu, ctxs, n, base, shape):
    a, b = (rc.contract_case(f"few-{n}-{base}-{shape}-{x}") for x in "ab")
    assert a.too_few == set(rc.FEW_A) and b.too_few == set(rc.FEW_B) and a.count == b.count == 11
    ctx = ctxs(a.n, a.f)
    assert ctx.codec == "fft"
    want = [_forms(gpu, ctx, c) for c in (a, b)]
    # two consecutive batches: the rehash, recheck and digest of prev run in the
    # next call, beside cur's verify and decode, and must still skip prev's -3s
    devs = [rc.DevCase(gpu, c) for c in (a, b)]
    bs = [d.rx_batch(ctx) for d in devs]
    ctx.dev_receive_step(None, bs[0], None)
    ctx.dev_receive_step(None, bs[1], bs[0])
    ctx.dev_receive_step(None, None, bs[1])
    gpu.rbc.lib.rbc_device_sync(0)
    for c, d, w in zip((a, b), devs, want):
        got = d.read()
        rc.check_against_oracle(c, got)
        _same(c, w, got, "two batches")


# ---- 3. dirty pads -------------------------------------------------------------
@pytest.mark.parametrize("pattern", rc.DIRTY_PATTERNS)
@pytest.mark.parametrize("n,f,S", rc.DIRTY_GEOMS)
def test_dirty_pads_change_no_output(gpu, ctxs, n, f, S, pattern):
    clean, dirty = (rc.contract_case(f"pads-{n}-{S}-{pattern}-{x}") for x in ("clean", "dirty"))
    assert dirty.dirty_pads and not clean.dirty_pads
    ctx = ctxs(n, f)
    assert ctx.codec == ("matrix" if n == 37 else "fft")
    a, b = _forms(gpu, ctx, clean), _forms(gpu, ctx, dirty)
    _same(clean, a, b, "dirty pads")
    if pattern == "none":  # nothing regenerated: bytes [0, S) of every row are as received
        for case, got in ((clean, a), (dirty, b)):
            assert np.array_equal(got["rows"], case.receiver_rows()[:, :, :S])


# ---- 4. the k-th valid row at a chosen index -----------------------------------
@pytest.mark.parametrize("n,pos", [(n, pos) for (n, _), poss in rc.KTH_POS.items() for pos in poss])
def test_first_k_valid_boundary(gpu, ctxs, n, pos):
    case = rc.contract_case(f"kth-{n}-{pos}")
    assert case.S == 13 and case.count == 8 and case.want_status[0] == 0
    _both_codecs(gpu, ctxs, case)


# ---- 5. more than 65535 instances ----------------------------------------------
def _round_trip(gpu, ctx, values, B, present, garbage):
    """shard_commit, then verify + interpolate with the absent rows overwritten."""
    n, k, count = ctx.n, ctx.k, len(values)
    S = (B + k - 1) // k
    sp, vp, d = 64, values.shape[1], ctx.depth
    mb = gpu.DeviceBuffer
    dv, dsh, dlv, drt = mb(values.nbytes), mb(count * n * sp), mb(count * n * 32), mb(count * 32)
    dbr = mb(count * n * d * 32)
    dv.upload(values)
    ctx.dev_shard_commit(None, count, dv, vp, None, B, dsh, sp, None, dlv, drt, dbr)
    gpu.rbc.lib.rbc_device_sync(0)
    committed = dsh.download().reshape(count, n, sp).copy()
    held = np.where(present[:, :, None] == 1, committed, garbage)
    dsh.upload(held)
    dpr, dva, dlr = mb(count * n), mb(count * n), mb(count * n * 32)
    dout, ddg, dst = mb(count * vp), mb(count * 32), mb(count * 4)
    dpr.upload(present)
    dst.upload(np.full(count, -1, np.int32))
    ctx.dev_verify(None, count, dsh, sp, None, S, dbr, drt, dpr, dva, dlr)
    ctx.dev_interpolate(None, count, dsh, sp, None, S, dva, dlr, 1, drt, dout, vp, ddg, dst)
    gpu.rbc.lib.rbc_device_sync(0)
    return dict(committed=committed, held=held,
                roots=drt.download().reshape(count, 32).copy(),
                branches=dbr.download().reshape(count, n, d, 32).copy(),
                valid=dva.download().reshape(count, n).copy(),
                rows=dsh.download().reshape(count, n, sp).copy(),
                values=dout.download().reshape(count, vp).copy(),
                digests=ddg.download().reshape(count, 32).copy(),
                status=dst.download().view(np.int32).copy())


def test_instance_counts_beyond_65535(gpu):
    """65536 + 11 instances of (4,1): the FFT launch puts the instance on
    gridDim.y.  Either every call succeeds and every instance round-trips, or
    the argument checks refuse the count (RBC_ERR_INVALID_ARG, nothing
    enqueued) and the matrix codec runs the same batch.

    On an MI355X the runtime accepts gridDim.y = 65547 and the first outcome
    holds, so rbc_gpu.h states no limit on count."""
    n, f, B, count = 4, 1, 7, 65536 + 11
    rng = np.random.default_rng(65536)
    values = rng.integers(0, 256, (count, 32), dtype=np.uint8)
    present = np.ones((count, n), np.uint8)
    present[np.arange(count), rng.integers(0, n, count)] = 0
    garbage = rng.integers(0, 256, (count, n, 64), dtype=np.uint8)
    ctx = gpu.Context(n, f)
    assert ctx.codec == "fft" and ctx.k == 2
    try:
        r = _round_trip(gpu, ctx, values, B, present, garbage)
    except gpu.RBCError as e:
        assert e.code == -10, e  # RBC_ERR_INVALID_ARG from the argument checks, and nothing else
        ctx.set_codec("matrix")
        r = _round_trip(gpu, ctx, values, B, present, garbage)
    assert not r["status"].any(), np.flatnonzero(r["status"])[:8]
    assert np.array_equal(r["valid"], present)
    assert np.array_equal(r["values"][:, :B], values[:, :B])
    assert not r["values"][:, B:8].any()  # the Split pad inside the value
    assert np.array_equal(r["rows"], r["committed"])  # the absent row is back, zero pad included
    fixed = [0, 65534, 65535, 65536, count - 1]
    sample = fixed + [int(i) for i in rng.permutation(count) if i not in fixed][:59]
    assert len(set(sample)) == 64
    for i in sample:
        shards, root, br, _ = rbc_ref.encode_commit(n, f, values[i, :B])
        assert np.array_equal(r["committed"][i, :, :4], shards) and not r["committed"][i, :, 4:].any(), i
        assert bytes(r["roots"][i]) == root and np.array_equal(r["branches"][i], br), i
        st, val, dig = rbc_ref.interpolate(n, f, r["held"][i, :, :4], present[i], root)
        assert st == 0 and np.array_equal(r["values"][i, :8], val) and bytes(r["digests"][i]) == dig, i
