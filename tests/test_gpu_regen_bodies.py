"""Every straight-line pass body of gf_regen_kernel on the GPU.

The FFT codec's interpolate regenerates the m missing data rows of an instance
with gf_regen_kernel, in passes of at most RC rows; dispatch_rows<1, RC>
instantiates one body per exact row count: 1..40 for the 256-byte-tile form
(W = 1, rows of at most 2048 bytes) and 1..24 for the 512-byte-tile form
(W = 2).  Each case of launch_rules.REGEN_BODY_CASES is one batch whose
instance i misses exactly m_i data rows at seeded random positions and holds
every parity row, so one launch runs one body per instance;
tests/test_launch_rules.py asserts without a GPU that the cases reach all 64
bodies under the launcher's own rule (host_shared.h's rbc_gf_regen_form).

S = 260 (pitch 320) is two 256-byte tiles for a block of three waves, the
second tile 64 bytes wide; S = 2049 (pitch 2112) is five 512-byte tiles in
groups of four with a 64-byte last tile.  The absent rows hold garbage over
the whole pitch.  After the call -- rbc_dev_verify + rbc_dev_interpolate, and
rbc_dev_receive_step -- every row equals the oracle's committed row and is
zero from S to the pitch, every value is the input, and leaves, digests,
valid and status are the oracle's.  All buffers are carved from one guarded
arena (tests/dev_arena.py): nothing outside the outputs may change."""
import numpy as np
import pytest

import dev_arena as da
import launch_rules as lr
import rx_cases as rc

pytestmark = pytest.mark.gpu

_cases = {}


def _case(n, f, S, ms):
    if (n, S) not in _cases:
        _cases[(n, S)] = rc.Case(n, f, S, len(ms), "data_missing", 9100 + n + S, missing=ms)
    return _cases[(n, S)]


@pytest.mark.parametrize("mode", ["oneshot", "step"])
@pytest.mark.parametrize("n,f,S,ms", lr.REGEN_BODY_CASES,
                         ids=[f"n{n}-S{S}-m1..{ms[-1]}" for n, f, S, ms in lr.REGEN_BODY_CASES])
def test_every_regen_pass_body(gpu, n, f, S, ms, mode):
    case = _case(n, f, S, ms)
    k = case.k
    assert [int((case.present[i, :k] == 0).sum()) for i in range(case.count)] == ms
    assert (case.present[:, k:] == 1).all() and not case.want_status.any()
    W, rows_per_pass, _ = lr.gf_regen_form(False, S, case.spitch)
    assert max(ms) <= rows_per_pass and W == (1 if S <= 2048 else 2)  # one pass, one body per instance
    ctx = gpu.Context(n, f)
    assert ctx.codec == "fft"
    arena, _ = da.make(gpu, da.rx_specs(case), seed=n + S, row_pitch=case.spitch)
    dev = da.RxRegions(arena, case)
    held = case.receiver_rows()
    gone = case.present == 0
    # the absent rows are poisoned: garbage on [0, S) and in the pad
    assert ((held[gone][:, :S] != case.want_rows[gone]).mean(axis=1) > 0.5).all() and held[gone][:, S:].any(axis=1).all()
    if mode == "oneshot":
        dev.verify(ctx)
        dev.interpolate(ctx)
    else:
        b = dev.rx_batch(ctx)
        ctx.dev_receive_step(None, b, None)
        ctx.dev_receive_step(None, None, b)
    gpu.rbc.lib.rbc_device_sync(0)
    got = dev.read(arena.check())
    rc.check_against_oracle(case, got, prefill=dev.prefill())
    # every row, received or regenerated, data or parity: the committed one, zero from S to the pitch
    assert np.array_equal(got["rows"], case.want_rows) and np.array_equal(case.want_rows, case.rows_in)
    assert not got["pitch_rows"][:, :, S:].any()
    # every value is the input: the data rows joined, the Split pad zero
    assert np.array_equal(got["values"][:, : k * S], case.rows_in[:, :k].reshape(case.count, k * S))
    assert not got["values"][:, case.B: k * S].any()
