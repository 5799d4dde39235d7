"""rbc_dev_receive_step over three consecutive batches, (A, -), (B, A), (C, B),
(-, C), against the serial path (rbc_dev_verify then rbc_dev_interpolate) on
the same inputs and against the oracle.

Consecutive batches differ in exactly what the step's shared workspace carries
from one call to the next -- the changed-row flags, the list of rows to hash
and the instances handed to the full recheck: A holds a Byzantine non-codeword
instance (flags set, full recheck), B is clean, C holds another non-codeword
instance index and one corrupted ECHO.  Whatever of prev's state the call's
decode of cur overwrote too early would show as a wrong status, leaf or row of
prev.  Every batch has its own shard, branch, leaf, valid, status, digest and
value buffers.

With a marks struct every recorded event is complete after a stream sync, and
prev_released does not precede the root recheck's status write: a second
stream that waits for that event alone reads prev's final statuses."""
import numpy as np
import pytest

import rx_cases as rc

pytestmark = pytest.mark.gpu


def _batches(n, f, S):
    k = n - 2 * f
    odd = 1  # a codeword with one altered unused parity row (rx_cases: odd instances)
    a = rc.Case(n, f, S, 4, "worst", seed=11 * n + 1, byz={odd})
    b = rc.Case(n, f, S, 4, "parity", seed=11 * n + 2)
    c = rc.Case(n, f, S, 4, "worst", seed=11 * n + 3, byz={2}, corrupt={0})
    assert (a.want_status != 0).sum() == 1 and not b.want_status.any() and c.want_status[2] == -8
    assert c.bad[0] >= 0 and k > 0
    return [a, b, c]


def _step_sequence(gpu, cases, marks):
    n, f = cases[0].n, cases[0].f
    rx = gpu.Context(n, f)
    st, side = gpu.Stream(0), gpu.Stream(0)
    devs = [rc.DevCase(gpu, c) for c in cases]
    bs = [d.rx_batch(rx) for d in devs]
    released = []  # prev's statuses as a stream that waited for prev_released alone saw them
    events = []
    prev = None
    for cur in bs + [None]:
        if marks:
            ev = {name: gpu.Event() for name in ("hashed", "decode_begin", "decoded", "hash_begin", "rows_hashed",
                                                 "prev_released")}
            if cur is None:  # no decode in the flush call
                del ev["decode_begin"], ev["decoded"]
            if prev is None:
                del ev["prev_released"]
            rx.dev_receive_step(st.ptr, cur, prev, **ev)
            events.append(ev)
            if prev is not None:
                side.wait(ev["prev_released"])
                side.sync()
                released.append(devs[bs.index(prev)].read_status())
        else:
            rx.dev_receive_step(st.ptr, cur, prev)
        prev = cur
    st.sync()
    for ev in events:  # complete: an elapsed time between two of them can be taken
        names = list(ev)
        for x, y in zip(names, names[1:]):
            assert ev[x].elapsed_ms(ev[y]) > -1e9
        if "decoded" in ev:
            assert ev["hash_begin"].elapsed_ms(ev["rows_hashed"]) >= 0
            assert ev["hashed"].elapsed_ms(ev["decode_begin"]) >= 0
            assert ev["decode_begin"].elapsed_ms(ev["decoded"]) >= 0
    gpu.rbc.lib.rbc_device_sync(0)
    return [d.read() for d in devs], released


@pytest.mark.parametrize("n,f,S", [(128, 42, 260), (4, 1, 64), (256, 85, 64)])
def test_receive_step_three_batches_equal_serial_path(gpu, n, f, S):
    cases = _batches(n, f, S)
    ctx = gpu.Context(n, f)
    want = []
    for c in cases:
        d = rc.DevCase(gpu, c)
        d.serial(ctx)
        gpu.rbc.lib.rbc_device_sync(0)
        want.append(d.read())
    for marks in (False, True):
        got, released = _step_sequence(gpu, cases, marks)
        for bi, c in enumerate(cases):
            rc.check_against_oracle(c, got[bi])
            ok = c.want_status == 0
            for key in ("rows", "valid", "leaves", "status"):
                assert np.array_equal(got[bi][key], want[bi][key]), (bi, key)
            assert np.array_equal(got[bi]["values"][ok], want[bi]["values"][ok]), bi
            assert np.array_equal(got[bi]["digests"][ok], want[bi]["digests"][ok]), bi
            if marks:  # final when prev_released completes
                assert np.array_equal(released[bi], c.want_status), (bi, released[bi])
