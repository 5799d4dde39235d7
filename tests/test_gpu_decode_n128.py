"""The N=128 FFT decode (rs_fft_kernel<7,44,128,decode>: class bytes held in
scalar registers, compare loads prefetched one output group ahead) through
rbc_dev_verify + rbc_dev_interpolate(leaves_verified = 1), against the oracle.

Shard lengths: 4 and 5 (one lane's whole dword, then one byte into the next
lane's), 252 / 256 / 260 (a 64-lane tile one dword short, exactly full, and one
dword into a second tile), 763 (the C4 length: three tiles, a 3-byte last
dword) and 2052 (nine tiles, a row pad of 60 bytes: long enough for the decode
itself to join the value).  Every pattern of rx_cases.PATTERNS: per case every shard row,
valid byte, leaf, status, digest and the joined value with its zero tail are
compared with the oracle; the row view (values_out = NULL) and the matrix
codec must leave the same bytes.  N=64 and N=256 run one length to show the
other geometries compute what they did."""
import numpy as np
import pytest

import rx_cases as rc

pytestmark = pytest.mark.gpu

LENS = (4, 5, 252, 256, 260, 763, 2052)


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


def _run_all_forms(gpu, ctxs, n, f, S, pattern, seed):
    case = rc.Case(n, f, S, 8, pattern, seed)
    dev = rc.DevCase(gpu, case)
    fft = ctxs(n, f)
    assert fft.codec == "fft"
    dev.serial(fft)
    got = dev.read()
    rc.check_against_oracle(case, got)
    if pattern == "none":  # nothing regenerated: the receiver's buffer is untouched, pads included
        assert np.array_equal(dev.shards.download().reshape(8, n, case.spitch), case.receiver_rows())
    if pattern == "byzantine":  # the compared rows that differ were stored and re-hashed (odd: exactly one)
        assert all(len(case.changed[i]) == 1 for i in range(1, 8, 2))
    # the row view: no join, everything else the same
    dev.reset()
    dev.serial(fft, joined=False)
    view = dev.read()
    rc.check_against_oracle(case, view, joined=False)
    assert (view["values"] == 0xA5).all()
    # the matrix codec leaves the same bytes
    dev.reset()
    mat = ctxs(n, f, "matrix")
    assert mat.codec == "matrix"
    dev.serial(mat)
    other = dev.read()
    ok = case.want_status == 0
    for key in ("rows", "valid", "leaves", "status"):
        assert np.array_equal(got[key], other[key]), key
    assert np.array_equal(got["values"][ok], other["values"][ok])
    assert np.array_equal(got["digests"][ok], other["digests"][ok])


@pytest.mark.parametrize("pattern", rc.PATTERNS)
@pytest.mark.parametrize("S", LENS)
def test_decode_n128_every_pattern_against_oracle(gpu, ctxs, S, pattern):
    _run_all_forms(gpu, ctxs, 128, 42, S, pattern, seed=1000 * S + rc.PATTERNS.index(pattern))


@pytest.mark.parametrize("pattern", ["corrupt_data", "byzantine"])
@pytest.mark.parametrize("n,f", [(64, 21), (256, 85)])
def test_decode_other_geometries_unchanged(gpu, ctxs, n, f, pattern):
    _run_all_forms(gpu, ctxs, n, f, 260, pattern, seed=n)
