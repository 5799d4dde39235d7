"""CPU checks of the small run-time-geometry additive-FFT codec's structure
(tests/fft_small_model.py mirrors rs_fft_small.hip: fft_any_model's transform at
W = 8, 16, 32, and the packing, masks and compare of a lane that owns several
dword columns).  Every output byte must equal klauspost v1.9.1's encode-matrix
product, at every (n, k) the kernel accepts."""
import numpy as np
import pytest

import fft_small_model as fsm
import rbc_oracle as orc

_rng = np.random.default_rng(20261021)
_DATA = [_rng.integers(0, 256, 4, dtype=np.uint8) for _ in range(32)]  # shared, never written
_MATRIX = {}


def _want(n, k):
    if (n, k) not in _MATRIX:
        _MATRIX[(n, k)] = orc.gf_rows(orc.encode_matrix(k, n)[k:], _DATA[:k]) if n > k else []
    return _MATRIX[(n, k)]


def _check(n, k, logw):
    got = fsm.encode(k, n, _DATA[:k], logw=logw)
    assert len(got) == n
    assert all(np.array_equal(g, d) for g, d in zip(got[:k], _DATA))
    assert all(np.array_equal(g, w) for g, w in zip(got[k:], _want(n, k))), (n, k, logw)


def test_width_rule():
    assert [fsm.width_log2(n) for n in (2, 7, 8, 9, 16, 17, 31, 32)] == [3, 3, 3, 4, 4, 5, 5, 5]
    assert [fsm.wide_lane(w) for w in (8, 16, 32)] == [4, 4, 2]
    assert fsm.lane_widths(7) == (1, 4) and fsm.lane_widths(16) == (1, 4) and fsm.lane_widths(17) == (1, 2)


def test_every_geometry_at_the_rule_width_equals_the_matrix_product():
    cases = [(n, k) for n in range(2, 33) for k in range(1, n + 1)]
    assert len(cases) == 527
    for n, k in cases:
        _check(n, k, None)


def test_every_geometry_at_width_32_equals_the_matrix_product():
    """W < 2n is not needed: the widest transform runs every n, down to n = 2."""
    for n in range(2, 33):
        for k in range(1, n + 1):
            _check(n, k, 5)


def test_width_16_runs_every_n_up_to_16():
    for n in range(2, 17):
        for k in range(1, n + 1):
            _check(n, k, 4)


@pytest.mark.parametrize("n,f,bfly,mac", [(7, 2, 14, 1), (10, 3, 28, 0), (13, 4, 32, 1), (20, 6, 36, 0),
                                          (31, 10, 78, 4), (32, 10, 80, 4)])
def test_butterfly_count_is_the_design_figure(n, f, bfly, mac):
    """butterflies (one constant multiply each) and unwinding
    multiplies per byte column, against the matrix product's k (n - k) MACs."""
    k = n - 2 * f
    cnt = fsm.Counter()
    fsm.encode(k, n, [np.zeros(1, np.uint8)] * k, cnt)
    assert (cnt.bfly, cnt.mac) == (bfly, mac)
    assert (cnt.mul < k * (n - k)) == (n >= 13)  # the arithmetic gain starts at N = 13


SHARD_LENS = list(range(1, 41)) + list(range(1020, 1031))


@pytest.mark.parametrize("cw", [1, 2, 4])
def test_tail_mask_keeps_exactly_the_bytes_below_S(cw):
    rng = np.random.default_rng(7)
    for S in SHARD_LENS:
        pitch = (S + 63) // 64 * 64
        row = rng.integers(1, 256, pitch, dtype=np.uint8)  # no zero byte: a kept byte is seen
        got = fsm.masked_row(row, S, cw)
        assert np.array_equal(got[:S], row[:S]), (S, cw)
        assert not got[S:].any(), (S, cw)  # every byte of the pitch is stored, as zero past S


@pytest.mark.parametrize("cw", [1, 2, 4])
def test_pad_mask_keeps_exactly_the_bytes_of_the_value(cw):
    """The data rows that carry Split's zero pad: row j keeps value bytes [j S, B)."""
    rng = np.random.default_rng(8)
    k = 5
    for S in SHARD_LENS:
        pitch = (S + 63) // 64 * 64
        for short in range(k):  # every B with ceil(B / k) == S; at S <= 4 whole rows are pad
            B = k * S - short
            assert (B + k - 1) // k == S
            for j in range(k):
                lim = fsm.pad_limit(j, S, B)
                assert lim == min(S, max(B - j * S, 0))
                row = rng.integers(1, 256, pitch, dtype=np.uint8)
                got = fsm.masked_row(row, lim, cw)
                assert np.array_equal(got[:lim], row[:lim]) and not got[lim:].any(), (S, B, j, cw)


@pytest.mark.parametrize("cw", [1, 2, 4])
def test_every_lane_owns_its_own_bytes_and_all_of_the_row(cw):
    for pitch in (64, 192, 1024, 1088, 2112):
        seen = np.zeros(pitch, np.int32)
        for _, _, off in fsm.lanes(pitch, cw):
            assert off % (4 * cw) == 0 and off + 4 * cw <= pitch
            seen[off: off + 4 * cw] += 1
        assert (seen == 1).all(), (pitch, cw)


@pytest.mark.parametrize("cw", [1, 2, 4])
def test_compare_flags_a_lane_when_any_of_its_dwords_differs(cw):
    rng = np.random.default_rng(9)
    for S in (1, 13, 61, 1028):
        pitch = (S + 63) // 64 * 64
        new = rng.integers(0, 256, pitch, dtype=np.uint8)  # the regenerated row, garbage past S included
        held = new.copy()
        held[S:] = 0
        assert fsm.flagged_lanes(held, new, S, cw) == []
        for at in sorted({0, S // 2, S - 1}):
            bad = held.copy()
            bad[at] ^= 0x40
            col = at // (4 * cw)
            assert fsm.flagged_lanes(bad, new, S, cw) == [(col // 64, col % 64)], (S, at, cw)
        if S < pitch:  # a dirty pad byte of the held row is seen too: the row is rewritten with zeros there
            bad = held.copy()
            bad[S] = 1
            assert len(fsm.flagged_lanes(bad, new, S, cw)) == 1
