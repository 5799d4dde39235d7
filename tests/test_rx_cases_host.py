"""The cases of test_gpu_receiver_contract.py, on the host alone: the C oracle
(rbc_ref.interpolate), the Python oracle (rbc_oracle.Encoder.reconstruct) and
what rx_cases.Case expects agree with each other on every instance, so a
failure of the device tests can only be the kernels'.  No device is used."""
import numpy as np
import pytest

import rbc_ref
import rx_cases as rc

PURE_BYZANTINE = ("byzantine", "byzantine_data_gone")


@pytest.mark.parametrize("cid", list(rc.CONTRACT))
def test_case_references_agree(cid):
    c = rc.contract_case(cid)
    rows = c.receiver_rows()
    assert rows.shape == (c.count, c.n, c.spitch) and c.spitch % 64 == 0 and c.spitch >= c.S
    for i in range(c.count):
        Si = int(c.lens[i])
        st, val, _ = rbc_ref.interpolate(c.n, c.f, rows[i, :, :Si], c.want_valid[i], c.roots[i].tobytes())
        assert st == c.want_status[i], (i, st)
        if st == 0:
            assert np.array_equal(val, c.want_rows[i, : c.k, :Si].reshape(-1)), i
        # a received row carries what was committed; only the corrupted ECHO differs
        for j in np.flatnonzero(c.present[i]):
            assert np.array_equal(rows[i, j, :Si], c.rows_in[i, j, :Si]) == (j != c.bad[i]), (i, j)
        # every instance that is not too_few holds at least n - f ECHOs, or (kth_at) at least k + 1
        held = int(c.present[i].sum())
        assert held == c.k - 1 if i in c.too_few else held >= min(c.n - c.f, c.k + 1), (i, held)
    # no more than the too_few instances have rows, a value or a digest that cannot be compared
    assert set(np.flatnonzero(~c.specified.all(axis=1))) == c.too_few
    assert set(np.flatnonzero(c.want_status == -3)) == c.too_few
    # every batch delivers something, unless all of it is Byzantine by construction
    if not (c.pattern in PURE_BYZANTINE):
        assert (c.want_status == 0).any()
    if c.pattern == "kth_at":
        assert (c.want_status == 0).sum() == 1 and (c.want_status == -8).sum() == c.count - 1


@pytest.mark.parametrize("cid", [x for x in rc.CONTRACT if rc.CONTRACT[x][0][4] in rc.GONE_PATTERNS])
def test_first_k_rule_is_observable(cid):
    """The re-encoding of the last k valid rows differs from that of the first
    k: a decode that picked another valid set would leave other rows."""
    c = rc.contract_case(cid)
    assert len(c.gone) >= c.count - 1
    for i in c.gone:
        valid = np.flatnonzero(c.want_valid[i])
        assert len(valid) > c.k
        Si = int(c.lens[i])
        # want_rows is the re-encoding of valid[:k]: it keeps those rows as they were received
        assert np.array_equal(c.want_rows[i, valid[: c.k], :Si], c.rows_in[i, valid[: c.k], :Si])
        last = rc.reencode_from(c.n, c.k, c.rows_in[i, :, :Si], valid[-c.k:])
        assert not np.array_equal(last, c.want_rows[i, :, :Si]), i
        if c.pattern == "kth_at":
            pos = rc.CONTRACT[cid][1]["pos"]
            assert valid[c.k - 1] == pos and valid[-1] > pos
            assert any(j > pos for j in c.changed[i])  # an unused valid row above pos is replaced


@pytest.mark.parametrize("cid", [x for x in rc.CONTRACT if x.endswith("-dirty")])
def test_dirty_pads_change_no_expectation(cid):
    dirty, clean = rc.contract_case(cid), rc.contract_case(cid[: -len("dirty")] + "clean")
    assert dirty.dirty_pads and not clean.dirty_pads
    for key in ("want_rows", "want_valid", "want_status", "rows_in", "present", "roots", "branches", "bad", "lens"):
        assert np.array_equal(getattr(dirty, key), getattr(clean, key)), key
    assert np.array_equal(dirty.want_leaves(), clean.want_leaves())
    a, b = dirty.receiver_rows(), clean.receiver_rows()
    S = dirty.S
    assert np.array_equal(a[:, :, :S], b[:, :, :S])
    got = dirty.present == 1
    # every pad byte of a received row is non-zero (the partial dword's pad
    # bytes when S % 4 != 0, and every whole lane past S); clean: all zero
    assert dirty.spitch - rc.round_up(S, 4) >= 4
    assert (a[got][:, S:] != 0).all() and not b[got][:, S:].any()
    assert np.array_equal(a[~got], b[~got])  # absent rows: the same garbage
