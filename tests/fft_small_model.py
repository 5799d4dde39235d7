#!/usr/bin/env python3
"""Python model of `rs_fft_small_kernel` (csrc/rs_fft_small.hip): the run-time-
geometry additive-FFT encoder of fft_any_model.py at the widths W = 8, 16, 32,
and the column packing of a lane that owns CW adjacent dword columns (test
infrastructure: pins the kernel's structure against the oracle on the CPU).

The transform is fft_any_model's, function for function and unchanged: solve_any
with swapped halves and run-time cosets, fft_out pruned to [k, n).  What this
file adds is

* the width rule: the smallest of 8, 16, 32 that is >= n (host_shared.h's
  rbc_fft_small_logw).  W < 2n, which rs_fft_any.hip's launcher guarantees, is
  not needed: encode() takes any LOGW with 2^LOGW >= n;
* the wider lane built for each width (rbc_fft_small_wide_lane): 4 dwords at
  W = 8 and 16, 2 at W = 32;
* the packing: lane L of column tile t owns the dwords (64 t + L) CW + c,
  c < CW, of every row, i.e. the bytes [off + 4c, off + 4c + 4) with
  off = 4 CW (64 t + L);
* the masks, per dword: keep_bytes4(S - off - 4c) on every row (the tail), and
  keep_bytes4(lim - off - 4c) on the data rows that carry Split's zero pad,
  lim = max(B - j S, 0);
* the decode compare: a lane flags a position when any of its CW masked dwords
  differs from what the row holds, and then stores all CW.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_any_model as fam  # noqa: E402

Counter = fam.Counter
LANES = 64


def width_log2(n_total):
    """LOGW of the kernel that runs n_total (2 <= n_total <= 32)."""
    assert 2 <= n_total <= 32
    return 3 if n_total <= 8 else 4 if n_total <= 16 else 5


def wide_lane(w):
    """The wider lane width built for transform width w."""
    return 4 if w <= 16 else 2


def lane_widths(n_total):
    return (1, wide_lane(1 << width_log2(n_total)))


def encode(k, n_total, data, cnt=None, logw=None):
    """data: k rows (uint8 arrays) -> n_total rows (systematic codeword), by the
    transform of width 2^logw (default: the width rule)."""
    cnt = cnt if cnt is not None else Counter()
    logw = width_log2(n_total) if logw is None else logw
    w = 1 << logw
    assert logw >= fam.G and 1 <= k <= n_total <= w
    zero = np.zeros_like(data[0])
    v = [np.array(data[j]) if j < k else zero.copy() for j in range(w)]
    fam.solve_any(v, logw, k, cnt)
    assert all(not v[j].any() for j in range(k, w)), "coefficients [k, W) must be zero after solve"
    out = [np.array(data[j]) for j in range(k)] + [None] * (n_total - k)
    fam.fft_out(v, logw, 0, k, k, n_total, out, cnt)
    return out


# ---- the column packing ------------------------------------------------------------
def keep_bytes4(nv):
    return 0xFFFFFFFF if nv >= 4 else 0 if nv <= 0 else (1 << (8 * nv)) - 1


def lane_offset(tile, lane, cw):
    """Byte offset inside the row of the first dword of `lane` of column tile `tile`."""
    return 4 * cw * (LANES * tile + lane)


def tiles(row_pitch, cw):
    """The launch's column tiles: grid.x of launch_small."""
    return (row_pitch // 4 + LANES * cw - 1) // (LANES * cw)


def lanes(row_pitch, cw):
    """(tile, lane, off) of every lane that runs: off < row_pitch."""
    for t in range(tiles(row_pitch, cw)):
        for lane in range(LANES):
            off = lane_offset(t, lane, cw)
            if off < row_pitch:
                yield t, lane, off


def dwords(row, off, cw):
    """What a lane loads of a row (a uint8 array of row_pitch bytes): cw little-endian dwords."""
    return [int.from_bytes(row[off + 4 * c: off + 4 * c + 4].tobytes(), "little") for c in range(cw)]


def masked_row(row, limit, cw):
    """Every lane loads its dwords of `row`, keeps the bytes below `limit`
    (per dword: keep_bytes4(limit - off - 4c)) and stores them: the row as the
    kernel leaves it."""
    pitch = len(row)
    assert pitch % (4 * cw) == 0
    out = np.full(pitch, 0xEE, np.uint8)  # a byte no lane stores stays 0xEE
    for _, _, off in lanes(pitch, cw):
        for c, x in enumerate(dwords(row, off, cw)):
            x &= keep_bytes4(limit - off - 4 * c)
            out[off + 4 * c: off + 4 * c + 4] = np.frombuffer(x.to_bytes(4, "little"), np.uint8)
    return out


def pad_limit(j, S, B):
    """Bytes of data row j that come from the value of B bytes: min(S, max(B - j S, 0))."""
    return S if j * S + S <= B else max(B - j * S, 0)


def flagged_lanes(old, new, S, cw):
    """The lanes whose compare fails: any of the lane's dwords of `new`, masked to
    the bytes below S, differs from the same dword of `old` (unmasked, as held)."""
    bad = []
    for t, lane, off in lanes(len(old), cw):
        o, x = dwords(old, off, cw), dwords(new, off, cw)
        if any(o[c] != (x[c] & keep_bytes4(S - off - 4 * c)) for c in range(cw)):
            bad.append((t, lane))
    return bad


def main():
    rng = np.random.default_rng(1)
    for (n, f) in [(7, 2), (10, 3), (13, 4), (16, 5), (19, 6), (20, 6), (25, 8), (31, 10), (32, 10)]:
        k = n - 2 * f
        data = [rng.integers(0, 256, 8, dtype=np.uint8) for _ in range(k)]
        want = fam.fm.orc.gf_rows(fam.fm.orc.encode_matrix(k, n)[k:], data)
        cnt = Counter()
        got = encode(k, n, data, cnt)
        ok = all(np.array_equal(g, w) for g, w in zip(got[k:], want))
        print(f"N={n:3d} k={k:3d} W={1 << width_log2(n):2d}: {'OK ' if ok else 'BAD'} butterflies={cnt.bfly} "
              f"unwind macs={cnt.mac} moves={cnt.copy} (matrix MACs {k * (n - k)})")


if __name__ == "__main__":
    main()
