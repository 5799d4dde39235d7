#!/usr/bin/env python3
"""Python model of `rs_fft_wide_kernel` (csrc/rs_fft_wide.hip): the
run-time-geometry additive-FFT encoder of fft_any_model.py for 129 <= n <= 256
as two 128-row halves (test infrastructure: pins the kernel's structure against
the oracle on the CPU).

P = P0 + s7 P1 with P0, P1 of fewer than 128 novel coefficients; s7 is 0 on the
positions 0..127 and 1 on 128..255 and W_7(0) = 0 (asserted in the tests), so
P = P0 on the lower half and P0 + P1 on the upper half.  The model keeps what
the kernel keeps: a list `v` of 128 rows, and `park`, the 128 rows set aside.

* k <= 128: solve (fft_any_model's, LOGW = 7) gives P0; park; the final
  transform on coset 0 emits [k, 128); reload; the final transform on coset 128
  emits [128, n), the row at position p sitting in v[p - 128].
* k > 128: the inverse transform of rows 0..127 gives P0; park; fft_rt on coset
  128 pruned to tp = k - 128 outputs gives E; v[i] = row(128 + i) ^ E[i] for
  i < tp, zero after; the solve recursion started at coset 128 with T = tp
  gives P1; v ^= park; the final transform on coset 128 with nz = 128 emits
  [k, n).

`solve_from` is fft_any_model.solve_any with a starting coset; `fft_out` is its
fft_out with the register offset and the coset apart.  The counter is
fft_any_model's; parking and reloading count as `copy` row moves.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_any_model as fam  # noqa: E402
import fft_model as fm  # noqa: E402

G = fam.G
HW = 128
Counter = fam.Counter
tw = fam.tw


def solve_from(v, logw, k, lam0, cnt):
    """v[0 .. k - lam0): evaluations at lam0 .. k-1, zeros after -> the coefficients."""
    lam, t, done = lam0, k - lam0, False
    moved = 0
    for m in range(logw, 0, -1):
        h = 1 << (m - 1)
        if done or t <= h:
            continue
        fam.ifft_rt(v, m - 1, 0, lam, cnt)
        if t == 2 * h:
            fam.ifft_rt(v, m - 1, h, lam + h, cnt)
            c = tw(m - 1, lam)
            for i in range(h):
                b = v[i] ^ v[h + i]
                v[h + i] = b
                v[i] = v[i] ^ fam.MUL[c, b]
            cnt.bfly += h
            done = True
        else:
            tp = t - h
            g = [v[i].copy() for i in range(h)]
            fam.fft_rt(g, m - 1, 0, lam + h, tp, cnt)
            for i in range(h):
                d = v[h + i] ^ g[i] if i < tp else v[h + i]
                v[h + i] = v[i]
                v[i] = d
            cnt.copy += 3 * h
            moved |= 1 << m
            lam += h
            t = tp
    for m in range(1, logw + 1):
        if not moved & (1 << m):
            continue
        h = 1 << (m - 1)
        lam_m = lam0 + ((moved & ~((2 << m) - 1)) >> 1)
        tp = k - lam_m - h
        c = tw(m - 1, lam_m)
        for i in range(h):
            p1, gi = v[i], v[h + i]
            v[h + i] = p1
            v[i] = gi ^ fam.MUL[c, p1] if i < tp else gi
        cnt.mac += tp
        cnt.copy += 2 * h


def fft_out(v, m, off, lam, nz, k, n, out, cnt):
    """The node at register offset `off` covers the positions [lam, lam + 2^m)."""
    if m >= G and (lam >= n or lam + (1 << m) <= k):
        return
    if m <= G:
        ev = fm.fft(m, lam, v[off:off + (1 << m)])
        cnt.bfly += m << (m - 1) if m else 0
        for i in range(1 << m):
            if k <= lam + i < n:
                out[lam + i] = ev[i]
        return
    h = 1 << (m - 1)
    if nz <= h:
        for i in range(h):
            v[off + h + i] = v[off + i]
        cnt.copy += h
    else:
        c = fm.twiddle(m - 1, lam)
        for i in range(h):
            b = v[off + h + i]
            a2 = v[off + i] ^ fam.MUL[c, b]
            v[off + i] = a2
            v[off + h + i] = a2 ^ b
        cnt.bfly += h
    nzc = min(nz, h)
    fft_out(v, m - 1, off, lam, nzc, k, n, out, cnt)
    fft_out(v, m - 1, off + h, lam + h, nzc, k, n, out, cnt)


def encode(k, n_total, data, cnt=None):
    """data: k rows (uint8 arrays) -> n_total rows (systematic codeword)."""
    cnt = cnt if cnt is not None else Counter()
    assert HW < n_total <= 2 * HW and 1 <= k <= n_total
    zero = np.zeros_like(data[0])
    out = [np.array(data[j]) for j in range(k)] + [None] * (n_total - k)
    v = [np.array(data[j]) if j < k else zero.copy() for j in range(HW)]
    if k <= HW:
        solve_from(v, 7, k, 0, cnt)
        assert all(not v[j].any() for j in range(k, HW)), "coefficients [k, 128) must be zero after solve"
        park = [r.copy() for r in v]
        fft_out(v, 7, 0, 0, k, k, n_total, out, cnt)
        v = [r.copy() for r in park]
        cnt.copy += 2 * HW
        nz = k
    else:
        tp = k - HW
        fam.ifft_rt(v, 7, 0, 0, cnt)  # P0
        park = [r.copy() for r in v]
        fam.fft_rt(v, 7, 0, HW, tp, cnt)  # E
        v = [np.array(data[HW + i]) ^ v[i] if i < tp else zero.copy() for i in range(HW)]
        solve_from(v, 7, k, HW, cnt)  # P1
        assert all(not v[j].any() for j in range(tp, HW)), "P1's coefficients [tp, 128) must be zero"
        v = [a ^ b for a, b in zip(v, park)]
        cnt.copy += 2 * HW
        nz = HW
    fft_out(v, 7, 0, HW, nz, k, n_total, out, cnt)
    return out


def main():
    rng = np.random.default_rng(1)
    for (n, f) in [(200, 66), (256, 85), (200, 20), (256, 32)]:
        k = n - 2 * f
        data = [rng.integers(0, 256, 8, dtype=np.uint8) for _ in range(k)]
        want = fm.orc.gf_rows(fm.orc.encode_matrix(k, n)[k:], data)
        cnt = Counter()
        got = encode(k, n, data, cnt)
        ok = all(np.array_equal(g, w) for g, w in zip(got[k:], want))
        print(f"N={n:3d} k={k:3d}: {'OK ' if ok else 'BAD'} butterflies={cnt.bfly} unwind macs={cnt.mac} "
              f"moves={cnt.copy} (matrix MACs {k * (n - k)})")


if __name__ == "__main__":
    main()
