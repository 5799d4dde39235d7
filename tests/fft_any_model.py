#!/usr/bin/env python3
"""Python model of `rs_fft_any_kernel` (csrc/rs_fft_any.hip): the additive-FFT
Reed-Solomon encoder of fft_model.py with n and k at run time (test
infrastructure: pins the kernel's structure against the oracle on the CPU).

It does what the kernel does, step by step, on a list `v` of W = 2^LOGW rows:

* solve.  The levels M = LOGW..1 are walked from the top.  With T rows of the
  active block of 2^M known: T == 2^M finishes with an inverse transform;
  T <= 2^(M-1) goes one level down; else the lower half is inverted to g, the
  first tp = T - 2^(M-1) outputs of FFT(g) on the upper coset are subtracted
  from the upper rows, and the halves trade places so that the active block
  stays at row 0.  The levels that moved are unwound in reverse: swap back,
  P0 = g + w P1 on the first tp rows.
* The inner transforms take their constants from TW, the table the kernel holds
  in constant memory: TW[tw_base(j) + (lam >> (j+1))] = W_j(lam).
* Rows [T, 2^M) of the active block stay zero throughout, so the coefficients
  [k, W) are zero after solve (asserted here, relied on by the kernel).
* The final transform at coset 0 skips every sub-transform of >= 2^G rows whose
  outputs lie outside [k, n), and copies where a layer's upper inputs are zero.

Counter: `bfly` butterflies (one constant multiply each), `mac` the multiplies
of the unwinding, `copy` row moves (swaps, zero-input layers).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_model as fm  # noqa: E402  (the field tables)

MUL = fm.MUL
G = 3  # rs_fft_any.hip's G


def tw_base(j):
    return 256 - (256 >> j)


TW = [0] * 255
for _j in range(8):
    for _c in range(256 >> (_j + 1)):
        TW[tw_base(_j) + _c] = fm.twiddle(_j, _c << (_j + 1))


def tw(j, lam):
    return TW[tw_base(j) + (lam >> (j + 1))]


class Counter:
    def __init__(self):
        self.bfly = 0
        self.mac = 0
        self.copy = 0

    @property
    def mul(self):
        return self.bfly + self.mac


def _mac(a, x, c):
    return a ^ MUL[c, x]


def ifft_rt(v, m, off, lam, cnt):
    if m == 0:
        return
    h = 1 << (m - 1)
    ifft_rt(v, m - 1, off, lam, cnt)
    ifft_rt(v, m - 1, off + h, lam + h, cnt)
    c = tw(m - 1, lam)
    for i in range(h):
        b = v[off + i] ^ v[off + h + i]
        v[off + h + i] = b
        v[off + i] = _mac(v[off + i], b, c)
    cnt.bfly += h


def fft_rt(v, m, off, lam, tp, cnt):
    if m == 0:
        return
    if m >= G and off > 0 and off >= tp:
        return
    h = 1 << (m - 1)
    c = tw(m - 1, lam)
    for i in range(h):
        b = v[off + h + i]
        a2 = _mac(v[off + i], b, c)
        v[off + i] = a2
        v[off + h + i] = a2 ^ b
    cnt.bfly += h
    fft_rt(v, m - 1, off, lam, tp, cnt)
    fft_rt(v, m - 1, off + h, lam + h, tp, cnt)


def solve_any(v, logw, k, cnt):
    lam, t, done = 0, k, False
    moved = 0  # bit M: the recursion moved up at level M (lam and tp follow from it and k)
    for m in range(logw, 0, -1):
        h = 1 << (m - 1)
        if done or t <= h:
            continue
        ifft_rt(v, m - 1, 0, lam, cnt)
        if t == 2 * h:
            ifft_rt(v, m - 1, h, lam + h, cnt)
            c = tw(m - 1, lam)
            for i in range(h):
                b = v[i] ^ v[h + i]
                v[h + i] = b
                v[i] = _mac(v[i], b, c)
            cnt.bfly += h
            done = True
        else:
            tp = t - h
            g = [v[i].copy() for i in range(h)]
            fft_rt(g, m - 1, 0, lam + h, tp, cnt)
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
        lam_m = (moved & ~((2 << m) - 1)) >> 1
        tp = k - lam_m - h
        c = tw(m - 1, lam_m)
        for i in range(h):
            p1, gi = v[i], v[h + i]
            v[h + i] = p1
            v[i] = _mac(gi, p1, c) if i < tp else gi
        cnt.mac += tp
        cnt.copy += 2 * h


def fft_out(v, m, off, nz, k, n, out, cnt):
    if m >= G and (off >= n or off + (1 << m) <= k):
        return
    if m <= G:
        ev = fm.fft(m, off, v[off:off + (1 << m)])
        cnt.bfly += m << (m - 1) if m else 0
        for i in range(1 << m):
            if k <= off + i < n:
                out[off + i] = ev[i]
        return
    h = 1 << (m - 1)
    if nz <= h:
        for i in range(h):
            v[off + h + i] = v[off + i]
        cnt.copy += h
    else:
        c = fm.twiddle(m - 1, off)
        for i in range(h):
            b = v[off + h + i]
            a2 = _mac(v[off + i], b, c)
            v[off + i] = a2
            v[off + h + i] = a2 ^ b
        cnt.bfly += h
    nzc = min(nz, h)
    fft_out(v, m - 1, off, nzc, k, n, out, cnt)
    fft_out(v, m - 1, off + h, nzc, k, n, out, cnt)


def width_log2(n_total):
    """LOGW of the kernel that runs n_total (33 <= n_total <= 256)."""
    return (n_total - 1).bit_length()


def encode(k, n_total, data, cnt=None):
    """data: k rows (uint8 arrays) -> n_total rows (systematic codeword)."""
    cnt = cnt if cnt is not None else Counter()
    logw = width_log2(n_total)
    w = 1 << logw
    assert 1 <= k <= n_total <= w < 2 * n_total
    zero = np.zeros_like(data[0])
    v = [np.array(data[j]) if j < k else zero.copy() for j in range(w)]
    solve_any(v, logw, k, cnt)
    assert all(not v[j].any() for j in range(k, w)), "coefficients [k, W) must be zero after solve"
    out = [np.array(data[j]) for j in range(k)] + [None] * (n_total - k)
    fft_out(v, logw, 0, k, k, n_total, out, cnt)
    return out


def main():
    rng = np.random.default_rng(1)
    for (n, f) in [(64, 20), (100, 33), (128, 30), (128, 42), (200, 66), (256, 85)]:
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
