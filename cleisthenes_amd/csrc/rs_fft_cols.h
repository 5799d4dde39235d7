// rs_fft_cols.h -- rs_fft_rt.h's run-time-geometry pieces for a lane that owns CW adjacent dword
// columns of every row: the rows are v[R][CW], every butterfly runs on the CW dwords of its two
// rows, and what is fetched or built once per (layer, coset) group -- the five-dword scalar table
// of an inner transform, the literal table registers of the final one -- serves all CW columns.
// CW = 1 is rs_fft_rt.h's arithmetic, instruction for instruction.  The recursions are the same
// (tests/fft_any_model.py); they are restated here, not generalised in place, so that rs_fft_rt.h
// and with it the kernels of rs_fft_any.hip and rs_fft_wide.hip stay as they are.  Used by
// rs_fft_small.hip (W = 8, 16, 32).
#pragma once
#include "rs_fft_rt.h"

namespace {

// sfor over [0, N) rows with a scheduling barrier after every 8 butterflies (rows_for)
template <int N, int CW, class F>
RBC_DEV void rows_for_c(F &&f) {
    constexpr int CH = CW >= 8 ? 1 : 8 / CW;  // rows per chunk
    sfor<0, (N + CH - 1) / CH>([&](auto C) {
        constexpr int c = decltype(C)::value;
        sfor<CH * c, (CH * c + CH < N ? CH * c + CH : N)>(f);
        if constexpr (N > CH) __builtin_amdgcn_sched_barrier(0);
    });
}

// ifft_rt on v[OFF .. OFF+2^M)[CW]
template <int M, int OFF, int R, int CW>
RBC_DEV void ifft_c(uint32_t (&v)[R][CW], uint32_t lam) {
    if constexpr (M > 0) {
        constexpr int H = 1 << (M - 1);
        ifft_c<M - 1, OFF>(v, lam);
        if constexpr (M >= SBR) __builtin_amdgcn_sched_barrier(0);
        ifft_c<M - 1, OFF + H>(v, lam + H);
        if constexpr (M >= SBR) __builtin_amdgcn_sched_barrier(0);
        const lch::Tab t = tw_load<M - 1>(lam);
        rows_for_c<H, CW>([&](auto I) {
            constexpr int i = decltype(I)::value;
            sfor<0, CW>([&](auto C) {
                constexpr int c = decltype(C)::value;
                const uint32_t b = v[OFF + i][c] ^ v[OFF + H + i][c];
                v[OFF + H + i][c] = b;
                v[OFF + i][c] = mac_rt(v[OFF + i][c], b, t);
            });
        });
    }
}

// fft_rt on v[OFF .. OFF+2^M)[CW]: only the outputs v[0 .. tp) of the whole array are needed
template <int M, int OFF, int R, int CW>
RBC_DEV void fft_c(uint32_t (&v)[R][CW], uint32_t lam, int tp) {
    if constexpr (M > 0) {
        if constexpr (M >= G && OFF > 0) {
            if (OFF >= tp) return;
        }
        constexpr int H = 1 << (M - 1);
        const lch::Tab t = tw_load<M - 1>(lam);
        rows_for_c<H, CW>([&](auto I) {
            constexpr int i = decltype(I)::value;
            sfor<0, CW>([&](auto C) {
                constexpr int c = decltype(C)::value;
                const uint32_t b = v[OFF + H + i][c], a2 = mac_rt(v[OFF + i][c], b, t);
                v[OFF + i][c] = a2;
                v[OFF + H + i][c] = a2 ^ b;
            });
        });
        if constexpr (M >= SBR) __builtin_amdgcn_sched_barrier(0);
        fft_c<M - 1, OFF>(v, lam, tp);
        if constexpr (M >= SBR) __builtin_amdgcn_sched_barrier(0);
        fft_c<M - 1, OFF + H>(v, lam + H, tp);
    }
}

// solve_any at coset 0 on v[2^LOGW][CW]: v[0 .. k) the data rows, the rows after them zeros; on
// return v[0 .. k) hold the novel coefficients, the rows after them zeros.
template <int LOGW, int CW>
RBC_DEV void solve_c(uint32_t (&v)[1 << LOGW][CW], int k) {
    uint32_t lam = 0, moved = 0;  // solve_any's: the coset label, the levels that moved up
    int T = k;
    bool done = false;
    sfor<0, LOGW>([&](auto L) {
        constexpr int M = LOGW - decltype(L)::value, H = 1 << (M - 1);
        if (!done && T > H) {
            ifft_c<M - 1, 0>(v, lam);
            __builtin_amdgcn_sched_barrier(0);
            if (T == 2 * H) {  // the whole block is known: finish its inverse transform
                ifft_c<M - 1, H>(v, lam + H);
                __builtin_amdgcn_sched_barrier(0);
                const lch::Tab t = tw_load<M - 1>(lam);
                rows_for_c<H, CW>([&](auto I) {
                    constexpr int i = decltype(I)::value;
                    sfor<0, CW>([&](auto C) {
                        constexpr int c = decltype(C)::value;
                        const uint32_t b = v[i][c] ^ v[H + i][c];
                        v[H + i][c] = b;
                        v[i][c] = mac_rt(v[i][c], b, t);
                    });
                });
                done = true;
            } else {
                // v[0 .. H) = g = P0 + w P1.  d = upper rows - FFT_{lam+H}(g)[0 .. tp) goes to the
                // front, g to the back.
                const int tp = T - H;
                uint32_t g[H][CW];
                sfor<0, H>([&](auto I) {
                    sfor<0, CW>([&](auto C) { g[decltype(I)::value][decltype(C)::value] = v[decltype(I)::value][decltype(C)::value]; });
                });
                fft_c<M - 1, 0>(g, lam + H, tp);
                __builtin_amdgcn_sched_barrier(0);
                rows_for_c<H, CW>([&](auto I) {
                    constexpr int i = decltype(I)::value;
                    sfor<0, CW>([&](auto C) {
                        constexpr int c = decltype(C)::value;
                        const uint32_t d = v[H + i][c] ^ (i < tp ? g[i][c] : 0u);
                        v[H + i][c] = v[i][c];
                        v[i][c] = d;
                    });
                });
                moved |= 1u << M;
                lam += H;
                T = tp;
            }
        }
    });
    sfor<1, LOGW + 1>([&](auto MM) {
        constexpr int M = decltype(MM)::value, H = 1 << (M - 1);
        if (moved & (1u << M)) {  // v[0 .. H) = P1 (zeros from tp on), v[H .. 2H) = g
            const uint32_t lam_m = (moved & ~((2u << M) - 1u)) >> 1;  // the levels above M that moved
            const lch::Tab t = tw_load<M - 1>(lam_m);
            const int tp = k - (int)lam_m - H;
            rows_for_c<H, CW>([&](auto I) {
                constexpr int i = decltype(I)::value;
                sfor<0, CW>([&](auto C) {
                    constexpr int c = decltype(C)::value;
                    const uint32_t p1 = v[i][c], gi = v[H + i][c];
                    v[H + i][c] = p1;
                    v[i][c] = i < tp ? mac_rt(gi, p1, t) : gi;  // P0 = g + w P1
                });
            });
        }
    });
}

// lch::fft_full with every coefficient nonzero: all 2^M evaluations on coset LAM + V_M, in place
template <int M, int LAM, int OFF, int R, int CW>
RBC_DEV void fft_full_c(uint32_t (&v)[R][CW]) {
    if constexpr (M > 0) {
        constexpr int H = 1 << (M - 1);
        constexpr uint32_t w = lch::twiddle(M - 1, LAM);
        const lch::TR tr = lch::tab_regs<w>();
        sfor<0, H>([&](auto I) {
            constexpr int i = decltype(I)::value;
            sfor<0, CW>([&](auto C) {
                constexpr int c = decltype(C)::value;
                const uint32_t b = v[OFF + H + i][c], a2 = lch::mac<w>(v[OFF + i][c], b, tr);
                v[OFF + i][c] = a2;
                v[OFF + H + i][c] = a2 ^ b;
            });
        });
        fft_full_c<M - 1, LAM, OFF>(v);
        fft_full_c<M - 1, LAM + H, OFF + H>(v);
    }
}

// fft_out at coset 0 (LAM = OFF) on v[R][CW]
template <int M, int OFF, int R, int CW, class ST>
RBC_DEV void fft_out_c(uint32_t (&v)[R][CW], int nz, int k, int n, ST &st) {
    if constexpr (M >= G) {
        if (OFF >= n || OFF + (1 << M) <= k) return;
    }
    if constexpr (M <= G) {
        fft_full_c<M, OFF, OFF>(v);
        st(IC<OFF>{});
    } else {
        constexpr int H = 1 << (M - 1);
        constexpr uint32_t w = lch::twiddle(M - 1, OFF);
        if (nz <= H) {  // the upper coefficients are all zero
            sfor<0, H>([&](auto I) {
                sfor<0, CW>([&](auto C) {
                    v[OFF + H + decltype(I)::value][decltype(C)::value] = v[OFF + decltype(I)::value][decltype(C)::value];
                });
            });
        } else {
            const lch::TR tr = lch::tab_regs<w>();
            rows_for_c<H, CW>([&](auto I) {
                constexpr int i = decltype(I)::value;
                sfor<0, CW>([&](auto C) {
                    constexpr int c = decltype(C)::value;
                    const uint32_t b = v[OFF + H + i][c], a2 = lch::mac<w>(v[OFF + i][c], b, tr);
                    v[OFF + i][c] = a2;
                    v[OFF + H + i][c] = a2 ^ b;
                });
            });
        }
        const int nzc = nz < H ? nz : H;
        fft_out_c<M - 1, OFF>(v, nzc, k, n, st);
        if constexpr (M >= SBR) __builtin_amdgcn_sched_barrier(0);
        fft_out_c<M - 1, OFF + H>(v, nzc, k, n, st);
    }
}

}  // namespace
