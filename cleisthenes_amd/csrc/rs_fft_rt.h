// rs_fft_rt.h -- the additive-FFT pieces whose geometry is a run-time value:
// the butterfly constants as tables in constant memory, the transforms on a
// coset whose label is wave-uniform, the solve recursion with k as an argument
// and the final transform that skips what lies outside [k, n).  Shared by
// rs_fft_any.hip (W = 64, 128) and rs_fft_wide.hip (two 128-row halves); each
// translation unit gets its own copy of the tables.
#pragma once
#include "device_common.h"
#include "rs_fft_lch.h"

namespace {

using namespace rbcdev;

// kTw.d[tw_base(j) + c] = make_tab(W_j(c << (j+1))), padded to 8 dwords
struct TwTab {
    uint32_t d[255][8];
};
constexpr int tw_base(int j) { return 256 - (256 >> j); }
constexpr TwTab make_tw() {
    TwTab t{};
    uint32_t s[256] = {};  // s_j(x), j = 0: x
    for (uint32_t x = 0; x < 256; ++x) s[x] = x;
    for (int j = 0; j < 8; ++j) {
        const uint32_t sv = s[1u << j], inv = lch::ginv(sv);
        for (int c = 0; c < (256 >> (j + 1)); ++c) {
            const lch::Tab b = lch::make_tab(lch::gmul(s[(uint32_t)c << (j + 1)], inv));
            uint32_t(&e)[8] = t.d[tw_base(j) + c];
            e[0] = b.t0lo, e[1] = b.t0hi, e[2] = b.t1lo, e[3] = b.t1hi, e[4] = b.t2;
        }
        for (uint32_t x = 0; x < 256; ++x) s[x] = lch::gmul(s[x], s[x] ^ sv);
    }
    return t;
}
__constant__ static const TwTab kTw = make_tw();

// the tables of W_J(lam); lam is wave-uniform, so these are scalar loads
template <int J>
RBC_DEV lch::Tab tw_load(uint32_t lam) {
    const uint32_t *e = kTw.d[tw_base(J) + (lam >> (J + 1))];
    return lch::Tab{e[0], e[1], e[2], e[3], e[4]};
}

// a + c*x for 4 packed bytes, c's tables in SGPRs
RBC_DEV uint32_t mac_rt(uint32_t a, uint32_t x, const lch::Tab &t) {
    const uint32_t p0 = perm(t.t0hi, t.t0lo, x & 0x07070707u);
    const uint32_t p1 = perm(t.t1hi, t.t1lo, (x >> 3) & 0x07070707u);
    const uint32_t p2 = perm(t.t2, t.t2, (x >> 6) & 0x03030303u);
    return xor3(a, p0, p1) ^ p2;
}

using lch::IC;
using lch::sfor;

// sfor over [0, N) in chunks of 8 with a scheduling barrier between them: the
// butterflies of a layer are independent, and the scheduler would otherwise
// keep the temporaries of all of them in flight
template <int N, class F>
RBC_DEV void rows_for(F &&f) {
    sfor<0, (N + 7) / 8>([&](auto C) {
        constexpr int c = decltype(C)::value;
        sfor<8 * c, (8 * c + 8 < N ? 8 * c + 8 : N)>(f);
        if constexpr (N > 8) __builtin_amdgcn_sched_barrier(0);
    });
}

constexpr int G = 3;  // sub-transforms of 2^G rows are skipped or stored as a group
// run-time transforms of >= 2^SBR rows are scheduled one after the other: each (layer, coset) group
// holds five table SGPRs, and the scheduler would otherwise fetch the tables of many groups ahead
constexpr int SBR = 3;

// Inverse transform of v[OFF .. OFF+2^M) on coset lam + V_M, in place.
template <int M, int OFF, int R>
RBC_DEV void ifft_rt(uint32_t (&v)[R], uint32_t lam) {
    if constexpr (M > 0) {
        constexpr int H = 1 << (M - 1);
        ifft_rt<M - 1, OFF>(v, lam);
        // keep the scheduler from interleaving independent sub-transforms: their
        // temporaries and table registers would add up (rs_fft_lch.h's fft)
        if constexpr (M >= SBR) __builtin_amdgcn_sched_barrier(0);
        ifft_rt<M - 1, OFF + H>(v, lam + H);
        if constexpr (M >= SBR) __builtin_amdgcn_sched_barrier(0);
        const lch::Tab t = tw_load<M - 1>(lam);
        rows_for<H>([&](auto I) {
            constexpr int i = decltype(I)::value;
            const uint32_t b = v[OFF + i] ^ v[OFF + H + i];
            v[OFF + H + i] = b;
            v[OFF + i] = mac_rt(v[OFF + i], b, t);
        });
    }
}

// Evaluations on coset lam + V_M of the polynomial with novel coefficients
// v[OFF .. OFF+2^M), in place.  Only the outputs v[0 .. tp) of the whole array
// are needed: a sub-transform of >= 2^G rows that starts at or past tp is skipped.
template <int M, int OFF, int R>
RBC_DEV void fft_rt(uint32_t (&v)[R], uint32_t lam, int tp) {
    if constexpr (M > 0) {
        if constexpr (M >= G && OFF > 0) {
            if (OFF >= tp) return;
        }
        constexpr int H = 1 << (M - 1);
        const lch::Tab t = tw_load<M - 1>(lam);
        rows_for<H>([&](auto I) {
            constexpr int i = decltype(I)::value;
            const uint32_t b = v[OFF + H + i], a2 = mac_rt(v[OFF + i], b, t);
            v[OFF + i] = a2;
            v[OFF + H + i] = a2 ^ b;
        });
        if constexpr (M >= SBR) __builtin_amdgcn_sched_barrier(0);
        fft_rt<M - 1, OFF>(v, lam, tp);
        if constexpr (M >= SBR) __builtin_amdgcn_sched_barrier(0);
        fft_rt<M - 1, OFF + H>(v, lam + H, tp);
    }
}

// v[0 .. k - lam0) hold the evaluations at lam0 .. k-1 of a polynomial with fewer than k - lam0
// novel coefficients (lam0 a multiple of W; 0: the data rows), the rows after them zeros; on
// return v[0 .. k - lam0) hold those coefficients, the rows after them zeros.
template <int LOGW>
RBC_DEV void solve_any(uint32_t (&v)[1 << LOGW], int k, uint32_t lam0 = 0) {
    // bit M of moved: the recursion moved to the upper half at level M.  The coset label is lam0 plus
    // the halves 2^(M-1) it moved by, and T = k - lam rows of the active block are known.
    uint32_t lam = lam0, moved = 0;
    int T = k - (int)lam0;
    bool done = false;
    sfor<0, LOGW>([&](auto L) {
        constexpr int M = LOGW - decltype(L)::value, H = 1 << (M - 1);
        if (!done && T > H) {
            ifft_rt<M - 1, 0>(v, lam);
            __builtin_amdgcn_sched_barrier(0);
            if (T == 2 * H) {  // the whole block is known: finish its inverse transform
                ifft_rt<M - 1, H>(v, lam + H);
                __builtin_amdgcn_sched_barrier(0);
                const lch::Tab t = tw_load<M - 1>(lam);
                rows_for<H>([&](auto I) {
                    constexpr int i = decltype(I)::value;
                    const uint32_t b = v[i] ^ v[H + i];
                    v[H + i] = b;
                    v[i] = mac_rt(v[i], b, t);
                });
                done = true;
            } else {
                // v[0 .. H) = g = P0 + w P1.  d = upper rows - FFT_{lam+H}(g)[0 .. tp)
                // = FFT_{lam+H}(P1)[0 .. tp) goes to the front, g to the back.
                const int tp = T - H;
                uint32_t g[H];
                sfor<0, H>([&](auto I) { g[decltype(I)::value] = v[decltype(I)::value]; });
                fft_rt<M - 1, 0>(g, lam + H, tp);
                __builtin_amdgcn_sched_barrier(0);
                rows_for<H>([&](auto I) {
                    constexpr int i = decltype(I)::value;
                    const uint32_t d = v[H + i] ^ (i < tp ? g[i] : 0u);
                    v[H + i] = v[i];
                    v[i] = d;
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
            const uint32_t lam_m = lam0 + ((moved & ~((2u << M) - 1u)) >> 1);  // the levels above M that moved
            const lch::Tab t = tw_load<M - 1>(lam_m);
            const int tp = k - (int)lam_m - H;
            rows_for<H>([&](auto I) {
                constexpr int i = decltype(I)::value;
                const uint32_t p1 = v[i], gi = v[H + i];
                v[H + i] = p1;
                v[i] = i < tp ? mac_rt(gi, p1, t) : gi;  // P0 = g + w P1
            });
        }
    });
}

// The final transform: evaluations at LAM .. LAM + 2^M - 1 of the polynomial
// with novel coefficients v[OFF .. OFF + 2^M), of which the first nz are
// nonzero; the node covers the outputs [LAM, LAM + 2^M) and leaves them in the
// registers its coefficients had.  Nodes of >= 2^G rows outside [k, n) are
// skipped; a finished 2^G-row group is handed to st(IC<OFF>).
template <int M, int OFF, int LAM = OFF, int R, class ST>
RBC_DEV void fft_out(uint32_t (&v)[R], int nz, int k, int n, ST &st) {
    if constexpr (M >= G) {
        if (LAM >= n || LAM + (1 << M) <= k) return;
    }
    if constexpr (M <= G) {
        lch::fft_full<M, LAM, OFF, (1 << M)>(v);
        st(IC<OFF>{});
    } else {
        constexpr int H = 1 << (M - 1);
        constexpr uint32_t w = lch::twiddle(M - 1, LAM);
        if (nz <= H) {  // the upper coefficients are all zero
            sfor<0, H>([&](auto I) { v[OFF + H + decltype(I)::value] = v[OFF + decltype(I)::value]; });
        } else {
            const lch::TR tr = lch::tab_regs<w>();
            rows_for<H>([&](auto I) {
                constexpr int i = decltype(I)::value;
                const uint32_t b = v[OFF + H + i], a2 = lch::mac<w>(v[OFF + i], b, tr);
                v[OFF + i] = a2;
                v[OFF + H + i] = a2 ^ b;
            });
        }
        const int nzc = nz < H ? nz : H;
        fft_out<M - 1, OFF, LAM>(v, nzc, k, n, st);
        // keep the scheduler from interleaving the two independent halves
        if constexpr (M >= SBR) __builtin_amdgcn_sched_barrier(0);
        fft_out<M - 1, OFF + H, LAM + H>(v, nzc, k, n, st);
    }
}

RBC_DEV uint32_t keep_bytes4(int nv) { return nv >= 4 ? 0xffffffffu : (nv <= 0 ? 0u : ((1u << (8 * nv)) - 1u)); }

// blockIdx -> (tile_x, tile_y) in the XCD-aware order of rs_fft_kernel: consecutive blocks go
// round the 8 XCDs, so each XCD gets a contiguous run of tiles
RBC_DEV void xcd_tile(uint32_t &tile_x, uint32_t &tile_y) {
    const uint32_t gx = gridDim.x, total = gx * gridDim.y, t8 = total & ~7u;
    uint32_t lin = blockIdx.y * gx + blockIdx.x;
    if (lin < t8) lin = (lin & 7u) * (t8 >> 3) + (lin >> 3);
    tile_y = lin / gx;
    tile_x = lin - tile_y * gx;
}

}  // namespace
