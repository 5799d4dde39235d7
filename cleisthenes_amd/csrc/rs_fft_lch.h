// rs_fft_lch.h -- the Lin-Chung-Han additive FFT over GF(2^8)/0x11D as device
// templates: field arithmetic and butterfly constants at compile time, the
// constant multiply of 4 packed bytes, and the unrolled transforms.  Shared by
// rs_fft.hip (one kernel per geometry) and, through rs_fft_rt.h, rs_fft_any.hip and
// rs_fft_wide.hip (n and k at run time).
#pragma once
#include <utility>

#include "device_common.h"

namespace lch {

using rbcdev::perm;
using rbcdev::xor3;

constexpr uint32_t gmul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 0; i < 8; ++i) {
        if (b & 1u) r ^= a;
        b >>= 1;
        a <<= 1;
        if (a & 0x100u) a ^= 0x11du;
    }
    return r;
}
constexpr uint32_t ginv(uint32_t a) {
    uint32_t r = 1, e = 254;  // a^254 = a^-1
    while (e) {
        if (e & 1u) r = gmul(r, a);
        a = gmul(a, a);
        e >>= 1;
    }
    return r;
}
// s_j(x): vanishing polynomial of V_j = span{1..2^(j-1)}; linearized, so
// s_{j+1}(x) = s_j(x) * (s_j(x) + s_j(2^j)).
constexpr uint32_t s_eval(int j, uint32_t x) {
    if (j == 0) return x;
    const uint32_t a = s_eval(j - 1, x);
    return gmul(a, a ^ s_eval(j - 1, 1u << (j - 1)));
}
// butterfly constant of layer j on coset lambda: W_j(lambda)
constexpr uint32_t twiddle(int j, uint32_t lam) { return gmul(s_eval(j, lam), ginv(s_eval(j, 1u << j))); }

struct Tab {
    uint32_t t0lo, t0hi, t1lo, t1hi, t2;
};
constexpr Tab make_tab(uint32_t c) {
    uint32_t m[8] = {};
    m[0] = c;
    for (int i = 1; i < 8; ++i) m[i] = gmul(m[i - 1], 2);
    Tab t{};
    t.t0lo = (m[0] << 8) | (m[1] << 16) | ((m[0] ^ m[1]) << 24);
    t.t0hi = m[2] | ((m[2] ^ m[0]) << 8) | ((m[2] ^ m[1]) << 16) | ((m[2] ^ m[1] ^ m[0]) << 24);
    t.t1lo = (m[3] << 8) | (m[4] << 16) | ((m[3] ^ m[4]) << 24);
    t.t1hi = m[5] | ((m[5] ^ m[3]) << 8) | ((m[5] ^ m[4]) << 16) | ((m[5] ^ m[4] ^ m[3]) << 24);
    t.t2 = (m[6] << 8) | (m[7] << 16) | ((m[6] ^ m[7]) << 24);
    return t;
}

// Per-group table registers.  gfx950 VOP3 reads one scalar operand, so one
// half of each 8-entry table must sit in a VGPR; all butterflies of one
// (layer, coset) group share the constant, so the two halves are
// materialised once per group (volatile: never CSE'd into a kernel-long
// register, which would cost occupancy) and the other half plus t2 ride in
// SGPRs.
struct TR {
    uint32_t lo0, lo1;
};
template <uint32_t C>
RBC_DEV TR tab_regs() {
    TR r{0u, 0u};
    if constexpr (C > 1) {
        constexpr Tab t = make_tab(C);
        asm volatile("v_mov_b32 %0, %1" : "=v"(r.lo0) : "i"(t.t0lo));
        asm volatile("v_mov_b32 %0, %1" : "=v"(r.lo1) : "i"(t.t1lo));
    }
    return r;
}

// a + C*x for 4 packed bytes (C compile-time, tables from tab_regs<C>())
template <uint32_t C>
RBC_DEV uint32_t mac(uint32_t a, uint32_t x, const TR &r) {
    if constexpr (C == 0) {
        return a;
    } else if constexpr (C == 1) {
        return a ^ x;
    } else {
        constexpr Tab t = make_tab(C);
        const uint32_t p0 = perm(t.t0hi, r.lo0, x & 0x07070707u);
        const uint32_t p1 = perm(t.t1hi, r.lo1, (x >> 3) & 0x07070707u);
        const uint32_t p2 = perm(t.t2, t.t2, (x >> 6) & 0x03030303u);
        return xor3(a, p0, p1) ^ p2;
    }
}

template <int B, int E, class F>
RBC_DEV void sfor(F &&f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        sfor<B + 1, E>(f);
    }
}

constexpr int cmin(int a, int b) { return a < b ? a : b; }
constexpr int cmax(int a, int b) { return a > b ? a : b; }

template <int V>
using IC = std::integral_constant<int, V>;

constexpr int SB = 4;  // sub-transforms of >= 2^SB rows are scheduled one after the other

// All 2^M evaluations on coset LAM + V_M, in place, of the polynomial whose
// novel coefficients are v[OFF .. OFF+2^M) (rows >= NZ are zero, never read).
template <int M, int LAM, int OFF, int NZ, int R>
RBC_DEV void fft_full(uint32_t (&v)[R]) {
    if constexpr (NZ <= 0) {
        sfor<0, (1 << M)>([&](auto I) { v[OFF + decltype(I)::value] = 0u; });
    } else if constexpr (M > 0) {
        constexpr int H = 1 << (M - 1);
        constexpr uint32_t w = twiddle(M - 1, LAM);
        constexpr int NZA = cmin(NZ, H), NZB = cmax(NZ - H, 0);
        const TR tr = NZB > 0 ? tab_regs<w>() : TR{0u, 0u};
        sfor<0, H>([&](auto I) {
            constexpr int i = decltype(I)::value;
            if constexpr (i < NZB) {
                const uint32_t a = v[OFF + i], b = v[OFF + H + i];
                const uint32_t a2 = mac<w>(a, b, tr);
                v[OFF + i] = a2;
                v[OFF + H + i] = a2 ^ b;
            } else if constexpr (i < NZA) {
                v[OFF + H + i] = v[OFF + i];  // b == 0
            }
        });
        fft_full<M - 1, LAM, OFF, NZA>(v);
        fft_full<M - 1, LAM + H, OFF + H, NZA>(v);
    }
}

// Evaluations on coset LAM + V_M of the polynomial whose novel coefficients are
// v[OFF .. OFF+2^M) (rows >= NZ are zero and never read).  Only the outputs
// with local index in [LO, HI) are needed.  Sub-transforms of size 2^G are
// completed in place and handed over as a group, st(IC<lam>, IC<off>, IC<lo>,
// IC<hi>): outputs v[off + lo .. off + hi) are the evaluations at lam + i --
// so a sink can batch its memory traffic per group.
template <int G, int M, int LAM, int OFF, int NZ, int LO, int HI, int R, class ST>
RBC_DEV void fft(uint32_t (&v)[R], ST &st) {
    if constexpr (LO >= HI) {
        return;
    } else if constexpr (M <= G) {
        fft_full<M, LAM, OFF, NZ>(v);
        st(IC<LAM>{}, IC<OFF>{}, IC<LO>{}, IC<HI>{});
    } else {
        constexpr int H = 1 << (M - 1);
        constexpr uint32_t w = twiddle(M - 1, LAM);
        constexpr int NZA = cmin(NZ, H), NZB = cmax(NZ - H, 0);
        constexpr bool needA = LO < H, needB = HI > H;
        constexpr uint32_t wt = needA ? w : (w ^ 1u);  // needB only: b' = a + (w+1) b
        const TR tr = NZB > 0 ? tab_regs<wt>() : TR{0u, 0u};
        sfor<0, H>([&](auto I) {
            constexpr int i = decltype(I)::value;
            if constexpr (i < NZB) {
                const uint32_t a = v[OFF + i], b = v[OFF + H + i];
                if constexpr (needA && needB) {
                    const uint32_t a2 = mac<wt>(a, b, tr);
                    v[OFF + i] = a2;
                    v[OFF + H + i] = a2 ^ b;
                } else if constexpr (needA) {
                    v[OFF + i] = mac<wt>(a, b, tr);
                } else {
                    v[OFF + H + i] = mac<wt>(a, b, tr);  // a + (w+1) b
                }
            } else if constexpr (i < NZA && needB) {
                v[OFF + H + i] = v[OFF + i];  // b == 0
            }
        });
        if constexpr (needA) fft<G, M - 1, LAM, OFF, NZA, LO, cmin(HI, H)>(v, st);
        // keep the scheduler from interleaving the two independent halves
        // (that would double the live rows and halve occupancy)
        if constexpr (needA && needB && M >= SB) __builtin_amdgcn_sched_barrier(0);
        if constexpr (needB) fft<G, M - 1, LAM + H, OFF + H, NZA, cmax(LO - H, 0), HI - H>(v, st);
    }
}

// Inverse transform on coset LAM + V_M, in place (all 2^M rows known).
template <int M, int LAM, int OFF, int R>
RBC_DEV void ifft(uint32_t (&v)[R]) {
    if constexpr (M > 0) {
        constexpr int H = 1 << (M - 1);
        ifft<M - 1, LAM, OFF>(v);
        ifft<M - 1, LAM + H, OFF + H>(v);
        constexpr uint32_t w = twiddle(M - 1, LAM);
        const TR tr = tab_regs<w>();
        sfor<0, H>([&](auto I) {
            constexpr int i = decltype(I)::value;
            const uint32_t b = v[OFF + i] ^ v[OFF + H + i];
            v[OFF + H + i] = b;
            v[OFF + i] = mac<w>(v[OFF + i], b, tr);
        });
    }
}

// Rows v[OFF .. OFF+T) hold the evaluations at the first T points of
// LAM + V_M of a polynomial with novel-coefficient support [0, T); on return
// they hold those coefficients (rows [T, 2^M) are zero by construction).
template <int M, int LAM, int OFF, int T, int R>
RBC_DEV void solve(uint32_t (&v)[R]) {
    constexpr int SZ = 1 << M;
    if constexpr (T == SZ) {
        ifft<M, LAM, OFF>(v);
    } else if constexpr (T <= SZ / 2) {
        solve<M - 1, LAM, OFF, T>(v);
    } else {
        constexpr int H = SZ / 2, TP = T - H;
        constexpr uint32_t w = twiddle(M - 1, LAM);
        ifft<M - 1, LAM, OFF>(v);  // g = P0 + w P1
        // d = vals[H..T) - FFT_{LAM+H}(g)[0..TP) = FFT_{LAM+H}(P1)[0..TP)
        uint32_t g[H];
        sfor<0, H>([&](auto I) { g[decltype(I)::value] = v[OFF + decltype(I)::value]; });
        auto sub = [&](auto Lam, auto Off, auto Lo, auto Hi) {
            sfor<decltype(Lo)::value, decltype(Hi)::value>([&](auto I) {
                constexpr int i = decltype(I)::value;
                v[OFF + H + decltype(Lam)::value - (LAM + H) + i] ^= g[decltype(Off)::value + i];
            });
        };
        fft<0, M - 1, LAM + H, 0, H, 0, TP>(g, sub);
        solve<M - 1, LAM + H, OFF + H, TP>(v);  // P1
        const TR tr = tab_regs<w>();
        sfor<0, TP>([&](auto I) {              // P0 = g + w P1
            constexpr int i = decltype(I)::value;
            v[OFF + i] = mac<w>(v[OFF + i], v[OFF + H + i], tr);
        });
    }
}

}  // namespace lch
