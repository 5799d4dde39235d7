// rs_fft_any.hip -- the additive-FFT Reed-Solomon codec of rs_fft.hip with the
// geometry at run time: one kernel per transform width W = 2^LOGW (the smallest
// power of two >= n, so 2n > W) and per mode, n and k as kernel arguments.  It
// computes the same linear map as rs_fft_kernel<LOGW, K, N> and as the matrix
// codec (rs_fft.hip's header), byte for byte, and follows the same launch
// contract (FftArgs) except the fused value join, which it does not have: the
// launcher refuses a.join, and the host stage leaves the join to join_kernel.
// Model and butterfly counts: tests/fft_any_model.py.
//
// What stays as in the specialised kernel: one lane owns one dword column of
// every row of one instance, the W rows live in VGPRs under static indices, and
// every branch is wave-uniform (k and n are kernel arguments).  What changes:
//
//   * solve.  Its recursion depends on k through three cases per level M
//     (T rows known of a block of 2^M): T == 2^M, an inverse transform;
//     T <= 2^(M-1), descend into the lower half; else the lower half is
//     inverted to g = P0 + w P1, FFT(g) on the upper coset is subtracted from
//     the upper rows and the recursion moves there.  The levels M = LOGW..1
//     are unrolled; when the recursion moves up, the halves trade places (the
//     subtraction and the swap are one pass), so the active block always
//     starts at register 0.  The levels that moved are remembered in a scalar
//     mask and unwound in reverse: swap back, P0 = g + w P1.
//   * Inner transforms run on a coset whose label is a run-time value; their
//     constants W_j(lambda) come from kTw, the five perm tables of make_tab
//     for each of the 255 (layer j, lambda >> (j+1)) pairs, fetched by scalar
//     loads (the index is wave-uniform).
//   * Rows [T, 2^M) of the active block are zero at every level: the rows
//     [k, W) start as zeros, FFT(g) is subtracted from the first T - 2^(M-1)
//     upper rows only, and the swaps move whole halves.  So the coefficients
//     [k, W) are zero after solve without a pass that clears them.
//   * The final transform sits at coset 0 and keeps compile-time constants.
//     It skips, behind uniform branches, every sub-transform whose outputs lie
//     outside [k, n), and turns a layer whose upper inputs are all zero
//     (k <= half) into copies.
//
// Built for W = 64 and W = 128 (33 <= n <= 128).  W = 256 is left out: with 256
// rows and the 128-row copy of g resident it does not fit the 512 registers of a
// lone wave without scratch (100 - 250 bytes a lane), so n > 128
// keeps the specialised transform or the matrix codec.  W = 128 takes 256 VGPRs
// and a few AGPRs, one wave per SIMD; W = 64 132 VGPRs.
#include "device_common.h"
#include "host_shared.h"
#include "kernels.h"
#include "rs_fft_lch.h"

using namespace rbcdev;

namespace {

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

// v[0 .. k) hold the data rows (the evaluations at 0..k-1), v[k .. W) zeros; on
// return v[0 .. k) hold the novel coefficients of the polynomial, v[k .. W) zeros.
template <int LOGW>
RBC_DEV void solve_any(uint32_t (&v)[1 << LOGW], int k) {
    // bit M of moved: the recursion moved to the upper half at level M.  The coset label is the sum
    // of the halves 2^(M-1) it moved by, and T = k - lam rows of the active block are known.
    uint32_t lam = 0, moved = 0;
    int T = k;
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
            const uint32_t lam_m = (moved & ~((2u << M) - 1u)) >> 1;  // the levels above M that moved
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

// The final transform: evaluations at 0..W-1 of the polynomial with novel
// coefficients v[0 .. W), of which v[nz' .. ) are zero; the node at OFF covers
// the outputs [OFF, OFF + 2^M) and holds nz nonzero coefficients at its front.
// Nodes of >= 2^G rows outside [k, n) are skipped; a finished 2^G-row group is
// handed to st(IC<OFF>).
template <int M, int OFF, int R, class ST>
RBC_DEV void fft_out(uint32_t (&v)[R], int nz, int k, int n, ST &st) {
    if constexpr (M >= G) {
        if (OFF >= n || OFF + (1 << M) <= k) return;
    }
    if constexpr (M <= G) {
        lch::fft_full<M, OFF, OFF, (1 << M)>(v);
        st(IC<OFF>{});
    } else {
        constexpr int H = 1 << (M - 1);
        constexpr uint32_t w = lch::twiddle(M - 1, OFF);
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
        fft_out<M - 1, OFF>(v, nzc, k, n, st);
        // keep the scheduler from interleaving the two independent halves
        if constexpr (M >= SBR) __builtin_amdgcn_sched_barrier(0);
        fft_out<M - 1, OFF + H>(v, nzc, k, n, st);
    }
}

RBC_DEV uint32_t keep_bytes4(int nv) { return nv >= 4 ? 0xffffffffu : (nv <= 0 ? 0u : ((1u << (8 * nv)) - 1u)); }

template <int LOGW, int MODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(LOGW >= 7 ? 1 : 2))) void rs_fft_any_kernel(
    FftArgs a) {
    set_wave_prio(a.prio);
    constexpr int W = 1 << LOGW, GS = 1 << G;
    const int k = a.k, n = a.n;  // 1 <= k <= n <= W < 2n (rbc_launch_rs_fft_any)
    // XCD-aware tile order, as rs_fft_kernel
    uint32_t tile_x = blockIdx.x, tile_y = blockIdx.y;
    {
        const uint32_t gx = gridDim.x, total = gx * gridDim.y, t8 = total & ~7u;
        uint32_t lin = blockIdx.y * gx + blockIdx.x;
        if (lin < t8) lin = (lin & 7u) * (t8 >> 3) + (lin >> 3);
        tile_y = lin / gx;
        tile_x = lin - tile_y * gx;
    }
    const int col = (int)tile_x * 64 + threadIdx.x;  // dword column inside the row
    const int inst = (int)tile_y;
    if (inst >= a.count) return;
    if (a.status && a.status[inst] != 0) return;
    const uint32_t off = 4u * (uint32_t)col;
    if (off >= a.row_pitch) return;
    constexpr bool ENC = MODE == GF_MODE_ENCODE || MODE == GF_MODE_ENCODE_PARITY;
    uint32_t S, B = 0;
    if constexpr (ENC) {
        B = a.lens ? a.lens[inst] : a.uniform_len;
        S = (B + (uint32_t)k - 1) / (uint32_t)k;
    } else {
        S = a.lens ? a.lens[inst] : a.uniform_len;
    }
    const uint32_t keep = keep_bytes4((int)S - (int)off);  // bytes past S are zero
    uint8_t *shards = a.shards + (size_t)inst * a.inst_pitch;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(shards, (short)0, (int)a.inst_pitch, 0x00020000);
    const int pitch = (int)a.row_pitch;
    auto row_store = [&](int pos, uint32_t x) { __builtin_amdgcn_raw_buffer_store_b32(x, rs, (int)off, pos * pitch, 0); };
    auto row_load = [&](int pos) -> uint32_t { return __builtin_amdgcn_raw_buffer_load_b32(rs, (int)off, pos * pitch, 0); };

    uint32_t v[W];
    if constexpr (ENC) {
        const uint8_t *val = a.values + (size_t)inst * a.value_pitch;
        const auto rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(val), (short)0, (int)a.value_pitch,
                                                           0x00020000);
        // Split: data row j is value[j*S, (j+1)*S), the zero pad by masking
        sfor<0, W>([&](auto J) {
            constexpr int j = decltype(J)::value;
            v[j] = 0u;
            if (j < k) v[j] = __builtin_amdgcn_raw_buffer_load_b32(rv, (int)off, (int)((uint32_t)j * S), 0);
        });
        sfor<0, W>([&](auto J) {
            constexpr int j = decltype(J)::value;
            if (j < k) {
                const uint32_t row0 = (uint32_t)j * S;
                if (row0 + S <= B) {  // a full data row
                    v[j] &= keep;
                } else {              // the rows carrying the zero pad
                    const int lim = (int)(B > row0 ? B - row0 : 0u);
                    v[j] &= keep_bytes4(lim - (int)off);
                }
                asm volatile("" : "+v"(v[j]));  // materialise the masked row (rs_fft.hip)
                row_store(j, v[j]);
            }
        });
    } else {
        sfor<0, W>([&](auto J) {
            constexpr int j = decltype(J)::value;
            v[j] = 0u;
            if (j < k) v[j] = row_load(j);
        });
    }

    solve_any<LOGW>(v, k);
    // opaque phase boundary, as rs_fft_kernel
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-lambda-capture"
    sfor<0, W>([&v](auto J) { asm volatile("" : "+v"(v[decltype(J)::value])); });
#pragma clang diagnostic pop

    if constexpr (MODE == GF_MODE_ENCODE) {
        auto st = [&](auto Off) {
            sfor<0, GS>([&](auto I) {
                constexpr int pos = decltype(Off)::value + decltype(I)::value;
                // no `& keep`: every input byte past S was masked to zero on load
                if (pos >= k && pos < n) row_store(pos, v[pos]);
            });
        };
        fft_out<LOGW, 0>(v, k, k, n, st);
    } else if constexpr (MODE == GF_MODE_ENCODE_PARITY) {
        // parity position pos goes to row pos - k of the instance's block of
        // the dense arena, through a descriptor bounded to that block
        const auto rp = __builtin_amdgcn_make_buffer_rsrc(a.parity + (size_t)inst * a.parity_inst_pitch, (short)0,
                                                           (n - k) * pitch, 0x00020000);
        auto st = [&](auto Off) {
            sfor<0, GS>([&](auto I) {
                constexpr int pos = decltype(Off)::value + decltype(I)::value;
                if (pos >= k && pos < n)
                    __builtin_amdgcn_raw_buffer_store_b32(v[pos], rp, (int)off, (pos - k) * pitch, 0);
            });
        };
        fft_out<LOGW, 0>(v, k, k, n, st);
    } else {
        const uint32_t *cls = reinterpret_cast<const uint32_t *>(a.cls + (size_t)inst * a.cls_stride);
        auto st = [&](auto Off) {
            constexpr int o = decltype(Off)::value;
            uint32_t c[GS], old[GS];
            // the group's class bytes (wave-uniform) and its compare loads first
            sfor<0, GS>([&](auto I) {
                constexpr int i = decltype(I)::value, pos = o + i;
                c[i] = 0u;
                old[i] = 0u;
                if (pos >= k && pos < n) c[i] = a.cls ? (cls[pos >> 2] >> (8 * (pos & 3))) & 0xffu : 1u;
                if (c[i] == 2u) old[i] = row_load(pos);
            });
            sfor<0, GS>([&](auto I) {
                constexpr int i = decltype(I)::value, pos = o + i;
                const uint32_t x = v[pos] & keep;
                if (c[i] == 1u) {
                    row_store(pos, x);
                } else if (c[i] == 2u && old[i] != x) {
                    row_store(pos, x);
                    if (a.flags && atomicOr(&a.flags[(size_t)inst * n + pos], 1u) == 0u)
                        a.list[atomicAdd(a.counter, 1u)] = ((uint32_t)inst << 8) | (uint32_t)pos;
                }
            });
        };
        fft_out<LOGW, 0>(v, k, k, n, st);
    }
}

template <int LOGW>
hipError_t launch_any(const FftArgs &a, hipStream_t st) {
    dim3 grid((a.row_pitch / 4 + 63) / 64, (unsigned)a.count);
    if (a.mode == GF_MODE_ENCODE)
        hipLaunchKernelGGL((rs_fft_any_kernel<LOGW, GF_MODE_ENCODE>), grid, dim3(64), 0, st, a);
    else if (a.mode == GF_MODE_ENCODE_PARITY)
        hipLaunchKernelGGL((rs_fft_any_kernel<LOGW, GF_MODE_ENCODE_PARITY>), grid, dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL((rs_fft_any_kernel<LOGW, GF_MODE_DECODE>), grid, dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t rbc_launch_rs_fft_any(const FftArgs &a, hipStream_t st) {
    if (a.count <= 0) return hipSuccess;
    if (a.row_pitch % 4 || a.join) return hipErrorInvalidValue;
    if (a.mode == GF_MODE_ENCODE_PARITY && !a.parity) return hipErrorInvalidValue;
    if (!rbc_fft_any_supported(a.n, a.k)) return hipErrorInvalidValue;
    if (a.n <= 64) return launch_any<6>(a, st);
    return launch_any<7>(a, st);
}
