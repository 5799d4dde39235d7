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
// Built for W = 64 and W = 128 (33 <= n <= 128).  W = 256 does not fit here:
// with 256 rows and the 128-row copy of g resident it overflows the 512
// registers of a lone wave (100 - 250 bytes of scratch a lane).
// n > 128 is rs_fft_wide.hip's: two 128-row halves built from the same pieces
// (rs_fft_rt.h), with the idle half parked in the LDS.  W = 128 takes 256 VGPRs
// and a few AGPRs, one wave per SIMD; W = 64 132 VGPRs.
#include "device_common.h"
#include "host_shared.h"
#include "kernels.h"
#include "rs_fft_rt.h"

using namespace rbcdev;

namespace {

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
