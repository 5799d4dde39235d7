// rs_fft_wide.hip -- the run-time-geometry additive-FFT codec of rs_fft_any.hip
// for 129 <= n <= 256, 1 <= k <= n: the 256-point transform as two 128-row
// halves, so that a lane never holds more than 128 rows (plus the 64-row g of
// the solve's top level) and the kernel needs no scratch.  Same linear map as
// the matrix codec and as rs_fft_kernel<8, K, N>, byte for byte; same launch
// contract as rs_fft_any_kernel (FftArgs, one lane per dword column of one
// instance, one-wave blocks in the XCD-aware order, wave-uniform branches, no
// fused join).  Model and butterfly counts: tests/fft_wide_model.py.
//
// Write P = P0 + s7 P1 with P0, P1 of fewer than 128 novel coefficients; s7,
// normalised as the transforms normalise it, is 0 on the positions 0..127 and 1
// on 128..255, and the top butterfly constant W_7(0) is 0.  So P = P0 on the
// lower half and P0 + P1 on the upper half: the top layer costs nothing, and
// each half is a 128-point transform on its own coset.  The 128 coefficients
// that are not being worked on wait in the LDS, 128 rows x 64 lanes x 4 bytes =
// 32 KB for the block's one wave; every lane reads back only what it wrote, so
// there is no barrier, and consecutive lanes hit consecutive banks.
//
//   k <= 128 (P1 = 0): solve_any<7> gives P0 from the k data rows; it is parked,
//     the final transform on coset 0 produces the rows [k, 128), P0 comes back
//     and the final transform on coset 128 produces the rows [128, n).
//   k > 128: the inverse transform of the rows 0..127 gives P0, which is parked;
//     its evaluations E on coset 128 (the first tp = k - 128 of them) turn the
//     data rows 128..k-1 into evaluations of P1, the solve recursion started at
//     coset 128 with T = tp gives P1, P0 is added back from the LDS and the
//     final transform on coset 128 produces the rows [k, n).
//
// Transforms on coset 128 hold their rows in the registers 0..127: the row at
// position p is v[p - 128] (fft_out's OFF and LAM).
#include "device_common.h"
#include "host_shared.h"
#include "kernels.h"
#include "rs_fft_rt.h"

using namespace rbcdev;

namespace {

constexpr int HW = 128;  // rows of one half

template <int MODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void rs_fft_wide_kernel(FftArgs a) {
    __shared__ uint32_t park[HW][64];
    set_wave_prio(a.prio);
    constexpr int GS = 1 << G;
    const int k = a.k, n = a.n;  // 1 <= k <= n, 128 < n <= 256 (rbc_launch_rs_fft_wide)
    uint32_t tile_x, tile_y;
    xcd_tile(tile_x, tile_y);
    const int lane = threadIdx.x;
    const int col = (int)tile_x * 64 + lane;  // dword column inside the row
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
    const uint8_t *val = ENC ? a.values + (size_t)inst * a.value_pitch : nullptr;
    const auto rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(val), (short)0,
                                                       ENC ? (int)a.value_pitch : 0, 0x00020000);

    // t[i] = data row P0 + i for P0 + i < k, else zero.  Encode: data row j is value[j*S, (j+1)*S),
    // the zero pad by masking, and the masked row is stored as it is loaded (rs_fft_any_kernel).
    auto load_rows = [&](auto Pos0, auto &t) {
        constexpr int p0 = decltype(Pos0)::value;
        constexpr int cnt = sizeof(t) / sizeof(t[0]);
        sfor<0, cnt>([&](auto I) {
            constexpr int i = decltype(I)::value, j = p0 + i;
            t[i] = 0u;
            if constexpr (ENC) {
                if (j < k) t[i] = __builtin_amdgcn_raw_buffer_load_b32(rv, (int)off, (int)((uint32_t)j * S), 0);
            } else {
                if (j < k) t[i] = row_load(j);
            }
        });
        if constexpr (ENC) {
            sfor<0, cnt>([&](auto I) {
                constexpr int i = decltype(I)::value, j = p0 + i;
                if (j < k) {
                    const uint32_t row0 = (uint32_t)j * S;
                    if (row0 + S <= B) {  // a full data row
                        t[i] &= keep;
                    } else {              // the rows carrying the zero pad
                        const int lim = (int)(B > row0 ? B - row0 : 0u);
                        t[i] &= keep_bytes4(lim - (int)off);
                    }
                    asm volatile("" : "+v"(t[i]));  // materialise the masked row (rs_fft.hip)
                    row_store(j, t[i]);
                }
            });
        }
    };

    // the final transform on coset PB: v[0 .. nz) are the nonzero coefficients, the rows
    // [max(k, PB), min(n, PB + 128)) go out of the registers v[pos - PB]
    const uint32_t *cls =
        MODE == GF_MODE_DECODE ? reinterpret_cast<const uint32_t *>(a.cls + (size_t)inst * a.cls_stride) : nullptr;
    const auto rp = __builtin_amdgcn_make_buffer_rsrc(
        MODE == GF_MODE_ENCODE_PARITY ? a.parity + (size_t)inst * a.parity_inst_pitch : nullptr, (short)0,
        MODE == GF_MODE_ENCODE_PARITY ? (n - k) * pitch : 0, 0x00020000);
    auto emit = [&](auto PB, uint32_t(&v)[HW], int nz) {
        constexpr int pb = decltype(PB)::value;
        if constexpr (MODE == GF_MODE_ENCODE) {
            auto st = [&](auto Off) {
                sfor<0, GS>([&](auto I) {
                    constexpr int r = decltype(Off)::value + decltype(I)::value, pos = pb + r;
                    // no `& keep`: every input byte past S was masked to zero on load
                    if (pos >= k && pos < n) row_store(pos, v[r]);
                });
            };
            fft_out<7, 0, pb>(v, nz, k, n, st);
        } else if constexpr (MODE == GF_MODE_ENCODE_PARITY) {
            // parity position pos goes to row pos - k of the instance's block of
            // the dense arena, through a descriptor bounded to that block
            auto st = [&](auto Off) {
                sfor<0, GS>([&](auto I) {
                    constexpr int r = decltype(Off)::value + decltype(I)::value, pos = pb + r;
                    if (pos >= k && pos < n)
                        __builtin_amdgcn_raw_buffer_store_b32(v[r], rp, (int)off, (pos - k) * pitch, 0);
                });
            };
            fft_out<7, 0, pb>(v, nz, k, n, st);
        } else {
            auto st = [&](auto Off) {
                constexpr int o = decltype(Off)::value;
                uint32_t c[GS], old[GS];
                // the group's class bytes (wave-uniform) and its compare loads first
                sfor<0, GS>([&](auto I) {
                    constexpr int i = decltype(I)::value, pos = pb + o + i;
                    c[i] = 0u;
                    old[i] = 0u;
                    if (pos >= k && pos < n) c[i] = a.cls ? (cls[pos >> 2] >> (8 * (pos & 3))) & 0xffu : 1u;
                    if (c[i] == 2u) old[i] = row_load(pos);
                });
                sfor<0, GS>([&](auto I) {
                    constexpr int i = decltype(I)::value, pos = pb + o + i;
                    const uint32_t x = v[o + i] & keep;
                    if (c[i] == 1u) {
                        row_store(pos, x);
                    } else if (c[i] == 2u && old[i] != x) {
                        row_store(pos, x);
                        if (a.flags && atomicOr(&a.flags[(size_t)inst * n + pos], 1u) == 0u)
                            a.list[atomicAdd(a.counter, 1u)] = ((uint32_t)inst << 8) | (uint32_t)pos;
                    }
                });
            };
            fft_out<7, 0, pb>(v, nz, k, n, st);
        }
    };
    // opaque phase boundary, as rs_fft_kernel
    auto boundary = [](uint32_t(&v)[HW]) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-lambda-capture"
        sfor<0, HW>([&v](auto J) { asm volatile("" : "+v"(v[decltype(J)::value])); });
#pragma clang diagnostic pop
    };

    // The lane's column of `park` for reading back, opaque to the compiler: it would otherwise
    // forward the parked values to their reloads and keep all 128 of them in registers meanwhile.
    auto unparked = [&]() {
        int l = lane;
        asm volatile("" : "+v"(l));
        return l;
    };

    uint32_t v[HW];
    int nz;  // nonzero coefficients of the polynomial on the upper half
    // Each case loads its own rows 0..127: loaded once ahead of the branch, some sixty of them stayed
    // live across the whole k > 128 case, and the kernel took 256 + 256 registers and 70 - 110 bytes
    // of scratch a lane.
    if (k <= HW) {
        load_rows(IC<0>{}, v);
        solve_any<7>(v, k);
        boundary(v);
        sfor<0, HW>([&](auto I) { park[decltype(I)::value][lane] = v[decltype(I)::value]; });
        emit(IC<0>{}, v, k);
        __builtin_amdgcn_sched_barrier(0);
        const int back = unparked();
        sfor<0, HW>([&](auto I) { v[decltype(I)::value] = park[decltype(I)::value][back]; });
        nz = k;
    } else {
        const int tp = k - HW;
        load_rows(IC<0>{}, v);
        ifft_rt<7, 0>(v, 0u);  // P0
        __builtin_amdgcn_sched_barrier(0);
        sfor<0, HW>([&](auto I) { park[decltype(I)::value][lane] = v[decltype(I)::value]; });
        fft_rt<7, 0>(v, (uint32_t)HW, tp);  // E = P0 on coset 128, the first tp rows
        __builtin_amdgcn_sched_barrier(0);
        // v[i] = row(128 + i) + E[i] = P1(128 + i) for i < tp, zeros after them
        sfor<0, HW / 32>([&](auto C) {
            constexpr int c0 = 32 * decltype(C)::value;
            uint32_t t[32];
            load_rows(IC<HW + c0>{}, t);
            sfor<0, 32>([&](auto I) {
                constexpr int i = decltype(I)::value;
                v[c0 + i] = c0 + i < tp ? v[c0 + i] ^ t[i] : 0u;
            });
            __builtin_amdgcn_sched_barrier(0);
        });
        solve_any<7>(v, k, (uint32_t)HW);  // P1
        __builtin_amdgcn_sched_barrier(0);
        const int back = unparked();
        rows_for<HW>([&](auto I) { v[decltype(I)::value] ^= park[decltype(I)::value][back]; });
        nz = HW;
    }
    boundary(v);
    emit(IC<HW>{}, v, nz);
}

hipError_t launch_wide(const FftArgs &a, hipStream_t st) {
    dim3 grid((a.row_pitch / 4 + 63) / 64, (unsigned)a.count);
    if (a.mode == GF_MODE_ENCODE)
        hipLaunchKernelGGL((rs_fft_wide_kernel<GF_MODE_ENCODE>), grid, dim3(64), 0, st, a);
    else if (a.mode == GF_MODE_ENCODE_PARITY)
        hipLaunchKernelGGL((rs_fft_wide_kernel<GF_MODE_ENCODE_PARITY>), grid, dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL((rs_fft_wide_kernel<GF_MODE_DECODE>), grid, dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t rbc_launch_rs_fft_wide(const FftArgs &a, hipStream_t st) {
    if (a.count <= 0) return hipSuccess;
    if (a.row_pitch % 4 || a.join) return hipErrorInvalidValue;
    if (a.mode == GF_MODE_ENCODE_PARITY && !a.parity) return hipErrorInvalidValue;
    if (!rbc_fft_wide_supported(a.n, a.k)) return hipErrorInvalidValue;
    return launch_wide(a, st);
}
