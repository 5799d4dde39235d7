// rs_fft_small.hip -- the run-time-geometry additive-FFT codec of rs_fft_any.hip for 2 <= n <= 32:
// one kernel per transform width W = 8, 16, 32 (the smallest of them >= n; W < 2n is not needed,
// tests/fft_small_model.py), per mode and per lane width CW, n and k as kernel arguments.  It
// computes the same linear map as the matrix codec and as rs_fft_kernel<2, 2, 4> and <4, 6, 16>,
// byte for byte, and follows rs_fft_any_kernel's launch contract: FftArgs with generic = 1,
// one-wave blocks in the XCD-aware tile order, the status skip, wave-uniform branches, no fused
// join, decode in 8-row compare groups with the same class bytes, flags and re-hash list.
//
// What is new is CW: a lane owns CW adjacent dword columns of every row (rs_fft_cols.h), so a
// wave covers 256 * CW bytes of each row.  With at most 32 rows the per-group costs of the
// run-time form weigh most: one five-dword scalar table fetch per (layer, coset) group, W - 1 of
// them for (W/2) log2 W butterflies, and one memory instruction per row and lane.  At CW = 4 one
// fetch, and the literal tables of the final transform, serve four columns, and a shard row is
// read as one 16-byte buffer access and written as two 8-byte ones (off % 16 == 0 and
// row_pitch % 16 == 0, which the launcher requires of this body, keep them aligned and inside the
// row).  CW = 1 is rs_fft_any_kernel's shape.  rbc_fft_small_lane (host_shared.h) chooses
// between them.  W = 32 has CW = 2 (8-byte accesses, 512 B a wave) in place of CW = 4: four
// columns of 32 rows and of the solve's 16-row copy g fill all 256 registers of two waves per
// SIMD and spill (20 to 164 bytes a lane); two columns take 132.
//
// Why no 16-byte store.  buffer_store_dwordx4 reads its data registers over several cycles, and
// the compiler pads a VALU write of them behind the store only when the store's soffset is not a
// register; here it is one (the row start).  Built that way, the first parity row's store was
// followed at once by the next butterfly writing its second data register, and with several
// waves on a SIMD (rows of 64 KiB and more) lanes 12..15 of every 16 stored that dword's later
// value: 20 to 260 thousand wrong bytes in 48 instances of 1 MiB, none at rows of 8 KiB.  A store
// of at most 8 bytes has no such window.  tests/test_gpu_fft_small.py's long-row test and
// tools/codec_bench.py's output comparison are the checks.
//
// The value read of the encode modes stays one dword load per column, at byte j*S + off + 4c of
// a descriptor bounded to value_pitch, whatever CW is: S is arbitrary, so the address is unaligned.
// A dword that straddles the end of the descriptor is out of range as a whole and reads as zero
// (measured: tests/test_gpu_fft_small.py's guarded arena, a value ending 1 byte short of its
// pitch, lost its last two bytes), so a data row whose dwords can reach past value_pitch
// (j*S + S + 3 > value_pitch, a wave-uniform test; the last rows of a value that ends within
// 3 bytes of its pitch) is read byte by byte, each byte range-checked on its own.  Nothing is
// read outside [0, value_pitch).  The tail mask and the Split-pad mask are per dword.  The
// decode compare is "any of the lane's dwords differs": then the lane stores its CW dwords and
// raises the flag, one atomicOr and at most one list append per (instance, position).
//
// No instantiation uses scratch (DESIGN.md 5.1 has the table).
#include "device_common.h"
#include "host_shared.h"
#include "kernels.h"
#include "rs_fft_cols.h"

using namespace rbcdev;

namespace {

typedef uint32_t u32x4 __attribute__((__vector_size__(16)));
typedef uint32_t u32x2 __attribute__((__vector_size__(8)));

// the lane's CW dwords of one row, at byte off + soff of the descriptor
template <int CW>
RBC_DEV void cols_load(uint32_t (&x)[CW], __amdgpu_buffer_rsrc_t rs, int off, int soff) {
    if constexpr (CW == 4) {
        const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(rs, off, soff, 0);
        x[0] = q[0], x[1] = q[1], x[2] = q[2], x[3] = q[3];
    } else if constexpr (CW == 2) {
        const u32x2 q = __builtin_amdgcn_raw_buffer_load_b64(rs, off, soff, 0);
        x[0] = q[0], x[1] = q[1];
    } else {
        sfor<0, CW>([&](auto C) {
            constexpr int c = decltype(C)::value;
            x[c] = __builtin_amdgcn_raw_buffer_load_b32(rs, off + 4 * c, soff, 0);
        });
    }
}
template <int CW>
RBC_DEV void cols_store(const uint32_t (&x)[CW], __amdgpu_buffer_rsrc_t rs, int off, int soff) {
    if constexpr (CW == 4) {  // two 8-byte stores, not one of 16 (the header says why)
        const u32x2 lo = {x[0], x[1]}, hi = {x[2], x[3]};
        __builtin_amdgcn_raw_buffer_store_b64(lo, rs, off, soff, 0);
        asm volatile("" ::: "memory");  // or the two are merged back into one dwordx4
        __builtin_amdgcn_raw_buffer_store_b64(hi, rs, off + 8, soff, 0);
    } else if constexpr (CW == 2) {
        const u32x2 q = {x[0], x[1]};
        __builtin_amdgcn_raw_buffer_store_b64(q, rs, off, soff, 0);
    } else {
        sfor<0, CW>([&](auto C) {
            constexpr int c = decltype(C)::value;
            __builtin_amdgcn_raw_buffer_store_b32(x[c], rs, off + 4 * c, soff, 0);
        });
    }
}

template <int LOGW, int CW, int MODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void rs_fft_small_kernel(FftArgs a) {
    set_wave_prio(a.prio);
    constexpr int W = 1 << LOGW, GS = 1 << G;
    static_assert(LOGW >= G, "fft_out_c hands over groups of 2^G rows");
    const int k = a.k, n = a.n;  // 1 <= k <= n <= W (rbc_launch_rs_fft_small)
    uint32_t tile_x, tile_y;
    xcd_tile(tile_x, tile_y);
    const int col = ((int)tile_x * 64 + (int)threadIdx.x) * CW;  // the lane's first dword column
    const int inst = (int)tile_y;
    if (inst >= a.count) return;
    if (a.status && a.status[inst] != 0) return;
    const uint32_t off = 4u * (uint32_t)col;
    if (off >= a.row_pitch) return;  // row_pitch % (4 * CW) == 0: the lane's CW dwords lie inside the row
    constexpr bool ENC = MODE == GF_MODE_ENCODE || MODE == GF_MODE_ENCODE_PARITY;
    uint32_t S, B = 0;
    if constexpr (ENC) {
        B = a.lens ? a.lens[inst] : a.uniform_len;
        S = (B + (uint32_t)k - 1) / (uint32_t)k;
    } else {
        S = a.lens ? a.lens[inst] : a.uniform_len;
    }
    uint32_t keep[CW];  // bytes past S are zero
    sfor<0, CW>([&](auto C) { keep[decltype(C)::value] = keep_bytes4((int)S - (int)off - 4 * decltype(C)::value); });
    uint8_t *shards = a.shards + (size_t)inst * a.inst_pitch;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(shards, (short)0, (int)a.inst_pitch, 0x00020000);
    const int pitch = (int)a.row_pitch;

    uint32_t v[W][CW];
    if constexpr (ENC) {
        const uint8_t *val = a.values + (size_t)inst * a.value_pitch;
        const auto rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(val), (short)0, (int)a.value_pitch,
                                                           0x00020000);
        // Split: data row j is value[j*S, (j+1)*S), the zero pad by masking
        sfor<0, W>([&](auto J) {
            constexpr int j = decltype(J)::value;
            sfor<0, CW>([&](auto C) { v[j][decltype(C)::value] = 0u; });
            if (j < k) {
                const uint32_t row0 = (uint32_t)j * S;
                if (row0 + S + 3u <= a.value_pitch) {
                    sfor<0, CW>([&](auto C) {
                        constexpr int c = decltype(C)::value;
                        v[j][c] = __builtin_amdgcn_raw_buffer_load_b32(rv, (int)off + 4 * c, (int)row0, 0);
                    });
                } else {  // a dword of this row may straddle the end of the value buffer
                    sfor<0, 4 * CW>([&](auto Bt) {
                        constexpr int bt = decltype(Bt)::value;
                        const uint32_t x = __builtin_amdgcn_raw_buffer_load_b8(rv, (int)off + bt, (int)row0, 0);
                        v[j][bt / 4] |= x << (8 * (bt % 4));
                    });
                }
            }
        });
        sfor<0, W>([&](auto J) {
            constexpr int j = decltype(J)::value;
            if (j < k) {
                const uint32_t row0 = (uint32_t)j * S;
                if (row0 + S <= B) {  // a full data row
                    sfor<0, CW>([&](auto C) { v[j][decltype(C)::value] &= keep[decltype(C)::value]; });
                } else {              // the rows carrying the zero pad
                    const int lim = (int)(B > row0 ? B - row0 : 0u);
                    sfor<0, CW>([&](auto C) {
                        constexpr int c = decltype(C)::value;
                        v[j][c] &= keep_bytes4(lim - (int)off - 4 * c);
                    });
                }
                // materialise the masked row (rs_fft.hip)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-lambda-capture"
                sfor<0, CW>([&v](auto C) { asm volatile("" : "+v"(v[j][decltype(C)::value])); });
#pragma clang diagnostic pop
                cols_store(v[j], rs, (int)off, j * pitch);
            }
        });
    } else {
        sfor<0, W>([&](auto J) {
            constexpr int j = decltype(J)::value;
            sfor<0, CW>([&](auto C) { v[j][decltype(C)::value] = 0u; });
            if (j < k) cols_load(v[j], rs, (int)off, j * pitch);
        });
    }

    solve_c<LOGW>(v, k);
    // opaque phase boundary, as rs_fft_kernel
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-lambda-capture"
    sfor<0, W>([&v](auto J) {
        sfor<0, CW>([&v](auto C) { asm volatile("" : "+v"(v[decltype(J)::value][decltype(C)::value])); });
    });
#pragma clang diagnostic pop

    if constexpr (MODE == GF_MODE_ENCODE) {
        auto st = [&](auto Off) {
            sfor<0, GS>([&](auto I) {
                constexpr int pos = decltype(Off)::value + decltype(I)::value;
                // no `& keep`: every input byte past S was masked to zero on load
                if (pos >= k && pos < n) cols_store(v[pos], rs, (int)off, pos * pitch);
            });
        };
        fft_out_c<LOGW, 0>(v, k, k, n, st);
    } else if constexpr (MODE == GF_MODE_ENCODE_PARITY) {
        // parity position pos goes to row pos - k of the instance's block of
        // the dense arena, through a descriptor bounded to that block
        const auto rp = __builtin_amdgcn_make_buffer_rsrc(a.parity + (size_t)inst * a.parity_inst_pitch, (short)0,
                                                           (n - k) * pitch, 0x00020000);
        auto st = [&](auto Off) {
            sfor<0, GS>([&](auto I) {
                constexpr int pos = decltype(Off)::value + decltype(I)::value;
                if (pos >= k && pos < n) cols_store(v[pos], rp, (int)off, (pos - k) * pitch);
            });
        };
        fft_out_c<LOGW, 0>(v, k, k, n, st);
    } else {
        const uint32_t *cls = reinterpret_cast<const uint32_t *>(a.cls + (size_t)inst * a.cls_stride);
        auto st = [&](auto Off) {
            constexpr int o = decltype(Off)::value;
            uint32_t c[GS], old[GS][CW];
            // the group's class bytes (wave-uniform) and its compare loads first
            sfor<0, GS>([&](auto I) {
                constexpr int i = decltype(I)::value, pos = o + i;
                c[i] = 0u;
                sfor<0, CW>([&](auto C) { old[i][decltype(C)::value] = 0u; });
                if (pos >= k && pos < n) c[i] = a.cls ? (cls[pos >> 2] >> (8 * (pos & 3))) & 0xffu : 1u;
                if (c[i] == 2u) cols_load(old[i], rs, (int)off, pos * pitch);
            });
            sfor<0, GS>([&](auto I) {
                constexpr int i = decltype(I)::value, pos = o + i;
                uint32_t x[CW], diff = 0u;
                sfor<0, CW>([&](auto C) {
                    constexpr int cc = decltype(C)::value;
                    x[cc] = v[pos][cc] & keep[cc];
                    diff |= old[i][cc] ^ x[cc];
                });
                if (c[i] == 1u) {
                    cols_store(x, rs, (int)off, pos * pitch);
                } else if (c[i] == 2u && diff != 0u) {  // any of the lane's dwords differs
                    cols_store(x, rs, (int)off, pos * pitch);
                    if (a.flags && atomicOr(&a.flags[(size_t)inst * n + pos], 1u) == 0u)
                        a.list[atomicAdd(a.counter, 1u)] = ((uint32_t)inst << 8) | (uint32_t)pos;
                }
            });
        };
        fft_out_c<LOGW, 0>(v, k, k, n, st);
    }
}

template <int LOGW, int CW>
hipError_t launch_small(const FftArgs &a, hipStream_t st) {
    dim3 grid((a.row_pitch / 4 + 64 * CW - 1) / (64 * CW), (unsigned)a.count);
    if (a.mode == GF_MODE_ENCODE)
        hipLaunchKernelGGL((rs_fft_small_kernel<LOGW, CW, GF_MODE_ENCODE>), grid, dim3(64), 0, st, a);
    else if (a.mode == GF_MODE_ENCODE_PARITY)
        hipLaunchKernelGGL((rs_fft_small_kernel<LOGW, CW, GF_MODE_ENCODE_PARITY>), grid, dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL((rs_fft_small_kernel<LOGW, CW, GF_MODE_DECODE>), grid, dim3(64), 0, st, a);
    return hipGetLastError();
}

template <int LOGW>
hipError_t launch_small_w(const FftArgs &a, hipStream_t st) {
    constexpr int WL = rbc_fft_small_wide_lane(1 << LOGW);
    int lane = a.lane ? a.lane : rbc_fft_small_lane(1 << LOGW, a.row_pitch);
    // the wide body's 8- or 16-byte row accesses need whole chunks in every row
    if (a.row_pitch % (4u * WL)) lane = 1;
    return lane == WL ? launch_small<LOGW, WL>(a, st) : launch_small<LOGW, 1>(a, st);
}

}  // namespace

hipError_t rbc_launch_rs_fft_small(const FftArgs &a, hipStream_t st) {
    if (a.count <= 0) return hipSuccess;
    if (a.row_pitch % 4 || a.join) return hipErrorInvalidValue;
    if (a.mode == GF_MODE_ENCODE_PARITY && !a.parity) return hipErrorInvalidValue;
    if (!rbc_fft_small_supported(a.n, a.k)) return hipErrorInvalidValue;
    if (!rbc_fft_small_lane_valid(a.n, a.lane)) return hipErrorInvalidValue;
    const int logw = rbc_fft_small_logw(a.n);
    if (logw == 3) return launch_small_w<3>(a, st);
    if (logw == 4) return launch_small_w<4>(a, st);
    return launch_small_w<5>(a, st);
}
