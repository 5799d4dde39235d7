// rs_fft.hip -- Reed-Solomon systematic encode over GF(2^8)/0x11D by additive
// FFT, for gfx950.  Bit-identical to klauspost/reedsolomon v1.9.1's matrix
// code (held at rbc/rbc.go:20; shard() at rbc/rbc.go:97-100) because it
// computes the same linear map:
//
//   klauspost's M = V * inv(V[:k]), V[r][c] = r^c, so shard r is P(r) for the
//   unique P with deg P < k and P(j) = data_j (j < k), evaluated at the field
//   elements with integer labels 0..N-1.  Those labels form the GF(2)-subspace
//   V_n = span{1, 2, .., 2^(n-1)}, the domain of the Lin-Chung-Han additive FFT
//   in the novel polynomial basis X_i = prod_{j in bits(i)} W_j, where
//   W_j = s_j / s_j(2^j) and s_j is the vanishing polynomial of V_j.  deg P < k
//   iff the novel coefficients vanish from index k on, so
//     coeffs  = solve(n, 0, data, k)   (only power-of-two IFFT/FFT blocks)
//     shards  = FFT(coeffs) at the positions [k, N)
//   Model and op counts: tests/fft_model.py (checked against the oracle by
//   tests/test_fft_model.py).
//
// Every butterfly constant W_j(lambda) is a compile-time constant, so the
// whole transform unrolls into straight-line VALU code: a constant multiply of
// 4 packed bytes is three v_perm_b32 lookups into literal 8-entry tables
// (the CDNA analogue of PSHUFB split-nibble tables), the add is v_bitop3 xor3.
// One lane owns one dword column of every row of one instance; the rows live
// in VGPRs for the whole transform (no LDS).  At N=128, k=44: 462 constant
// multiplies + ~550 xors per column instead of the matrix's 3,696 MACs.
//
// Modes: ENCODE reads data row j straight from the value bytes at j*S (Split,
// zero pad by masking) and writes data + parity rows; DECODE reads the k data
// rows of an already completed data half (interpolate: the missing data rows
// are regenerated first by gf_regen_kernel) and writes the parity positions by
// class: 0 skip (used), 1 store (missing), 2 compare (valid but unused: store,
// flag and queue for re-hash only if the re-encoding differs).  ENCODE_PARITY
// is ENCODE with two outputs: the data rows [I][k][pitch] and a dense parity
// arena [I][N-k][pitch] that leaves the device in one linear copy (a Go node
// already holds Split's data rows, rbc/rbc.go:97-100).
#include "device_common.h"
#include "kernels.h"
#include "rs_fft_lch.h"

using namespace rbcdev;

namespace {

RBC_DEV uint32_t keep_bytes4(int nv) { return nv >= 4 ? 0xffffffffu : (nv <= 0 ? 0u : ((1u << (8 * nv)) - 1u)); }

template <int LOGW, int K, int N, int MODE>
// waves_per_eu(2): at N=256 the decode variant otherwise takes 256 VGPRs + 25
// AGPRs (one wave per SIMD); with the hint it fits 256 with no scratch
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void rs_fft_kernel(FftArgs a) {
    set_wave_prio(a.prio);
    constexpr int W = 1 << LOGW;
    constexpr int G = 3;   // encode: outputs are stored in groups of 2^G rows
    // decode: compare groups of 2^GD rows.  N=128 VGPRs in the prefetch form
    // (below): 1 -> 137, 2 -> 143, 3 -> 157; in the two-stage pipeline the
    // other geometries keep: 1 -> 141, 2 -> 151 (measured: DESIGN.md 7.1)
    constexpr int GD = 2;
    static_assert(K >= 1 && K <= N && N <= W && 2 * N > W, "geometry");
    // XCD-aware tile order: the dispatcher deals workgroups round-robin over
    // the 8 XCDs (linear id % 8), so neighbouring column tiles of one instance
    // would land on different L2s.  Encode reads data row j at j*S, which is
    // not line aligned: a 256-B tile touches 3 lines, 2 of them shared with
    // its neighbours.  Remapping linear id L -> (L % 8) * (T8 / 8) + L / 8
    // gives each XCD a contiguous run of tiles, so the shared lines hit in
    // that XCD's L2 instead of being fetched twice from HBM.  Decode too: its
    // fused join stores row j at j*S, so neighbouring tiles (and row j's end
    // and row j+1's start) share value lines, merged in one L2 this way
    // (C1 / C2 / C3 +1-3 %, profiles/r06r/).
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
    // ENCODE_PARITY is ENCODE with the parity rows stored through a second
    // descriptor (below); ENCODE and DECODE compile as before
    constexpr bool ENC = MODE == GF_MODE_ENCODE || MODE == GF_MODE_ENCODE_PARITY;
    uint32_t S, B = 0;
    if constexpr (ENC) {
        B = a.lens ? a.lens[inst] : a.uniform_len;
        S = (B + K - 1) / K;
    } else {
        S = a.lens ? a.lens[inst] : a.uniform_len;
    }
    const uint32_t keep = keep_bytes4((int)S - (int)off);  // bytes past S are zero
    // every row access is base(SGPR) + off(one VGPR) + row*pitch(SGPR): one
    // VGPR of addressing for all N rows instead of a 64-bit pointer per row
    uint8_t *shards = a.shards + (size_t)inst * a.inst_pitch;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(shards, (short)0, (int)a.inst_pitch, 0x00020000);
    const int pitch = (int)a.row_pitch;
    auto row_store = [&](int pos, uint32_t x) { __builtin_amdgcn_raw_buffer_store_b32(x, rs, (int)off, pos * pitch, 0); };
    auto row_load = [&](int pos) -> uint32_t { return __builtin_amdgcn_raw_buffer_load_b32(rs, (int)off, pos * pitch, 0); };

    // N=128 decode, prefetch form of the compare (below): the class bytes of
    // the parity positions, wave-uniform, held in SGPRs from the start
    constexpr bool PF = MODE == GF_MODE_DECODE && N == 128;
    constexpr int CW0 = K / 4, CWN = (N + 3) / 4;
    uint32_t cw[PF ? CWN - CW0 : 1];
    (void)cw;

    uint32_t v[W];
    if constexpr (ENC) {
        const uint8_t *val = a.values + (size_t)inst * a.value_pitch;
        const auto rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(val), (short)0, (int)a.value_pitch,
                                                           0x00020000);
        // all K loads issued back to back, unconditionally (out-of-range
        // reads return 0 through the buffer descriptor); the Split zero pad
        // is applied by masking afterwards.  Unaligned dword reads are fine
        // on gfx950.
        lch::sfor<0, K>([&](auto J) {
            constexpr int j = decltype(J)::value;
            v[j] = __builtin_amdgcn_raw_buffer_load_b32(rv, (int)off, (int)((uint32_t)j * S), 0);
        });
        lch::sfor<0, K>([&](auto J) {
            constexpr int j = decltype(J)::value;
            const uint32_t row0 = (uint32_t)j * S;  // Split: data[j*S : (j+1)*S]
            if (row0 + S <= B) {                    // wave-uniform: a full data row
                v[j] &= keep;
            } else {                                // the rows carrying the zero pad
                const int lim = (int)(B > row0 ? B - row0 : 0u);
                v[j] &= keep_bytes4(lim - (int)off);
            }
            // materialise the masked row: otherwise the AND is folded into
            // the first butterfly (v_bitop3) and the raw row plus its mask
            // stay live through the transform (+44 VGPRs)
            asm volatile("" : "+v"(v[j]));
            row_store(j, v[j]);
        });
    } else {
        if constexpr (PF) {
            // issued with the row loads: one wait for all of them, and no
            // class lookup (a dependent load and a drain of every store in
            // flight) at each compare group later
            const uint32_t *cls = reinterpret_cast<const uint32_t *>(a.cls + (size_t)inst * a.cls_stride);
            lch::sfor<CW0, CWN>([&](auto J) {
                constexpr int j = decltype(J)::value;
                cw[j - CW0] = (uint32_t)__builtin_amdgcn_readfirstlane((int)cls[j]);
            });
        }
        lch::sfor<0, K>([&](auto J) { v[decltype(J)::value] = row_load(decltype(J)::value); });
        if (a.join) {
            // interpolate's value (rbc/rbc.go:88) straight from the loaded rows:
            // data row j at j*S, dword stores at byte offsets that need not be
            // aligned, the lane that straddles S writes its bytes one by one;
            // tile 0 zeroes the value's tail up to join_pitch.  The buffer
            // descriptor bounds every store to the instance's value row.
            const auto rj = __builtin_amdgcn_make_buffer_rsrc(a.join + (size_t)inst * a.join_pitch, (short)0,
                                                              (int)a.join_pitch, 0x00020000);
            const int nb = (int)S - (int)off;  // this lane's valid bytes per row
            lch::sfor<0, K>([&](auto J) {
                constexpr int j = decltype(J)::value;
                const int so = (int)((uint32_t)j * S);
                if (nb >= 4) {
                    __builtin_amdgcn_raw_buffer_store_b32(v[j], rj, (int)off, so, 0);
                } else if (nb > 0) {
                    for (int b = 0; b < nb; ++b)
                        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(v[j] >> (8 * b)), rj, (int)off + b, so, 0);
                }
            });
            if (tile_x == 0) {
                const uint32_t end = (uint32_t)K * S;
                for (int b = 0; b < 4; ++b) {
                    const uint32_t o = end + 4u * threadIdx.x + (uint32_t)b;
                    if (o < a.join_pitch) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)0, rj, (int)o, 0, 0);
                }
            }
        }
    }

    lch::solve<LOGW, 0, 0, K>(v);
    // opaque phase boundary: without it LLVM fuses xor chains of the final
    // transform with solve's and keeps raw input rows live to the end
    // (N=128 encode: 191 -> 127 VGPRs, 2 -> 4 waves per SIMD)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-lambda-capture"  // the capture is needed (asm operand)
    lch::sfor<0, K>([&v](auto J) { asm volatile("" : "+v"(v[decltype(J)::value])); });
#pragma clang diagnostic pop

    if constexpr (MODE == GF_MODE_ENCODE) {
        auto st = [&](auto Lam, auto Off, auto Lo, auto Hi) {
            lch::sfor<decltype(Lo)::value, decltype(Hi)::value>([&](auto I) {
                constexpr int i = decltype(I)::value, pos = decltype(Lam)::value + i;
                // no `& keep`: every input byte past S was masked to zero on
                // load, and the transform is column-wise linear
                if constexpr (pos >= K && pos < N) row_store(pos, v[decltype(Off)::value + i]);
            });
        };
        lch::fft<G, LOGW, 0, 0, K, K, N>(v, st);
    } else if constexpr (MODE == GF_MODE_ENCODE_PARITY) {
        // the data rows went to `shards` [I][K][pitch] above; parity position
        // pos goes to row pos - K of the instance's block of the dense arena
        // [I][N-K][pitch], through a descriptor of its own bounded to that
        // block (SGPRs only: same lane offset, same row-offset arithmetic)
        const auto rp = __builtin_amdgcn_make_buffer_rsrc(a.parity + (size_t)inst * a.parity_inst_pitch, (short)0,
                                                           (N - K) * pitch, 0x00020000);
        auto st = [&](auto Lam, auto Off, auto Lo, auto Hi) {
            lch::sfor<decltype(Lo)::value, decltype(Hi)::value>([&](auto I) {
                constexpr int i = decltype(I)::value, pos = decltype(Lam)::value + i;
                if constexpr (pos >= K && pos < N)
                    __builtin_amdgcn_raw_buffer_store_b32(v[decltype(Off)::value + i], rp, (int)off, (pos - K) * pitch,
                                                          0);
            });
        };
        lch::fft<G, LOGW, 0, 0, K, K, N>(v, st);
    } else if constexpr (PF) {
        // Prefetch form.  The compare loads of the NEXT output group are
        // issued before this group is compared and stored, and fly through
        // the next group's butterflies; the only state carried between
        // groups is that group's old rows (pold).  Every load is issued
        // unconditionally -- a position that is not compared reads through a
        // descriptor of zero records, which returns 0 without touching
        // memory -- so the wait before a compare is a counted one that leaves
        // the loads just issued in flight; behind a branch it would be a
        // full drain.
        constexpr int GS = 1 << GD;
        uint32_t pold[GS] = {};
        auto cls_at = [&](auto Pos) -> uint32_t {
            constexpr int pos = decltype(Pos)::value;
            return (cw[(pos >> 2) - CW0] >> (8 * (pos & 3))) & 0xffu;  // scalar
        };
        auto prefetch = [&](auto Lam, uint32_t (&dst)[GS]) {
            constexpr int lam = decltype(Lam)::value;
            lch::sfor<lch::cmax(K - lam, 0), lch::cmin(GS, N - lam)>([&](auto I) {
                constexpr int i = decltype(I)::value, pos = lam + i;
                const auto rc = __builtin_amdgcn_make_buffer_rsrc(
                    shards, (short)0, cls_at(lch::IC<pos>{}) == 2u ? (int)a.inst_pitch : 0, 0x00020000);
                dst[i] = __builtin_amdgcn_raw_buffer_load_b32(rc, (int)off, pos * pitch, 0);
            });
        };
        auto st = [&](auto Lam, auto Off, auto Lo, auto Hi) {
            constexpr int lam = decltype(Lam)::value, o = decltype(Off)::value;
            constexpr int lo = lch::cmax(decltype(Lo)::value, K - lam), hi = lch::cmin(decltype(Hi)::value, N - lam);
            if constexpr (lo < hi) {
                uint32_t nold[GS] = {};
                if constexpr (lam + GS < N) prefetch(lch::IC<lam + GS>{}, nold);
                lch::sfor<lo, hi>([&](auto I) {
                    constexpr int i = decltype(I)::value, pos = lam + i;
                    const uint32_t c = cls_at(lch::IC<pos>{}), x = v[o + i] & keep;
                    if (c == 1u) {
                        row_store(pos, x);
                    } else if (c == 2u && pold[i] != x) {
                        row_store(pos, x);
                        if (a.flags && atomicOr(&a.flags[(size_t)inst * N + pos], 1u) == 0u)
                            a.list[atomicAdd(a.counter, 1u)] = ((uint32_t)inst << 8) | (uint32_t)pos;
                    }
                });
                lch::sfor<0, GS>([&](auto I) { pold[decltype(I)::value] = nold[decltype(I)::value]; });
            }
        };
        prefetch(lch::IC<(K / GS) * GS>{}, pold);  // the first group's, in flight through the upper layers
        lch::fft<GD, LOGW, 0, 0, K, K, N>(v, st);
    } else {
        const uint32_t *cls = reinterpret_cast<const uint32_t *>(a.cls + (size_t)inst * a.cls_stride);
        // Software pipeline over output groups: the compare loads of group g
        // are in flight while group g-1 is compared and stored, so the HBM
        // latency of a compare read is paid once per kernel, not per group.
        constexpr int GS = 1 << GD;
        uint32_t px[GS], pold[GS], pc[GS];
        int ppos = 0, pcnt = 0;
        auto flush = [&]() {
            lch::sfor<0, GS>([&](auto I) {
                constexpr int i = decltype(I)::value;
                if (i < pcnt) {  // wave-uniform
                    const int pos = ppos + i;
                    if (pc[i] == 1u) {
                        row_store(pos, px[i]);
                    } else if (pc[i] == 2u && pold[i] != px[i]) {
                        row_store(pos, px[i]);
                        if (a.flags && atomicOr(&a.flags[(size_t)inst * N + pos], 1u) == 0u)
                            a.list[atomicAdd(a.counter, 1u)] = ((uint32_t)inst << 8) | (uint32_t)pos;
                    }
                }
            });
        };
        auto st = [&](auto Lam, auto Off, auto Lo, auto Hi) {
            constexpr int lam = decltype(Lam)::value, o = decltype(Off)::value;
            constexpr int lo = lch::cmax(decltype(Lo)::value, K - lam), hi = lch::cmin(decltype(Hi)::value, N - lam);
            if constexpr (lo < hi) {
                uint32_t c[hi - lo], old[hi - lo];
                // class lookups + the compare loads of this group
                lch::sfor<lo, hi>([&](auto I) {
                    constexpr int i = decltype(I)::value, pos = lam + i;
                    c[i - lo] = (cls[pos >> 2] >> (8 * (pos & 3))) & 0xffu;  // wave-uniform
                    old[i - lo] = 0;
                    if (c[i - lo] == 2u) old[i - lo] = row_load(pos);
                });
                flush();  // the previous group, while these loads fly
                lch::sfor<lo, hi>([&](auto I) {
                    constexpr int i = decltype(I)::value;
                    px[i - lo] = v[o + i] & keep;
                    pold[i - lo] = old[i - lo];
                    pc[i - lo] = c[i - lo];
                });
                ppos = lam + lo;
                pcnt = hi - lo;
            }
        };
        lch::fft<GD, LOGW, 0, 0, K, K, N>(v, st);
        flush();
    }
}

template <int LOGW, int K, int N>
hipError_t launch_fft(const FftArgs &a, hipStream_t st) {
    dim3 grid((a.row_pitch / 4 + 63) / 64, (unsigned)a.count);
    if (a.mode == GF_MODE_ENCODE)
        hipLaunchKernelGGL((rs_fft_kernel<LOGW, K, N, GF_MODE_ENCODE>), grid, dim3(64), 0, st, a);
    else if (a.mode == GF_MODE_ENCODE_PARITY)
        hipLaunchKernelGGL((rs_fft_kernel<LOGW, K, N, GF_MODE_ENCODE_PARITY>), grid, dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL((rs_fft_kernel<LOGW, K, N, GF_MODE_DECODE>), grid, dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t rbc_launch_rs_fft(const FftArgs &a, hipStream_t st) {
    if (a.generic && a.n > 128) return rbc_fft_wide_built() ? rbc_launch_rs_fft_wide(a, st) : hipErrorInvalidValue;
    if (a.generic && a.n <= 32) return rbc_fft_small_built() ? rbc_launch_rs_fft_small(a, st) : hipErrorInvalidValue;
    if (a.generic) return rbc_fft_any_built() ? rbc_launch_rs_fft_any(a, st) : hipErrorInvalidValue;
    if (a.count <= 0) return hipSuccess;
    if (a.row_pitch % 4) return hipErrorInvalidValue;
    if (a.mode == GF_MODE_ENCODE_PARITY && !a.parity) return hipErrorInvalidValue;
#define RBC_FFT_CASE(lw, kk, nn) \
    if (a.n == nn && a.k == kk) return launch_fft<lw, kk, nn>(a, st);
    RBC_FFT_GEOMS(RBC_FFT_CASE)
#undef RBC_FFT_CASE
    return hipErrorInvalidValue;
}
