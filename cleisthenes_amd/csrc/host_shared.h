// host_shared.h -- host-side facts shared by the HIP launchers and the host
// runtime (capi.cpp), kept in a header so a host-only build of the runtime
// (the sanitizer build in tests/test_sanitizers.py) needs no HIP compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

// Geometries with a specialised additive-FFT transform (rs_fft.hip): N = 3f+1
// (the BFT maximum f) for the benchmark sizes, as X(log2 N, k, N).  Other
// (N, k) use gf_rows_kernel.
#define RBC_FFT_GEOMS(X) \
    X(2, 2, 4)           \
    X(4, 6, 16)          \
    X(6, 22, 64)         \
    X(7, 44, 128)        \
    X(8, 86, 256)

inline bool rbc_fft_supported(int n, int k) {
#define RBC_FFT_SUP(lw, kk, nn) \
    if (n == nn && k == kk) return true;
    RBC_FFT_GEOMS(RBC_FFT_SUP)
#undef RBC_FFT_SUP
    return false;
}

// The run-time-geometry transform (rs_fft_any.hip): any 1 <= k <= n with
// 33 <= n <= 128; its width is the smallest power of two >= n.  (No W = 256
// kernel: it does not fit the register file without scratch.)
inline bool rbc_fft_any_supported(int n, int k) { return n >= 33 && n <= 128 && k >= 1 && k <= n; }
// The same for 129 <= n <= 256 (rs_fft_wide.hip): two 128-row halves, the idle
// one parked in the LDS.  A form of its own, chosen only by RBC_CODEC_FFT_WIDE.
inline bool rbc_fft_wide_supported(int n, int k) { return n >= 129 && n <= 256 && k >= 1 && k <= n; }
// The same for 2 <= n <= 32 (rs_fft_small.hip), at width 8, 16 or 32: the smallest
// of them >= n.  A form of its own, chosen only by RBC_CODEC_FFT_SMALL, at (4, 1)
// and (16, 5) too.
inline bool rbc_fft_small_supported(int n, int k) { return n >= 2 && n <= 32 && k >= 1 && k <= n; }
inline int rbc_fft_small_logw(int n) { return n <= 8 ? 3 : n <= 16 ? 4 : 5; }
// Its lane width: the adjacent dword columns a lane owns, 1 (a wave covers 256 B
// of each row) or the wider one built for the width W: 4 (1 KiB) at W = 8 and 16,
// 2 (512 B) at W = 32, where four columns of 32 rows and of the solve's 16-row
// copy do not fit 256 registers without scratch.  0 asks for rbc_fft_small_lane's
// choice.
constexpr int rbc_fft_small_wide_lane(int W) { return W <= 16 ? 4 : 2; }
inline bool rbc_fft_small_lane_valid(int n, int lane) {
    return lane == 0 || lane == 1 || (n <= 32 && lane == rbc_fft_small_wide_lane(1 << rbc_fft_small_logw(n)));
}
// The automatic choice, a function of the width W and the row pitch alone: the
// wider lane only in the (W, row length) classes where, measured against lane 1
// in one process, it won a call (disjoint min-max ranges) and lost none; lane 1
// on ties, on mixed results and between the two row lengths that were measured
// ("the small form", profiles/fft_small/):
//   W = 8,  rows of 5.5 KB: encode and receive won, commit tied; rows of 350 KB: encode lost.
//   W = 16: receive won at both lengths, encode or commit lost at (13, 4) and (16, 5): mixed.
//   W = 32, rows of 95 to 150 KB: receive won at (19, 6), (25, 8), (31, 10), encode and commit
//           tied; rows of 1.5 to 2.3 KB: receive won, encode or commit lost: mixed.
constexpr uint32_t kFftSmallLane8MaxPitch = 8u << 10;    // W = 8: the wider lane up to here
constexpr uint32_t kFftSmallLane32MinPitch = 64u << 10;  // W = 32: the wider lane from here
inline int rbc_fft_small_lane(int W, uint32_t row_pitch) {
    if (W == 8 && row_pitch <= kFftSmallLane8MaxPitch) return rbc_fft_small_wide_lane(W);
    if (W == 32 && row_pitch >= kFftSmallLane32MinPitch) return rbc_fft_small_wide_lane(W);
    return 1;
}

// Trees (merkle_kernel) or instances (merkle_recheck_kernel) packed into each
// one-wave block of `count` trees of `width` leaves: up to 512 / W (<= 64, 16 KiB
// of node LDS), halved until the grid has >= 512 blocks so that a small batch
// still spreads over every CU (C2 and C4: 2 trees per block).
// (C4, W = 256, measured: 1 tree per block 0.68 ms, 2 trees 0.63, 4 trees 0.95;
// in the pipelined step 4 trees per block equal to 2 at C2 and C4, gpu_r04l.sh)
inline int rbc_trees_per_block(int width, int count) {
    int g = width >= 512 ? 1 : (512 / width < 64 ? 512 / width : 64);
    while (g > 1 && (count + g - 1) / g < 512) g >>= 1;
    return g;
}

// Rows per GF chunk (accumulators held in VGPRs) of the matrix codec.
constexpr int kGfRcMax = 21;
// The RC values gf_rows_kernel is instantiated for (rbc_launch_gf_rows).
constexpr int kRC[] = {1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17,
                       18, 19, 20, 21, 22, 23, 24, 26, 28, 30, 32, 36, 40, 42, 44, 48};

// The body of rbc_gf_pick_rc (kernels.h; defined beside the launchers in
// kernels.hip, so a host-only build may link a stand-in for it).
inline int rbc_gf_pick_rc_impl(int R, int rcmax) {
    // fewest chunks of <= rcmax rows, then the smallest instantiated RC covering them
    if (R <= 0) return 1;
    if (rcmax < 1) rcmax = 1;
    if (rcmax > 48) rcmax = 48;
    const int chunks = (R + rcmax - 1) / rcmax;
    const int want = (R + chunks - 1) / chunks;
    for (int rc : kRC)
        if (rc >= want) return rc;
    return 48;
}

// The form of gf_regen_kernel (gf_regen.hip) that rbc_launch_gf_regen runs: one
// wave per column tile of 64 lanes x W words owns every missing row, in passes
// of at most RC rows (one straight-line body per exact row count 1..RC), NT
// tiles to a block.  512-B tiles (W = 2), or 256-B tiles (W = 1) for rows of at
// most 2 KiB, where they keep the lanes busy (C4: S = 763 -> 3 tiles, 99 %).
// The row length is the uniform one, or the pitch when lengths are per instance.
constexpr int kRegenRowsShort = 40, kRegenTilesShort = 3;  // W = 1 (C4: m ~ 29 +- 4 of k = 86 in one pass)
constexpr int kRegenRowsLong = 24, kRegenTilesLong = 4;    // W = 2 (C1-C3: m ~ 7-15 of k = 22-44)
struct RbcRegenForm {
    int W, RC, NT;
};
inline RbcRegenForm rbc_gf_regen_form(bool per_instance_lens, uint32_t uniform_len, uint32_t row_pitch) {
    const uint32_t S = per_instance_lens ? row_pitch : uniform_len;
    if (S <= 2048) return {1, kRegenRowsShort, kRegenTilesShort};
    return {2, kRegenRowsLong, kRegenTilesLong};
}

// klauspost Split's data shards without copying whole rows (rbc/rbc.go:97-100:
// Split returns slices of the caller's value, and allocates only where it has
// to pad).  With S = ceil(len / k), row j is data[j*S, (j+1)*S) itself while it
// lies wholly inside the value; the other rows live in `tail`: the row that
// straddles len (its remaining bytes, then zeros) and the all-zero rows after it.
inline size_t rbc_split_tail_bytes_impl(int k, size_t len) {
    if (k <= 0 || len == 0) return 0;
    const size_t S = (len + (size_t)k - 1) / (size_t)k;
    return ((size_t)k - len / S) * S;
}
// Status values are include/rbc_gpu.h's RBC_OK (0), RBC_ERR_SHORT_DATA (-6) and
// RBC_ERR_INVALID_ARG (-10); nothing is written unless RBC_OK is returned.
inline int rbc_split_rows_impl(int k, const uint8_t *data, size_t len, uint8_t *tail, size_t tail_cap,
                               const uint8_t **rows_out, size_t *shard_len, size_t *tail_used) {
    if (k <= 0 || !rows_out) return -10;
    if (len == 0) return -6;  // Split: len(data) == 0
    if (!data) return -10;
    const size_t S = (len + (size_t)k - 1) / (size_t)k;
    const size_t full = len / S;  // rows with (j+1)*S <= len
    const size_t need = ((size_t)k - full) * S;
    if (need > tail_cap || (need && !tail)) return -10;
    for (size_t j = 0; j < full; ++j) rows_out[j] = data + j * S;
    if (need) {
        const size_t rem = len - full * S;  // bytes of the straddling row that are data
        for (size_t b = 0; b < rem; ++b) tail[b] = data[full * S + b];
        for (size_t b = rem; b < need; ++b) tail[b] = 0;
        for (size_t j = full; j < (size_t)k; ++j) rows_out[j] = tail + (j - full) * S;
    }
    if (shard_len) *shard_len = S;
    if (tail_used) *tail_used = need;
    return 0;
}

// Bytes of the pb.Message of a VAL (type 0) / ECHO (1) request for shard
// `index` of S bytes with a depth-`depth` branch: the host mirror of the
// marshal kernel's layout().total (wire.hip), for sizing out_pitch.
inline size_t rbc_val_message_bytes(int n, int depth, uint32_t S, uint32_t index, int type) {
    auto b64 = [](uint64_t x) { return (x + 2) / 3 * 4; };
    auto vl = [](uint64_t v) {
        uint64_t l = 1;
        while (v >= 0x80) {
            v >>= 7;
            ++l;
        }
        return l;
    };
    const bool empty0 = depth > 0 && (int)(index ^ 1u) >= n;
    const uint64_t br = 32u * (uint64_t)(depth - (empty0 ? 1 : 0));
    const uint64_t J = br ? 84 + b64(br) + b64(S) : 86 + b64(S);
    const uint64_t R = 1 + vl(J) + J + (type ? 2 : 0);
    return (size_t)(1 + vl(R) + R);
}

// The same for a payload codec (include/rbc_protocol.h: 0 JSON, 1 binary, whose
// payload is 40 + branch + S bytes; the mirror of wire.hip's bin_layout().total);
// 0 for an unknown codec.
inline size_t rbc_val_message_bytes_codec(int codec, int n, int depth, uint32_t S, uint32_t index, int type) {
    if (codec == 0) return rbc_val_message_bytes(n, depth, S, index, type);
    if (codec != 1) return 0;
    auto vl = [](uint64_t v) {
        uint64_t l = 1;
        while (v >= 0x80) {
            v >>= 7;
            ++l;
        }
        return l;
    };
    const bool empty0 = depth > 0 && (int)(index ^ 1u) >= n;
    const uint64_t J = 40 + 32u * (uint64_t)(depth - (empty0 ? 1 : 0)) + S;
    const uint64_t R = 1 + vl(J) + J + (type ? 2 : 0);
    return (size_t)(1 + vl(R) + R);
}
