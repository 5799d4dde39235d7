// kernels.h -- argument blocks and launchers of the batched RBC kernels
// (host side of kernels.hip).  Plain structs passed by value to the kernels.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/rbc_gpu.h"
#include "host_shared.h"

// GF_MODE_ENCODE_PARITY: encode whose data rows and parity rows go to two
// buffers, data [I][k][pitch] and a dense parity arena [I][p][pitch]
// (rbc_dev_shard_commit_parity); rs_fft only, gf_rows takes GfArgs::parity
enum { GF_MODE_ENCODE = 0, GF_MODE_DECODE = 1, GF_MODE_ENCODE_PARITY = 2 };

struct GfArgs {
    int count;                 // instances
    int tiles;                 // column tiles per instance (gf_rows: 16 * tpb bytes; gf_regen: set by its launcher)
    int rc;                    // rows per chunk (template)
    int tpb;                   // gf_rows: threads per block, 256 (4 KiB tiles); 0 = 256
    int wpt;                   // gf_regen: words per lane (set by rbc_launch_gf_regen)
    int R, K;                  // output rows, input rows per instance
    int mode;                  // GF_MODE_*
    const uint8_t *in;         // encode: values [I][value_pitch]; decode: shards [I][N][pitch]
    uint64_t in_inst_pitch;
    uint32_t in_row_pitch;     // decode only
    uint32_t in_inst_bytes;    // readable bytes per instance (buffer bound)
    uint8_t *out;              // shards [I][N][pitch]
    uint64_t out_inst_pitch;
    uint32_t out_row_pitch;
    uint8_t *copy;             // encode: data rows written through; decode: used rows copied (out != in)
    const uint32_t *lens;      // encode: B_i; decode: S_i (nullptr -> uniform_len)
    uint32_t uniform_len;
    const uint8_t *coef;       // R x K bytes (+ inst * coef_inst_stride)
    uint64_t coef_inst_stride;
    const uint8_t *in_idx;     // decode: [I][idx_stride] input row positions (K used)
    const uint8_t *out_idx;    // decode: [I][idx_stride2] output row positions (R regen)
    uint32_t idx_stride, idx_stride2;
    const int32_t *status;     // skip instances with status != 0 (nullable)
    // decode compare mode (nmiss != nullptr): output rows r >= nmiss[inst] are
    // present-and-verified shards; they are compared with the regenerated
    // bytes instead of re-hashed, and only a mismatching row is stored,
    // flagged and appended to the hash list
    const int32_t *nmiss;
    uint32_t *flags;           // [I][n]
    uint32_t *list;            // (inst << 8 | pos) rows to hash
    uint32_t *counter;
    int n;
    const int32_t *rcount;     // per-instance output row count (nullable -> R)
    int prio;                  // wave issue priority 0..3 (set_wave_prio)
    // encode, optional: output row r goes to parity + inst * parity_inst_pitch +
    // r * out_row_pitch instead of row K + r of `out`; `copy` [I][K][out_row_pitch]
    // (out_inst_pitch = K * out_row_pitch) still receives the data rows
    uint8_t *parity;
    uint64_t parity_inst_pitch;
};

struct ShaArgs {
    int count;
    int rows_per_inst;         // row slots per instance
    const uint8_t *rows;       // [I][N][row_pitch]
    uint64_t inst_pitch;
    uint32_t row_pitch;
    const uint32_t *lens;      // S_i (nullable)
    uint32_t uniform_len;
    const uint8_t *idx;        // optional row positions [I][idx_stride]
    uint32_t idx_stride;
    const int32_t *status;     // nullable
    uint8_t *leaves;           // [I][N][32] (nullable)
    uint64_t leaves_inst_pitch;
    int per_message;           // 1: each instance is one ECHO message (leaf index = idx[inst])
    const uint64_t *row_offs;  // per_message: message i's bytes at rows + row_offs[i] (nullable: i * inst_pitch)
    const uint32_t *list;      // list mode: rows (inst << 8 | pos), count in *list_count
    const uint32_t *list_count;
    // verify
    int n, depth;
    const uint8_t *branches;   // [I][N][d][32]
    uint64_t br_inst_pitch;
    const uint8_t *roots;      // [I][32]
    const uint8_t *present;    // [I][N] (nullable -> all present)
    uint8_t *valid;            // [I][N]
    int prio;                  // wave issue priority 0..3 (set_wave_prio)
};

// validateMessage per message (sha_rows_kernel<true>, per_message): instance i
// is one ECHO of lens[i] bytes at rows + i * msg_pitch (a caller with packed
// messages sets row_offs instead) from leaf idx[i], its branch at branches +
// i * bslot and its root at roots + 32 i; valid[i] = the verdict, leaves
// (nullable) [count][32] = the message's leaf.  The caller adds what only it
// has: row_offs, row_pitch, status, prio.
inline ShaArgs sha_message_args(int count, int n, int depth, const uint8_t *rows, uint64_t msg_pitch,
                                const uint32_t *lens, const uint8_t *idx, const uint8_t *branches, uint64_t bslot,
                                const uint8_t *roots, uint8_t *valid, uint8_t *leaves = nullptr) {
    ShaArgs a{};
    a.count = count;
    a.rows_per_inst = 1;
    a.rows = rows;
    a.inst_pitch = msg_pitch;
    a.lens = lens;
    a.idx = idx;
    a.idx_stride = 1;
    a.leaves = leaves;
    a.leaves_inst_pitch = leaves ? 32 : 0;
    a.per_message = 1;
    a.n = n;
    a.depth = depth;
    a.branches = branches;
    a.br_inst_pitch = bslot;
    a.roots = roots;
    a.valid = valid;
    return a;
}

struct MerkleArgs {
    int count, n, width, depth, k;
    const uint8_t *leaves;     // [I][N][32]
    uint64_t leaves_inst_pitch;
    uint8_t *roots;            // build: out; check: recomputed root out (nullable)
    uint8_t *branches;         // build: [I][N][d][32] (nullable)
    uint64_t br_inst_pitch;
    const uint8_t *expect_roots;  // check
    int32_t *status;           // check: in/out
    uint8_t *digests;          // check: [I][32] (nullable)
    int trees_per_block;       // set by rbc_launch_merkle
    int prio;                  // wave issue priority 0..3 (set_wave_prio)
    const uint8_t *only;       // check: [I] nonzero = recheck this instance, others untouched (nullable = all)
    int stop_m;                // build, set by rbc_launch_merkle: stop at the layer of stop_m nodes (0 = root)
};

// merkle_recheck_kernel: the receive step's root recheck over the nodes ECHO
// verify established
struct RecheckArgs {
    int count, n, width, depth;
    const uint8_t *leaves;     // [I][N][32]: verified leaves + the regenerated rows' hashes
    uint64_t leaves_inst_pitch;
    const uint8_t *branches;   // [I][N][d][32]: the received ECHO branches
    uint64_t br_inst_pitch;
    const uint8_t *valid;      // [I][N]
    const uint32_t *flags;     // [I][N]: valid rows the re-encoding changed (decode compare)
    const uint8_t *vroots;     // [I][32]: the roots the branches were verified against
    const uint8_t *expect_roots;  // [I][32]
    int32_t *status;           // in/out
    uint8_t *need_full;        // [I] out: 1 = leave the instance to the full recheck (merkle_kernel<true>, only)
    int inst_per_block;        // set by rbc_launch_recheck
    int prio;
};
hipError_t rbc_launch_recheck(const RecheckArgs &a, hipStream_t st);

// merkle_path_kernel: shared-path branch verification over precomputed leaves
struct PathArgs {
    int count, n, width, lg_width, depth;
    const uint8_t *leaves;     // [I][N][32]
    uint64_t leaves_inst_pitch;
    const uint8_t *branches;   // [I][N][d][32]
    uint64_t br_inst_pitch;
    const uint8_t *roots;      // [I][32]
    const uint8_t *present;    // [I][N] (nullable -> all present)
    const int32_t *status;     // nullable
    uint8_t *valid;            // [I][N]
    int inst_per_block;        // set by rbc_launch_merkle_path
    int prio;                  // wave issue priority 0..3 (set_wave_prio)
};

struct PrepArgs {
    int count, n, k;
    const uint8_t *valid;      // [I][valid_stride]
    uint32_t valid_stride;
    const uint8_t *M;          // encode matrix [n][k]
    uint8_t *used;             // [I][used_stride]   first k valid positions
    uint32_t used_stride;
    uint8_t *regen;            // [I][regen_stride]  the other n-k positions
    uint32_t regen_stride;
    uint8_t *dmat;             // [I][dmat_stride] = (n-k) x k decode matrix
    uint64_t dmat_stride;
    int32_t *status;           // out
    // compare mode: regen = [missing..., present-unused...], nmiss[i] = #missing,
    // missing rows appended to list, flags[i][*] zeroed
    int32_t *nmiss;
    uint32_t *flags;
    uint32_t *list;
    uint32_t *counter;
    // FFT codec: D covers only the missing data rows (rcount[i] of them, they
    // lead `regen`); cls[i][pos] = 0 skip / 1 store / 2 compare for pos >= k
    int fft;
    int32_t *rcount;
    uint8_t *cls;
    uint32_t cls_stride;
    const uint8_t *gf_exp;     // device exp[512] / log[256] tables (FFT prepare)
    const uint8_t *gf_log;
    int prio;                  // wave issue priority 0..3 (set_wave_prio)
};

struct JoinArgs {
    int count, k;
    uint32_t chunks;           // 16-byte chunks per instance (= value_pitch / 16)
    uint32_t blocks_per_inst;  // set by rbc_launch_join
    const uint8_t *shards;     // full codeword rows
    uint64_t inst_pitch;
    uint32_t row_pitch;
    uint32_t inst_bytes;       // readable bytes per instance
    const uint32_t *lens;      // S_i (nullable)
    uint32_t uniform_len;
    uint8_t *values;           // [I][value_pitch]
    uint32_t value_pitch;
    const int32_t *status;
    int prio;                  // wave issue priority 0..3 (set_wave_prio)
};

// rs_fft_kernel (rs_fft.hip): additive-FFT systematic encode, one lane per
// dword column of one instance
struct FftArgs {
    int count, n, k;
    int mode;                  // GF_MODE_ENCODE: values -> data + parity rows;
                               // GF_MODE_DECODE: data rows -> parity rows by class
    const uint8_t *values;     // encode: [I][value_pitch]
    uint32_t value_pitch;
    uint8_t *shards;           // [I][N][row_pitch]
    uint64_t inst_pitch;
    uint32_t row_pitch;
    const uint32_t *lens;      // encode: B_i, decode: S_i (nullable)
    uint32_t uniform_len;
    const int32_t *status;     // nullable
    // decode: per-position class [I][cls_stride] (0 skip, 1 store, 2 compare);
    // nullptr -> store every parity position
    const uint8_t *cls;
    uint32_t cls_stride;       // multiple of 4
    uint32_t *flags;           // [I][n]
    uint32_t *list;
    uint32_t *counter;
    int prio;                  // wave issue priority 0..3 (set_wave_prio)
    // decode, optional: also assemble interpolate's value from the k data rows
    // the kernel loads anyway -- join[i][0 .. k*S) = data rows 0..k-1 of S
    // bytes, zeros up to join_pitch (uniform S only, join_pitch - k*S < 256)
    uint8_t *join;
    uint32_t join_pitch;
    // GF_MODE_ENCODE_PARITY: `shards` is the data rows [I][k][row_pitch]
    // (inst_pitch = k * row_pitch); parity position pos is stored at
    // parity + inst * parity_inst_pitch + (pos - k) * row_pitch
    uint8_t *parity;           // [I][n-k][row_pitch]
    uint64_t parity_inst_pitch;
    int generic;               // run the run-time-geometry transform (rs_fft_any.hip; n > 128: rs_fft_wide.hip;
                               // n <= 32: rs_fft_small.hip)
    int lane;                  // rs_fft_small.hip only: dword columns per lane, 0 = rbc_fft_small_lane's choice
};

// VAL / ECHO marshaling (wire.hip): message (i, j) = pb.Message bytes of
// the request for shard j of instance i, at out + (i*n + j)*out_pitch.
struct WireArgs {
    int count, n, depth, type;
    const uint8_t *shards;
    uint64_t inst_pitch;
    uint32_t row_pitch;
    const uint32_t *lens;  // per instance, or NULL: uniform_len
    uint32_t uniform_len;
    const uint8_t *branches;  // [count][n][depth][32]
    const uint8_t *roots;     // [count][32]
    uint8_t *out;
    uint64_t out_pitch;  // % 16 == 0
    uint32_t *out_lens;  // [count*n], nullable
    int codec;           // payload codec (include/rbc_protocol.h): 0 JSON, 1 binary
};
hipError_t rbc_launch_marshal_val(const WireArgs &a, hipStream_t st);

// The three wire launchers choose their kernel by the `codec` field of their
// arguments (include/rbc_protocol.h, RBC_HAS_WIRE_BINARY): 0 the Go-JSON
// payload, 1 the binary one (marshal_val_bin_kernel, unmarshal_val_bin_kernel,
// unmarshal_echo_bin_kernel), with the same output contracts; any other value
// is hipErrorInvalidValue.
//
// Per-message status of the unmarshal kernel (include/rbc_protocol.h)
enum { WIRE_OK = 0, WIRE_FALLBACK = 1, WIRE_OTHER_ROOT = 2, WIRE_OTHER_LEN = 3 };

// VAL / ECHO unmarshaling (wire.hip), the inverse: message i is the bytes
// msgs[offs[i], offs[i] + lens[i]) from the node at Merkle leaf idx[i].  A
// canonical message (byte-for-byte what marshal_val_kernel writes) has its
// fields decoded to the device forms; every other one only gets status
// WIRE_FALLBACK.  The kernel reads msgs[offs[i], offs[i] + round_up(lens[i], 16))
// at most and writes nothing outside message i's own output slots.
struct WireRxArgs {
    int count, n, depth;
    const uint8_t *msgs;
    const uint64_t *offs;  // % 16 == 0
    const uint32_t *lens;
    const uint8_t *idx;    // sender's leaf index
    uint8_t *rows;         // shard i at rows + i*row_pitch, zeros up to round_up(S, 64)
    uint32_t row_pitch;    // % 64 == 0
    uint32_t *shard_lens;  // [count] (0 for a fallback message)
    uint8_t *branches;     // [count][max(depth,1)][32], device form
    uint8_t *roots;        // [count][32]
    uint8_t *types;        // [count]
    int32_t *status;       // [count] WIRE_OK / WIRE_FALLBACK
    int codec;             // payload codec: 0 JSON, 1 binary
};
hipError_t rbc_launch_unmarshal_val(const WireRxArgs &a, hipStream_t st);

// ECHO unmarshaling into the receiver's batch layout (wire.hip,
// unmarshal_echo_kernel): message m, read like WireRxArgs' message i, belongs
// to instance inst[m] and goes to slot r = inst[m]*n + idx[m] of shards /
// branches / present -- the rbc_rx_batch layout, so every shard is written
// once, where verify and decode read it.  Status in this order: shape not
// derivable (WireRxArgs' rule, inst[m] >= count included) -> WIRE_FALLBACK;
// derived S != the instance's length -> WIRE_OTHER_LEN, nothing of the slot
// written; a byte not canonical -> WIRE_FALLBACK; the message's root (decoded
// in registers, never stored) != roots[inst[m]] -> WIRE_OTHER_ROOT; else
// WIRE_OK and present[r] = 1.  Nothing is written outside message m's own
// slots; two messages naming one slot are the caller's error.
struct WireEchoArgs {
    int count, msgs, n, depth;   // instances, messages
    const uint8_t *ring;
    const uint64_t *offs;        // [msgs] % 16 == 0
    const uint32_t *lens;        // [msgs]
    const uint32_t *inst;        // [msgs] < count
    const uint8_t *idx;          // [msgs] sender's leaf index
    const uint8_t *roots;        // [count][32] the root each instance collects ECHOs for
    const uint32_t *shard_lens;  // [count], or NULL: uniform_len
    uint32_t uniform_len;
    uint8_t *shards;             // [count][n][shard_pitch], zeros from S to round_up(S, 64)
    uint32_t shard_pitch;        // % 64 == 0
    uint8_t *branches;           // [count][n][max(depth,1)][32], device form
    uint8_t *present;            // [count][n]: 1 written for WIRE_OK, else untouched
    int32_t *msg_status;         // [msgs]
    uint8_t *types;              // [msgs], nullable
    int codec;                   // payload codec: 0 JSON, 1 binary
};
hipError_t rbc_launch_unmarshal_echo(const WireEchoArgs &a, hipStream_t st);

// READY unmarshaling (wire.hip, unmarshal_ready_kernel): message m, read like
// WireEchoArgs' message m, is a READY of the member at leaf idx[m] for
// instance inst[m].  READY has one canonical form of one length under both
// payload codecs: rbc_pb_encode_rbc(RBC_MSG_READY, rbc_json_encode_ready(root, 32)).
// Status in this order: lens[m] != msg_len, inst[m] >= count or idx[m] >= n
// (decided before any byte of the message is read) -> WIRE_FALLBACK; a byte
// not canonical -> WIRE_FALLBACK; the root (decoded in registers, never stored)
// != roots[inst[m]] -> WIRE_OTHER_ROOT; else WIRE_OK and
// ready[inst[m]*n + idx[m]] = 1.  A message writes msg_status[m] and that one
// byte only; the kernel never clears a byte of ready, so two messages naming
// one slot store the same 1.
struct WireReadyArgs {
    int count, msgs, n;        // instances, messages, members
    uint32_t msg_len;          // the host encoder's READY size; the launcher rejects any other than the kernel's
    const uint8_t *ring;
    const uint64_t *offs;      // [msgs] % 16 == 0
    const uint32_t *lens;      // [msgs]
    const uint32_t *inst;      // [msgs] < count
    const uint8_t *idx;        // [msgs] sender's leaf index
    const uint8_t *roots;      // [count][32] the root each instance collects READYs for
    uint8_t *ready;            // [count][n]: 1 written for WIRE_OK, else untouched
    int32_t *msg_status;       // [msgs]
};
hipError_t rbc_launch_unmarshal_ready(const WireReadyArgs &a, hipStream_t st);

// Per-instance quorum tally (wire.hip, quorum_kernel): E = non-zero bytes of
// valid[i][0..n) (valid NULL: 0), R = non-zero bytes of ready[i][0..n), st =
// status[i] (status NULL: nothing is known, `have` is false).
//   have       = st == 0 && (E >= n-f || (R >= 2f+1 && E >= n-2f))
//   send_ready = R >= f+1 || have
//   if send_ready && self >= 0 && !ready[i][self]: ready[i][self] = 1, R += 1
//   deliver    = st == 0 && R >= 2f+1 && E >= n-2f
// flags[i]: 1 E >= n-f, 2 R >= f+1 before the own bit, 4 send_ready, 8 deliver.
struct QuorumArgs {
    int count, n, f, self;     // self in [-1, n): -1 turns the own-READY write off
    const uint8_t *valid;      // [count][n], nullable
    uint8_t *ready;            // [count][n]; only ready[i][self] is ever written
    const int32_t *status;     // [count], nullable
    uint32_t *echo_counts;     // [count] E
    uint32_t *ready_counts;    // [count] R after the own bit
    uint8_t *flags;            // [count]
};
enum { QUORUM_ECHO = 1, QUORUM_AMPLIFY = 2, QUORUM_SEND_READY = 4, QUORUM_DELIVER = 8 };
hipError_t rbc_launch_quorum(const QuorumArgs &a, hipStream_t st);

// a.generic == 0: rs_fft_kernel<LOGW, K, N> (rs_fft.hip, the RBC_FFT_GEOMS geometries); else it
// hands over to rbc_launch_rs_fft_any (rs_fft_any.hip: n and k at run time, no fused join).
// That one is a weak reference: a relink of the library from a fixed list of objects (the test
// mutants, a host-only build) has no rs_fft_any.o; there the form counts as not built
// (rbc_fft_any_built), and rbc_ctx_set_codec refuses it.  With a.generic and n > 128 it hands over
// to rbc_launch_rs_fft_wide (rs_fft_wide.hip, 129 <= n <= 256), with a.generic and n <= 32 to
// rbc_launch_rs_fft_small (rs_fft_small.hip, 2 <= n <= 32), weak references in the same way.
hipError_t rbc_launch_rs_fft(const FftArgs &a, hipStream_t st);
hipError_t rbc_launch_rs_fft_any(const FftArgs &a, hipStream_t st) __attribute__((weak));
inline bool rbc_fft_any_built() { return rbc_launch_rs_fft_any != nullptr; }
hipError_t rbc_launch_rs_fft_wide(const FftArgs &a, hipStream_t st) __attribute__((weak));
inline bool rbc_fft_wide_built() { return rbc_launch_rs_fft_wide != nullptr; }
hipError_t rbc_launch_rs_fft_small(const FftArgs &a, hipStream_t st) __attribute__((weak));
inline bool rbc_fft_small_built() { return rbc_launch_rs_fft_small != nullptr; }

int rbc_gf_pick_rc(int R, int rcmax);  // GfArgs::rc; the rule is host_shared.h's rbc_gf_pick_rc_impl
hipError_t rbc_launch_gf_rows(const GfArgs &a, hipStream_t st);
// interpolate's missing data rows (FFT codec, gf_regen.hip): one wave per column tile of 256 * W
// bytes owns every row (W and the tiles chosen from the row length); needs rcount (row count <= R)
hipError_t rbc_launch_gf_regen(const GfArgs &a, hipStream_t st);
hipError_t rbc_launch_sha_rows(const ShaArgs &a, bool verify, hipStream_t st);
// receive step: v's rows (list or all; branch walk + verdict when v_walk) and
// r's listed regen rows in one launch (count <= 0 disables a side)
// zero0 / zero1 (nullable, 16 B each): counters one lane zeroes during the launch (receive step)
hipError_t rbc_launch_sha_rx(const ShaArgs &v, const ShaArgs &r, bool v_walk, hipStream_t st, uint4 *zero0 = nullptr,
                             uint4 *zero1 = nullptr);
hipError_t rbc_launch_merkle(const MerkleArgs &a, bool check, hipStream_t st);
hipError_t rbc_launch_merkle_path(const PathArgs &a, hipStream_t st);
hipError_t rbc_launch_decode_prepare(const PrepArgs &a, hipStream_t st);
hipError_t rbc_launch_digest(const uint8_t *leaves, uint64_t leaves_inst_pitch, int k, const int32_t *status,
                             uint8_t *digests, int count, hipStream_t st, int prio = 0);
hipError_t rbc_launch_join(const JoinArgs &a, hipStream_t st);
hipError_t rbc_launch_inject_faults(uint8_t *shards, uint64_t inst_pitch, uint32_t row_pitch,
                                    const int32_t *corrupt, int count, hipStream_t st);
// roots_src -> roots_dst (nullable): each instance's 32-B root copied on the way (receive step)
hipError_t rbc_launch_compact_present(const uint8_t *present, int n, int count, uint8_t *valid, uint32_t *list,
                                     uint32_t *counter, hipStream_t st, int prio = 0,
                                     const uint8_t *roots_src = nullptr, uint8_t *roots_dst = nullptr);
hipError_t rbc_launch_pack_records(const uint8_t *roots, const uint8_t *digests, const int32_t *status, int count,
                                   int slots, uint8_t *out, hipStream_t st);
hipError_t rbc_launch_fill_random(uint8_t *dst, uint64_t first_row, uint64_t rows, uint64_t pitch, uint64_t seed,
                                  hipStream_t st);
// present rows of a pinned host batch -> device rows (zero-copy reads), absent rows zeroed
hipError_t rbc_launch_gather_present(const uint8_t *host, uint64_t hpitch, uint32_t S, const uint8_t *present,
                                     uint8_t *dev, uint32_t dpitch, uint32_t rows, hipStream_t st);
// the messages of a pinned validate arena -> the same offsets of a device arena
// (zero-copy reads of bytes [offs[i], offs[i] + lens[i]) only; the rest untouched)
hipError_t rbc_launch_gather_msgs(const uint8_t *host, const uint64_t *offs, const uint32_t *lens, uint32_t count,
                                  uint8_t *dev, uint32_t avg_len, hipStream_t st);
// pinned host values (device array of their addresses) -> device value rows (zero-copy reads)
// rows [0, width) of src (src_pitch) into dst at dst_pitch, zeros to dst_pitch
hipError_t rbc_launch_pack_rows(const uint8_t *src, uint32_t src_pitch, uint8_t *dst, uint32_t dst_pitch,
                                uint32_t width, uint32_t rows, hipStream_t st);
// rows from device addresses (0 = absent), lens per instance of n rows
hipError_t rbc_launch_gather_ptrs(const uint64_t *ptrs, const uint32_t *lens, uint32_t n, uint8_t *dev,
                                  uint32_t dpitch, uint32_t rows, hipStream_t st);
hipError_t rbc_launch_gather_values(const uint64_t *ptrs, const uint32_t *lens, uint32_t count, uint8_t *dev,
                                    uint64_t vpitch, hipStream_t st);
hipError_t rbc_launch_count_mismatch(const uint8_t *a, uint64_t a_pitch, const uint8_t *b, uint64_t b_pitch,
                                     uint64_t rows, uint64_t len, uint32_t *counter, hipStream_t st);
hipError_t rbc_launch_count_mismatch_rows(const uint8_t *shards, uint64_t inst_pitch, uint32_t row_pitch, int k,
                                          uint32_t S, const uint8_t *values, uint64_t value_pitch, uint32_t B,
                                          uint64_t count, uint32_t *counter, hipStream_t st);
// receive-guard input: absent rows (present == 0) and corrupt[i] filled with seeded garbage
hipError_t rbc_launch_poison_rows(uint8_t *shards, uint64_t inst_pitch, uint32_t row_pitch, int n,
                                  const uint8_t *present, const int32_t *corrupt, uint64_t count, uint64_t seed,
                                  hipStream_t st);
