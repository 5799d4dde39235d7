/* rbc_protocol.h -- the RBC state machine above the data path (SURVEY §8f
 * rank 1-3), in C++ behind a C ABI because the reference's own language (Go)
 * is absent from this image.
 *
 * Mirrors rbc/rbc.go:9-100 (NewRBC, HandleMessage, handleValueRequest /
 * handleEchoRequest / handleReadyRequest, Value, Messages) and the request
 * types of rbc/request.go:9-21, exchanged as pb.Message (pb/message.proto:11-35;
 * the generated code carries RBC.type as field 2, pb/message.pb.go:182-183).
 *
 * Protocol (docs/RBC-EN.md, HBBFT): the proposer sends VAL(h, b_j, s_j) to
 * node j; a node multicasts ECHO(h, b_i, s_i) for the VAL it received; an ECHO
 * from node j counts iff validateMessage proves s_j at leaf j under h; with
 * N-f valid ECHOs for h the node interpolates and, when the re-encoded root
 * matches h, multicasts READY(h); f+1 READY(h) make it multicast READY(h) too;
 * 2f+1 READY(h) plus N-2f valid ECHOs deliver the value.
 *
 * Payload codec (unpinned by the reference: its handlers are stubs): the
 * request structs marshaled by Go encoding/json -- fields in struct order,
 * []byte as standard base64, nil slices as null, EchoRequest's embedded
 * ValRequest promoted: {"RootHash":"..","Branch":"..","Block":[".."]} and
 * {"RootHash":".."}.  Branch is the Go flat form (the non-empty siblings,
 * leaf to root) that rbc_validate_message takes.
 *
 * GPU work (shard + commit, validateMessage, interpolate) is submitted to an
 * rbc_batcher without blocking, so every instance and node of the process
 * shares launches; rbc_node_progress completes it.  Node indices are the
 * positions in the sorted member list (= Merkle leaf index). */
#ifndef RBC_PROTOCOL_H
#define RBC_PROTOCOL_H

#include <stddef.h>
#include <stdint.h>

#include "rbc_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RBC_MSG_VAL 0   /* pb.RBC_VAL   */
#define RBC_MSG_ECHO 1  /* pb.RBC_ECHO  */
#define RBC_MSG_READY 2 /* pb.RBC_READY */
#define RBC_ERR_PROTOCOL (-20) /* malformed or out-of-protocol message */

/* ---- codec (host only, no GPU) ------------------------------------------- */
/* pb.Message{rbc: pb.RBC{payload, type}} (signature/timestamp unset).
 * Returns the encoded size; writes only when it fits in cap. */
size_t rbc_pb_encode_rbc(int type, const uint8_t *payload, size_t payload_len, uint8_t *out, size_t cap);
/* Parse a pb.Message carrying an RBC: *type, *payload (points into msg). */
int rbc_pb_decode_rbc(const uint8_t *msg, size_t len, int *type, const uint8_t **payload, size_t *payload_len);
/* Go encoding/json of ValRequest / EchoRequest (one shape, block = Block[0];
 * block_len 0 -> "Block":null) and ReadyRequest.  Returns the size; writes
 * only when it fits. */
size_t rbc_json_encode_val(const uint8_t *root, size_t root_len, const uint8_t *branch, size_t branch_len,
                           const uint8_t *block, size_t block_len, uint8_t *out, size_t cap);
size_t rbc_json_encode_ready(const uint8_t *root, size_t root_len, uint8_t *out, size_t cap);
/* json.Unmarshal of the same shapes (keys case-insensitive, unknown keys
 * skipped): RootHash must be 32 bytes and Block hold exactly one shard.
 * RBC_ERR_PROTOCOL when malformed; RBC_ERR_INVALID_ARG (lens set) when a
 * buffer is short. */
int rbc_json_decode_val(const uint8_t *json, size_t len, uint8_t *root_out, uint8_t *branch_out, size_t branch_cap,
                        size_t *branch_len, uint8_t *block_out, size_t block_cap, size_t *block_len);
int rbc_json_decode_ready(const uint8_t *json, size_t len, uint8_t *root_out);

/* ---- device-side marshaling (the proposer's per-recipient VAL send path) --
 * For every instance i and row j, writes the pb.Message bytes of VAL / ECHO
 * (type) carrying (roots[i], flat branch j, shard j) -- byte-identical to
 * rbc_pb_encode_rbc(type, rbc_json_encode_val(...)) -- to
 * out + (i*n + j)*out_pitch, and out_lens[i*n + j] = its size (nullable).
 * Inputs in the rbc_dev_* layout (rbc_gpu.h): shards [count][n][shard_pitch],
 * branches [count][n][d][32], roots [count][32].  out_pitch % 16 == 0 and
 * >= round_up(rbc_val_message_size(n, S_max, 0, type), 16); bytes past a
 * message up to the next 16 are zeroed. */
int rbc_dev_marshal_val(rbc_ctx *ctx, void *stream, int count, int type, const uint8_t *shards,
                        uint32_t shard_pitch, const uint32_t *shard_lens, uint32_t uniform_shard_len,
                        const uint8_t *branches, const uint8_t *roots, uint8_t *out, uint64_t out_pitch,
                        uint32_t *out_lens);
/* Size of that message for shard length S at leaf `index` of an n-node tree. */
size_t rbc_val_message_size(int n, uint32_t shard_len, uint32_t index, int type);

/* The proposer's send path in one call (the gap at
 * conn.go:182-208, where Broadcaster.Broadcast sends one message to all while
 * VAL differs per recipient): shard + commit `count` proposals (host values),
 * marshal every per-recipient VAL on the device, and move the finished
 * pb.Message bytes to the caller's ring in ONE device-to-host copy:
 * msgs [count][n][msg_pitch] (message (i, j) for member j at
 * msgs + (i*n + j)*msg_pitch, msg_lens [count][n] bytes), roots_out
 * [count][32] (nullable).  msg_pitch % 16 == 0 and >= the largest
 * rbc_val_message_size(n, S_max, index, RBC_MSG_VAL).  Ring memory from
 * rbc_host_alloc is written directly by the DMA engine (no staging copy);
 * a gRPC writer sends msgs[i][j][:len] to member j with a pass-through codec
 * (INTEGRATION.md).  Asynchronous: complete with rbc_wait / rbc_poll. */
int rbc_shard_commit_val(rbc_ctx *ctx, int count, const uint8_t *const *values, const size_t *value_lens,
                         uint8_t *msgs, size_t msg_pitch, uint32_t *msg_lens, uint8_t *roots_out,
                         uint64_t *ticket);

/* ---- device-side unmarshaling (the receive path of VAL / ECHO) ------------
 * The mirror of rbc_dev_marshal_val, present when RBC_HAS_WIRE_RX is defined
 * (the ABI version stays 7: detect the addition by symbol).  Message i is the
 * raw pb.Message bytes msgs[offs[i], offs[i] + lens[i]) as a pass-through gRPC
 * codec hands them over, sent by the member at Merkle leaf idx[i].
 * offs[i] % 16 == 0 and the arena holds round_up(lens[i], 16) bytes from
 * offs[i]: the kernel reads no byte outside that range, whatever the message
 * says.
 *
 * A message is decoded when it is canonical: byte-for-byte what
 * rbc_pb_encode_rbc(type, rbc_json_encode_val(root, branch, block)) emits for
 * a 32-byte root, the flat branch of leaf idx[i] (32 bytes per non-empty
 * level), one block of 1..row_pitch bytes and type VAL or ECHO.  Then
 * status_out[i] = RBC_WIRE_OK and types_out[i], roots_out[i][32],
 * branches_out[i][max(depth,1)][32] (the rbc_dev_* form: a zero slot for an
 * empty level-0 sibling), shard_lens_out[i] = S and the shard at
 * rows + i*row_pitch (zeros from S to round_up(S, 64)) equal what
 * rbc_pb_decode_rbc + rbc_json_decode_val return for the same bytes.
 * Every other message -- whitespace, escapes, CR / LF inside base64, keys in
 * another case or order, unknown keys, READY, a branch of another length,
 * anything malformed -- gets status_out[i] = RBC_WIRE_FALLBACK and
 * shard_lens_out[i] = 0; its other outputs are unspecified, and the caller
 * runs it through the host decoder, which stays the authority on accepting
 * it.  Nothing is written outside message i's own slots.
 * All pointers are device memory, 16-byte aligned; row_pitch % 64 == 0. */
#define RBC_HAS_WIRE_RX 1
#define RBC_WIRE_OK 0
#define RBC_WIRE_FALLBACK 1
int rbc_dev_unmarshal_val(rbc_ctx *ctx, void *stream, int count, const uint8_t *msgs, const uint64_t *offs,
                          const uint32_t *lens, const uint8_t *idx, uint8_t *rows, uint32_t row_pitch,
                          uint32_t *shard_lens_out, uint8_t *branches_out, uint8_t *roots_out, uint8_t *types_out,
                          int32_t *status_out);

/* Validate ECHOs straight from their wire bytes; the shards stay on the
 * device.  rbc_wire_rx owns a stream and the device buffers for up to
 * max_msgs messages in a ring of up to max_ring_bytes per call, with one row
 * slot of row_pitch bytes (row_pitch % 64 == 0, >= the largest shard) per
 * message. */
typedef struct rbc_wire_rx rbc_wire_rx;
int rbc_wire_rx_create(rbc_ctx *ctx, int max_msgs, size_t max_ring_bytes, uint32_t row_pitch, rbc_wire_rx **out);
void rbc_wire_rx_destroy(rbc_wire_rx *rx); /* waits for its outstanding work */
/* One host-to-device copy of ring[0, ring_bytes) (direct DMA from
 * rbc_host_alloc memory, staged from pageable memory), the unmarshal kernel
 * into keep_dev (row i at keep_dev + i*row_pitch, keep_bytes >=
 * count*row_pitch, device memory of the context's device), validateMessage of
 * every decoded message against the root and branch it carries itself, and
 * one device-to-host copy of the small outputs:
 *   verdict_out[i]   1 valid, 0 decoded but the proof fails, 2 fallback (not
 *                    canonical: no proof attempted, decode it on the host)
 *   types_out[i], roots_out[i][32], shard_lens_out[i] (uint32), leaves_out[i][32]
 *                    (the shard's SHA-256; nullable) -- defined for verdicts 0 and 1.
 * leaves_out and the kept rows feed rbc_interpolate_batch_kept unchanged.
 * Every argument is checked before any device work (offs[i] % 16 == 0,
 * offs[i] + round_up(lens[i], 16) <= ring_bytes, idx[i] < n, count <=
 * max_msgs, ring_bytes <= max_ring_bytes, keep_dev / keep_bytes as above):
 * RBC_ERR_INVALID_ARG enqueues nothing.  Asynchronous: the outputs and the
 * ring belong to the call until rbc_wire_wait(ticket) returns; a second
 * rbc_wire_validate on the same rx first completes the one before. */
int rbc_wire_validate(rbc_wire_rx *rx, int count, const uint8_t *ring, size_t ring_bytes, const uint64_t *offs,
                      const uint32_t *lens, const uint8_t *idx, uint8_t *verdict_out, uint8_t *types_out,
                      uint8_t *roots_out, uint32_t *shard_lens_out, uint8_t *leaves_out, uint8_t *keep_dev,
                      size_t keep_bytes, uint64_t *ticket);
int rbc_wire_wait(rbc_wire_rx *rx, uint64_t ticket);
int rbc_wire_poll(rbc_wire_rx *rx, uint64_t ticket, int *done);

/* ---- ECHOs from wire bytes to delivered values in one call ----------------
 * The mirror of rbc_shard_commit_val, present when RBC_HAS_WIRE_RECEIVE is
 * defined (the ABI version stays 7: detect the addition by symbol).
 *
 * rbc_dev_unmarshal_echo decodes `msgs` received ECHO / VAL messages of
 * `count` instances straight into the rbc_rx_batch layout, so its outputs feed
 * rbc_dev_verify, rbc_dev_interpolate or rbc_dev_receive_step unchanged and
 * every shard is written once, at its leaf position.  Message m is
 * ring[offs[m], offs[m] + lens[m]) with the rules of rbc_dev_unmarshal_val
 * (offs[m] % 16 == 0, no byte read outside round_up(lens[m], 16) from
 * offs[m]); it was sent by the member at leaf idx[m] for instance
 * inst[m] < count, which collects ECHOs for roots[inst[m]] and whose shards
 * have shard_lens[inst[m]] bytes (shard_lens NULL: uniform_shard_len).  Its
 * slot is r = inst[m]*n + idx[m] of shards [count][n][shard_pitch], branches
 * [count][n][max(depth,1)][32] (device form: a zero slot for an empty level-0
 * sibling) and present [count][n].  msg_status[m], decided in this order:
 *   1. the shape cannot be derived from lens[m] and idx[m] (rbc_dev_unmarshal_val's
 *      rule)                                          -> RBC_WIRE_FALLBACK
 *   2. the derived shard length is not the instance's -> RBC_WIRE_OTHER_LEN
 *   3. a byte is not canonical                        -> RBC_WIRE_FALLBACK
 *   4. the message's root (compared on the device, never stored) is not
 *      roots[inst[m]]                                 -> RBC_WIRE_OTHER_ROOT
 *   5. otherwise RBC_WIRE_OK: present[r] = 1, the row holds the shard with
 *      zeros from S to round_up(S, 64), the branch slot the device-form branch.
 * A message with status 1, 2 or 3 writes nothing of its slot: row, branch slot
 * and present[r] stay as they were.  types[m] (types nullable) is the
 * message's type for RBC_WIRE_OK.  A message writes nothing outside its own row
 * slot, branch slot, present[r], msg_status[m] and types[m]; two messages
 * naming one slot are the caller's error.  All pointers are device memory, 16-byte aligned;
 * shard_pitch % 64 == 0 and >= every shard_lens[i].  The caller zeroes present
 * before the call, and shards where its consumer needs whole-pitch zeros. */
#define RBC_HAS_WIRE_RECEIVE 1
#define RBC_WIRE_OTHER_ROOT 2
#define RBC_WIRE_OTHER_LEN 3
int rbc_dev_unmarshal_echo(rbc_ctx *ctx, void *stream, int count, int msgs, const uint8_t *ring,
                           const uint64_t *offs, const uint32_t *lens, const uint32_t *inst, const uint8_t *idx,
                           const uint8_t *roots, const uint32_t *shard_lens, uint32_t uniform_shard_len,
                           uint8_t *shards, uint32_t shard_pitch, uint8_t *branches, uint8_t *present,
                           int32_t *msg_status, uint8_t *types);

/* The receiver: a ring of received ECHO pb.Messages for `count` instances
 * goes in; each instance's value, digest and status come out, from one
 * submission.  rbc_wire_receiver owns one stream and the device buffers
 * (shards, branches, present, valid, leaves, values, digests, status,
 * metadata) for up to max_count instances and max_msgs messages in a ring of
 * up to max_ring_bytes per call, with rows of shard_pitch bytes
 * (shard_pitch % 64 == 0, >= the largest shard). */
typedef struct rbc_wire_receiver rbc_wire_receiver;
int rbc_wire_receiver_create(rbc_ctx *ctx, int max_count, int max_msgs, size_t max_ring_bytes, uint32_t shard_pitch,
                             rbc_wire_receiver **out);
void rbc_wire_receiver_destroy(rbc_wire_receiver *rcv); /* waits for its outstanding work */
/* On the receiver's own stream: one host-to-device copy of the metadata, one
 * of ring[0, ring_bytes) (direct DMA from rbc_host_alloc memory, staged from
 * pageable memory), rbc_dev_unmarshal_echo into zeroed rows, rbc_dev_verify
 * over the decoded rows, rbc_dev_interpolate(leaves_verified = 1) over the
 * proven ones, and the copies back:
 *   verdict_out[m]  1 decoded and proven; 0 decoded, but the proof fails or
 *                   the root is another one; 2 fallback (not canonical: decode
 *                   it on the host); 3 the shard has another length than its
 *                   instance
 *   types_out[m]    (nullable) the message's type, for verdicts 0 and 1
 *   valid_out       [count][n], rbc_dev_verify's valid[]
 *   values_out      [count][value_pitch]: k*shard_lens[i] bytes, then zeros
 *   digests_out     [count][32] (nullable) and status_out [count], as
 *                   rbc_interpolate_batch defines them, over the proven rows.
 * An instance with messages of verdict 2 or 3 is completed by the caller: run
 * those messages through the host decoder and the instance through
 * rbc_interpolate_batch.
 * Every argument is checked before any device work, and RBC_ERR_INVALID_ARG
 * enqueues nothing: null pointers; count > max_count, msgs > max_msgs,
 * ring_bytes > max_ring_bytes; offs[m] % 16 != 0 or offs[m] +
 * round_up(lens[m], 16) > ring_bytes; inst[m] >= count, idx[m] >= n; two
 * messages with the same (inst, idx); shard_lens[i] == 0 or > shard_pitch;
 * value_pitch < k * max shard_lens[i].
 * Asynchronous: the outputs and the ring belong to the call until
 * rbc_wire_receive_wait(ticket) returns.  One submission is in flight at a
 * time: a second rbc_wire_receive on the same receiver first completes the
 * one before.  The call uses the context's decode workspace like any
 * rbc_dev_* caller: while a submission is in flight the context must not run
 * rbc_dev_verify, rbc_dev_interpolate or rbc_dev_receive_step work on another
 * stream. */
int rbc_wire_receive(rbc_wire_receiver *rcv, int count, int msgs, const uint8_t *ring, size_t ring_bytes,
                     const uint64_t *offs, const uint32_t *lens, const uint32_t *inst, const uint8_t *idx,
                     const uint8_t *roots, const size_t *shard_lens, uint8_t *verdict_out, uint8_t *types_out,
                     uint8_t *valid_out, uint8_t *values_out, size_t value_pitch, uint8_t *digests_out,
                     int32_t *status_out, uint64_t *ticket);
int rbc_wire_receive_wait(rbc_wire_receiver *rcv, uint64_t ticket);
int rbc_wire_receive_poll(rbc_wire_receiver *rcv, uint64_t ticket, int *done);

/* ---- binary VAL / ECHO payload codec (opt-in) -----------------------------
 * Present when RBC_HAS_WIRE_BINARY is defined (the ABI version stays 7: detect
 * the addition by symbol).  The reference pins only the pb.Message wrapper;
 * pb.RBC.payload is opaque bytes, so a deployment whose nodes all run this
 * library may carry the shard raw instead of as base64 inside JSON: 3/4 of
 * the bytes on the network and across PCIe.  The wrapper is unchanged,
 *   0x1a varint(R) 0x0a varint(J) <payload, J bytes> [0x10 type]
 * with R = 1 + varint_len(J) + J + (type ? 2 : 0), and the payload of VAL /
 * ECHO is (version 1):
 *   offset      size   field
 *   0           1      0xB1 magic (no JSON text begins with it, so each
 *                      decoder rejects the other's payload)
 *   1           1      0x01 version
 *   2           1      L: number of 32-byte branch entries, Go flat form
 *   3           1      0x00 reserved, must be zero
 *   4           4      S: shard length, little-endian u32
 *   8           32     root
 *   40          32*L   branch
 *   40 + 32*L   S      shard
 * J = 40 + 32*L + S, nothing behind the shard.  READY keeps its JSON payload.
 * Every (root, branch, shard, type) has exactly one encoding; a message's
 * length alone does not fix its type ((S, VAL) and (S - 2, ECHO) mostly share
 * a total), and some totals cannot occur (a varint grows there).
 *
 * rbc_bin_encode_val: root_len must be 32 and branch_len a multiple of 32
 * (at most 255 entries), else 0 is returned; block_len 0 is allowed (S = 0,
 * as "Block":null).  Returns the size; writes only when it fits.
 * rbc_bin_decode_val: RBC_ERR_PROTOCOL unless len >= 40, magic, version and
 * reserved byte are right and len == 40 + 32*L + S exactly;
 * RBC_ERR_INVALID_ARG (lens set) when a buffer is short.
 * rbc_payload_decode_val dispatches on the first payload byte: 0xB1 to the
 * binary decoder, anything else to rbc_json_decode_val -- the one call a
 * shim's fallback path needs. */
#define RBC_HAS_WIRE_BINARY 1
#define RBC_WIRE_CODEC_JSON 0
#define RBC_WIRE_CODEC_BINARY 1
#define RBC_BIN_MAGIC 0xB1
#define RBC_BIN_VERSION 0x01
size_t rbc_bin_encode_val(const uint8_t *root, size_t root_len, const uint8_t *branch, size_t branch_len,
                          const uint8_t *block, size_t block_len, uint8_t *out, size_t cap);
int rbc_bin_decode_val(const uint8_t *payload, size_t len, uint8_t *root_out, uint8_t *branch_out, size_t branch_cap,
                       size_t *branch_len, uint8_t *block_out, size_t block_cap, size_t *block_len);
int rbc_payload_decode_val(const uint8_t *payload, size_t len, uint8_t *root_out, uint8_t *branch_out,
                           size_t branch_cap, size_t *branch_len, uint8_t *block_out, size_t block_cap,
                           size_t *block_len);
/* rbc_val_message_size for a codec (codec 0 equals it); 0 for an unknown codec. */
size_t rbc_val_message_size_codec(int codec, int n, uint32_t shard_len, uint32_t index, int type);
/* The codec of a context's wire entry points, RBC_WIRE_CODEC_JSON by default.
 * rbc_dev_marshal_val, rbc_dev_unmarshal_val, rbc_dev_unmarshal_echo,
 * rbc_shard_commit_val, rbc_wire_validate and rbc_wire_receive read it when
 * they submit; their signatures and their JSON behaviour are unchanged.  In
 * binary mode "canonical" means: rbc_pb_decode_rbc + rbc_bin_decode_val accept
 * the message, the wrapper is minimal (minimal varints, exactly these fields
 * in this order), L is the flat branch length of leaf idx in an n-leaf tree
 * and 1 <= S <= the row pitch; a JSON message is RBC_WIRE_FALLBACK there, and
 * a binary one is in JSON mode.  A binary message's length leaves up to two
 * shapes, one per type ((S, VAL) and (S - 2, ECHO)): rbc_dev_unmarshal_val
 * keeps the one whose header the message carries; rbc_dev_unmarshal_echo takes
 * the one of the instance's shard length (none: RBC_WIRE_OTHER_LEN) and checks
 * the message against that one alone.  Every node of a deployment emits one codec.
 * Changing the codec while a wire submission of the context is in flight is
 * the caller's error. */
int rbc_ctx_set_wire_codec(rbc_ctx *ctx, int codec);
int rbc_ctx_wire_codec(const rbc_ctx *ctx, int *codec);

/* ---- READY from wire bytes, and the quorums of a batch of instances -------
 * Present when RBC_HAS_WIRE_READY is defined (the ABI version stays 7: detect
 * the addition by symbol).  READYs go in as wire bytes; per-instance counts
 * and the protocol's decisions come out.
 *
 * rbc_dev_unmarshal_ready decodes `msgs` received READY messages of `count`
 * instances into a sender bitmap.  Message m is ring[offs[m], offs[m] +
 * lens[m]) with the rules of rbc_dev_unmarshal_echo (offs[m] % 16 == 0, no
 * byte read outside round_up(lens[m], 16) from offs[m]); it was sent by the
 * member at leaf idx[m] for instance inst[m], which collects READYs for
 * roots[inst[m]].  A READY is decoded only when it is canonical: byte-for-byte
 * what rbc_pb_encode_rbc(RBC_MSG_READY, rbc_json_encode_ready(root, 32)) emits
 * -- one form of one length under both payload codecs (the size those two
 * calls return), so rbc_ctx_set_wire_codec does not affect it.  A root of 31 or 33
 * bytes encodes to as many characters: canonical requires '=' at the last
 * base64 character and not at the one before it.  The non-zero trailing bits
 * of the last quantum are ignored, as the host decoder ignores them.
 * msg_status[m], decided in this order:
 *   1. lens[m] is not that length, inst[m] >= count or idx[m] >= n (before any
 *      byte of the message is read)                   -> RBC_WIRE_FALLBACK
 *   2. a byte is not canonical                        -> RBC_WIRE_FALLBACK
 *   3. the message's root (compared on the device, never stored) is not
 *      roots[inst[m]]                                 -> RBC_WIRE_OTHER_ROOT
 *   4. otherwise RBC_WIRE_OK, and ready[inst[m]*n + idx[m]] = 1.
 * ready [count][n] is the caller's: the call only ever sets bytes in it, so it
 * accumulates over calls as READYs arrive, and two messages naming one slot
 * are harmless (both store the same 1).  A message writes nothing but
 * msg_status[m] and that one byte.  A RBC_WIRE_FALLBACK message goes through
 * the host decoder (rbc_pb_decode_rbc + rbc_json_decode_ready), which stays
 * the authority on accepting it.  All pointers are device memory; ring and
 * roots are 16-byte aligned.
 *
 * One limit: rbc_node counts each sender's FIRST READY, whatever its root, and
 * rejects the sender's later ones.  This path counts every READY for
 * roots[inst]: a sender whose first READY named another root and whose second
 * names this one is counted here and not there.  A caller that wants the
 * strict rule passes each sender's first READY only.  Nothing differs for
 * honest senders, who send one. */
#define RBC_HAS_WIRE_READY 1
int rbc_dev_unmarshal_ready(rbc_ctx *ctx, void *stream, int count, int msgs, const uint8_t *ring,
                            const uint64_t *offs, const uint32_t *lens, const uint32_t *inst, const uint8_t *idx,
                            const uint8_t *roots, uint8_t *ready, int32_t *msg_status);

/* The thresholds of one node (index `self`, or -1) over a batch of instances,
 * with (n, f) the context's geometry.  Per instance i: E = the non-zero bytes
 * of valid[i][0..n) (rbc_dev_verify's / rbc_wire_receive's valid; NULL: E = 0),
 * R = the non-zero bytes of ready[i][0..n), st = status[i] (what
 * rbc_dev_interpolate / rbc_wire_receive reported; NULL: nothing is known about
 * the interpolation, and `have` is false).  rbc_node's rules over counts:
 *   have       = st == RBC_OK && (E >= n-f || (R >= 2f+1 && E >= n-2f))
 *   send_ready = R >= f+1 || have
 *   if send_ready && self >= 0 && !ready[i][self]:  ready[i][self] = 1, R += 1
 *                                       (the node's own READY counts)
 *   deliver    = st == RBC_OK && R >= 2f+1 && E >= n-2f
 * echo_counts[i] = E, ready_counts[i] = R after the own bit (uint32), and
 * flags[i] holds RBC_QUORUM_ECHO (E >= n-f), RBC_QUORUM_AMPLIFY (R >= f+1
 * before the own bit), RBC_QUORUM_SEND_READY and RBC_QUORUM_DELIVER.  The call
 * writes ready[i][self] and nothing else of ready.  All pointers are device
 * memory; self in [-1, n). */
#define RBC_QUORUM_ECHO 1
#define RBC_QUORUM_AMPLIFY 2
#define RBC_QUORUM_SEND_READY 4
#define RBC_QUORUM_DELIVER 8
int rbc_dev_quorum(rbc_ctx *ctx, void *stream, int count, const uint8_t *valid, uint8_t *ready,
                   const int32_t *status, int self, uint32_t *echo_counts, uint32_t *ready_counts, uint8_t *flags);

/* Both steps from host memory in one submission.  rbc_wire_quorum_handle owns
 * one stream and the device buffers for up to max_count instances and max_msgs
 * messages in a ring of up to max_ring_bytes per call. */
typedef struct rbc_wire_quorum_handle rbc_wire_quorum_handle;
int rbc_wire_quorum_create(rbc_ctx *ctx, int max_count, int max_msgs, size_t max_ring_bytes,
                           rbc_wire_quorum_handle **out);
void rbc_wire_quorum_destroy(rbc_wire_quorum_handle *q); /* waits for its outstanding work */
/* On the handle's own stream: one host-to-device copy of the metadata (with
 * valid, status and the caller's bitmap), one of ring[0, ring_bytes) (direct
 * DMA from rbc_host_alloc memory, staged from pageable memory),
 * rbc_dev_unmarshal_ready, rbc_dev_quorum and one copy back:
 *   ready_inout      [count][n]: the bitmap so far goes in; it comes back with
 *                    the decoded READYs and the own bit OR-ed in
 *   verdict_out[m]   (uint8) the RBC_WIRE_* status of message m
 *   echo_counts_out, ready_counts_out [count] (uint32), flags_out [count]
 * valid [count][n] and status [count] are host memory and nullable, as in
 * rbc_dev_quorum.  The call keeps no state between submissions: the bitmap
 * lives with the caller.  msgs == 0 is allowed (ring, offs, lens, inst, idx,
 * roots and verdict_out may then be NULL): it only re-tallies, for example after new
 * ECHO results.  count == 0 with msgs == 0 returns ticket 0.
 * Every argument is checked before any device work, and RBC_ERR_INVALID_ARG
 * enqueues nothing: the checks of rbc_wire_receive -- null pointers; count >
 * max_count, msgs > max_msgs, ring_bytes > max_ring_bytes; offs[m] % 16 != 0
 * or offs[m] + round_up(lens[m], 16) > ring_bytes; inst[m] >= count,
 * idx[m] >= n -- except that two messages with the same (inst, idx) are
 * allowed, and self outside [-1, n).
 * Asynchronous: the outputs, ready_inout and the ring belong to the call until
 * rbc_wire_quorum_wait(ticket) returns.  One submission is in flight at a
 * time: a second rbc_wire_quorum on the same handle first completes the one
 * before. */
int rbc_wire_quorum(rbc_wire_quorum_handle *q, int count, int msgs, const uint8_t *ring, size_t ring_bytes,
                    const uint64_t *offs, const uint32_t *lens, const uint32_t *inst, const uint8_t *idx,
                    const uint8_t *roots, const uint8_t *valid, const int32_t *status, int self,
                    uint8_t *ready_inout, uint8_t *verdict_out, uint32_t *echo_counts_out,
                    uint32_t *ready_counts_out, uint8_t *flags_out, uint64_t *ticket);
int rbc_wire_quorum_wait(rbc_wire_quorum_handle *q, uint64_t ticket);
int rbc_wire_quorum_poll(rbc_wire_quorum_handle *q, uint64_t ticket, int *done);

/* ---- RBC instance (one proposer's broadcast, seen at one node) ----------- */
typedef struct rbc_node rbc_node;
/* NewRBC (rbc/rbc.go:38). */
int rbc_node_create(rbc_batcher *batcher, int n, int f, int self, int proposer, rbc_node **out);
void rbc_node_destroy(rbc_node *node); /* waits for its outstanding GPU work */
/* The payload codec of the VAL / ECHO this node emits (RBC_HAS_WIRE_BINARY),
 * RBC_WIRE_CODEC_JSON by default; call it before the first message.  A JSON
 * node behaves as ever (a binary VAL / ECHO is malformed to it); a binary node
 * emits binary VAL / ECHO and accepts either form (rbc_payload_decode_val's
 * rule), so a rolling upgrade works.  READY is JSON in both. */
int rbc_node_set_wire_codec(rbc_node *node, int codec);
/* Proposer only: shard + commit `value` (copied), then VAL(h, b_j, s_j) to every j.
 * The broadcast payload is framed as [u64 little-endian len][value] (len 0 is
 * allowed), so rbc_node_value returns exactly these bytes. */
int rbc_node_propose(rbc_node *node, const uint8_t *value, size_t len);
/* HandleMessage (rbc/rbc.go:47): a marshaled pb.Message from node `sender`.
 * Parses and submits its GPU check; the outcome applies in rbc_node_progress.
 * Returns RBC_ERR_PROTOCOL for a malformed, duplicate or out-of-protocol
 * message (it is dropped and counted). */
int rbc_node_handle_message(rbc_node *node, int sender, const uint8_t *msg, size_t len);
/* Completes submitted GPU work in order and advances the state machine:
 * wait = 0 applies only what is done, wait = 1 blocks until all is done.
 * *pending_out (nullable) = submissions still outstanding. */
int rbc_node_progress(rbc_node *node, int wait, int *pending_out);
/* Messages (rbc/rbc.go:74): pops the next outgoing message into buf;
 * *to = recipient index, or -1 for every node but this one (a node applies
 * its own ECHO/READY locally).  *len = 0: queue empty.  cap too small:
 * returns RBC_ERR_INVALID_ARG with *len = the size needed (message kept). */
int rbc_node_next_message(rbc_node *node, int *to, uint8_t *buf, size_t cap, size_t *len);
/* Value (rbc/rbc.go:69): *delivered = 1 once decided; the value is the
 * proposer's bytes, unframed from the interpolated k*S bytes.  A delivered
 * payload whose frame length exceeds it (a Byzantine proposer: every honest
 * node sees the same bytes) returns RBC_ERR_PROTOCOL with *delivered = 1 and
 * *len = 0.  buf NULL with cap 0: only *len and *delivered are set.
 * rbc_node_create requires n >= 3f + 1 (HBBFT quorum intersection). */
int rbc_node_value(rbc_node *node, uint8_t *buf, size_t cap, size_t *len, int *delivered);
/* Valid ECHOs and READYs for the leading root, READY sent (0/1), messages
 * rejected (bad proof, wrong sender, malformed, duplicate). */
int rbc_node_stats(rbc_node *node, int *echoes, int *readies, int *ready_sent, int *rejected);

#ifdef __cplusplus
}
#endif
#endif
