// wire_rx.cpp -- the receive half of the wire path (include/rbc_protocol.h):
// rbc_dev_unmarshal_val and rbc_wire_validate, which takes ECHOs as the raw
// pb.Message bytes a pass-through gRPC codec hands over, decodes them on the
// device (unmarshal_val_kernel, wire.hip) and proves each shard against the
// root and branch its own message carries, leaving the shards on the device
// for rbc_interpolate_batch_kept.
//
// A translation unit of its own on the public ABI plus kernels.h, like the
// batcher: the host runtime (capi.cpp) does not know it.  The session behind
// the handle (stream, event, staging blocks, tickets) is wire_session.h's,
// shared with wire_receive.cpp and wire_ready.cpp.
#include <string.h>

#include "../../include/rbc_protocol.h"
#include "kernels.h"
#include "wire_session.h"

using namespace wire;

namespace {

// where the small outputs of `count` messages sit in the one block that
// crosses back to the host
struct SmallOut {
    size_t valid, types, status, slens, roots, leaves, bytes;
    explicit SmallOut(size_t count) {
        Carver c;
        valid = c.take(count);
        types = c.take(count);
        status = c.take(count * 4);
        slens = c.take(count * 4);
        roots = c.take(count * 32);
        leaves = c.take(count * 32);
        bytes = c.o;
    }
};

// host-to-device metadata of `count` messages, one block
struct MetaIn {
    size_t offs, lens, idx, bytes;
    explicit MetaIn(size_t count) {
        Carver c;
        offs = c.take(count * 8);
        lens = c.take(count * 4);
        idx = c.take(count);
        bytes = c.o;
    }
};

}  // namespace

struct rbc_wire_rx : WireSession {
    rbc_ctx *ctx = nullptr;
    int n = 0, depth = 0, max_msgs = 0;
    size_t max_ring = 0, bslot = 32;
    uint32_t row_pitch = 0;
    uint8_t *d_ring = nullptr, *d_meta = nullptr, *d_small = nullptr, *d_branches = nullptr;
    uint8_t *h_meta = nullptr, *h_small = nullptr;  // pinned
    // the one submission in flight
    struct {
        int count = 0;
        uint8_t *verdict = nullptr, *types = nullptr, *roots = nullptr, *leaves = nullptr;
        uint32_t *slens = nullptr;
    } cur;

    void copy_out() override {
        const int count = cur.count;
        const SmallOut so((size_t)count);
        const int32_t *status = reinterpret_cast<const int32_t *>(h_small + so.status);
        for (int i = 0; i < count; ++i) cur.verdict[i] = status[i] != WIRE_OK ? 2 : (h_small[so.valid + i] ? 1 : 0);
        if (cur.types) memcpy(cur.types, h_small + so.types, (size_t)count);
        if (cur.slens) memcpy(cur.slens, h_small + so.slens, (size_t)count * 4);
        if (cur.roots) memcpy(cur.roots, h_small + so.roots, (size_t)count * 32);
        if (cur.leaves) memcpy(cur.leaves, h_small + so.leaves, (size_t)count * 32);
    }
};

extern "C" {

int rbc_dev_unmarshal_val(rbc_ctx *ctx, void *stream, int count, const uint8_t *msgs, const uint64_t *offs,
                          const uint32_t *lens, const uint8_t *idx, uint8_t *rows, uint32_t row_pitch,
                          uint32_t *shard_lens_out, uint8_t *branches_out, uint8_t *roots_out, uint8_t *types_out,
                          int32_t *status_out) {
    if (!ctx || count < 0 || row_pitch == 0 || row_pitch % 64) return RBC_ERR_INVALID_ARG;
    if (!msgs || !offs || !lens || !idx || !rows || !shard_lens_out || !branches_out || !roots_out || !types_out ||
        !status_out)
        return RBC_ERR_INVALID_ARG;
    if (!aligned16(msgs) || !aligned16(rows) || !aligned16(branches_out) || !aligned16(roots_out))
        return RBC_ERR_INVALID_ARG;
    if (count == 0) return RBC_OK;
    int k = 0, p = 0, depth = 0, device = 0;
    if (!wire_geometry(ctx, &k, &p, &depth, &device)) return RBC_ERR_INVALID_ARG;
    WIRE_HIP(hipSetDevice(device));
    WireRxArgs a{};
    a.count = count;
    a.n = k + p;
    a.depth = depth;
    a.msgs = msgs;
    a.offs = offs;
    a.lens = lens;
    a.idx = idx;
    a.rows = rows;
    a.row_pitch = row_pitch;
    a.shard_lens = shard_lens_out;
    a.branches = branches_out;
    a.roots = roots_out;
    a.types = types_out;
    a.status = status_out;
    if (rbc_ctx_wire_codec(ctx, &a.codec) != RBC_OK) return RBC_ERR_INVALID_ARG;
    WIRE_HIP(rbc_launch_unmarshal_val(a, reinterpret_cast<hipStream_t>(stream)));
    return RBC_OK;
}

int rbc_wire_rx_create(rbc_ctx *ctx, int max_msgs, size_t max_ring_bytes, uint32_t row_pitch, rbc_wire_rx **out) {
    if (!out) return RBC_ERR_INVALID_ARG;
    *out = nullptr;
    if (!ctx || max_msgs <= 0 || max_ring_bytes == 0 || row_pitch == 0 || row_pitch % 64) return RBC_ERR_INVALID_ARG;
    int k = 0, p = 0, depth = 0, device = 0;
    if (!wire_geometry(ctx, &k, &p, &depth, &device)) return RBC_ERR_INVALID_ARG;
    rbc_wire_rx *rx = new rbc_wire_rx();
    rx->ctx = ctx;
    rx->n = k + p;
    rx->depth = depth;
    rx->max_msgs = max_msgs;
    rx->max_ring = max_ring_bytes;
    rx->row_pitch = row_pitch;
    rx->bslot = (size_t)(depth > 1 ? depth : 1) * 32;
    const size_t m = (size_t)max_msgs;
    const size_t meta = MetaIn(m).bytes, small = SmallOut(m).bytes;
    const bool ok = rx->open(device) && rx->dev(&rx->d_ring, round_up(max_ring_bytes, 16)) &&
                    rx->dev(&rx->d_meta, meta) && rx->dev(&rx->d_small, small) &&
                    rx->dev(&rx->d_branches, m * rx->bslot) && rx->pin(&rx->h_meta, meta) &&
                    rx->pin(&rx->h_small, small);
    return session_created(rx, ok, out);
}

void rbc_wire_rx_destroy(rbc_wire_rx *rx) { session_destroy(rx); }

int rbc_wire_validate(rbc_wire_rx *rx, int count, const uint8_t *ring, size_t ring_bytes, const uint64_t *offs,
                      const uint32_t *lens, const uint8_t *idx, uint8_t *verdict_out, uint8_t *types_out,
                      uint8_t *roots_out, uint32_t *shard_lens_out, uint8_t *leaves_out, uint8_t *keep_dev,
                      size_t keep_bytes, uint64_t *ticket) {
    if (!rx || count < 0 || !ticket) return RBC_ERR_INVALID_ARG;
    if (count == 0) {
        *ticket = 0;
        return RBC_OK;
    }
    if (!ring || !ring_bytes || !offs || !lens || !idx || !verdict_out || !types_out || !roots_out ||
        !shard_lens_out || !keep_dev)
        return RBC_ERR_INVALID_ARG;
    if (count > rx->max_msgs || ring_bytes > rx->max_ring) return RBC_ERR_INVALID_ARG;
    if (keep_bytes / rx->row_pitch < (size_t)count || !aligned16(keep_dev)) return RBC_ERR_INVALID_ARG;
    // every message's 16-byte chunks inside the ring (no wrap-around), its leaf inside the tree
    for (int i = 0; i < count; ++i) {
        if (!ring_slot_ok(offs[i], lens[i], ring_bytes, idx[i], (size_t)rx->n)) return RBC_ERR_INVALID_ARG;
    }
    // both ends of the kept rows: device memory of the context's device
    if (!device_memory(keep_dev, rx->device) ||
        !device_memory(keep_dev + (size_t)count * rx->row_pitch - 1, rx->device))
        return RBC_ERR_INVALID_ARG;
    int codec = 0;  // the context's payload codec, read at submission
    if (rbc_ctx_wire_codec(rx->ctx, &codec) != RBC_OK) return RBC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(rx->mu);
    if (rx->begin() != RBC_OK) return RBC_ERR_DEVICE;  // the one in flight keeps its status with its ticket
    hipStream_t st = rx->stream;
    const MetaIn mi((size_t)count);
    const SmallOut so((size_t)count);
    memcpy(rx->h_meta + mi.offs, offs, (size_t)count * 8);
    memcpy(rx->h_meta + mi.lens, lens, (size_t)count * 4);
    memcpy(rx->h_meta + mi.idx, idx, (size_t)count);
    WIRE_HIP(hipMemcpyAsync(rx->d_meta, rx->h_meta, mi.bytes, hipMemcpyHostToDevice, st));
    WIRE_HIP(hipMemcpyAsync(rx->d_ring, ring, ring_bytes, hipMemcpyHostToDevice, st));
    WireRxArgs u{};
    u.count = count;
    u.n = rx->n;
    u.depth = rx->depth;
    u.msgs = rx->d_ring;
    u.offs = reinterpret_cast<const uint64_t *>(rx->d_meta + mi.offs);
    u.lens = reinterpret_cast<const uint32_t *>(rx->d_meta + mi.lens);
    u.idx = rx->d_meta + mi.idx;
    u.rows = keep_dev;
    u.row_pitch = rx->row_pitch;
    u.shard_lens = reinterpret_cast<uint32_t *>(rx->d_small + so.slens);
    u.branches = rx->d_branches;
    u.roots = rx->d_small + so.roots;
    u.types = rx->d_small + so.types;
    u.status = reinterpret_cast<int32_t *>(rx->d_small + so.status);
    u.codec = codec;
    WIRE_HIP(rbc_launch_unmarshal_val(u, st));
    // validateMessage per decoded message (fallback messages are skipped by their status)
    ShaArgs a = sha_message_args(count, rx->n, rx->depth, keep_dev, rx->row_pitch, u.shard_lens, u.idx,
                                 rx->d_branches, rx->bslot, u.roots, rx->d_small + so.valid, rx->d_small + so.leaves);
    a.row_pitch = rx->row_pitch;
    a.status = u.status;
    WIRE_HIP(rbc_launch_sha_rows(a, true, st));
    WIRE_HIP(hipMemcpyAsync(rx->h_small, rx->d_small, so.bytes, hipMemcpyDeviceToHost, st));
    WIRE_HIP(hipEventRecord(rx->done, st));
    rx->cur.count = count;
    rx->cur.verdict = verdict_out;
    rx->cur.types = types_out;
    rx->cur.roots = roots_out;
    rx->cur.slens = shard_lens_out;
    rx->cur.leaves = leaves_out;
    *ticket = rx->issue();
    return RBC_OK;
}

int rbc_wire_wait(rbc_wire_rx *rx, uint64_t ticket) { return session_wait(rx, ticket); }

int rbc_wire_poll(rbc_wire_rx *rx, uint64_t ticket, int *done) { return session_poll(rx, ticket, done); }

}  // extern "C"
