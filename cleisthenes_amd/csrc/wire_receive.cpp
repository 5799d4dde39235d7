// wire_receive.cpp -- ECHOs from wire bytes to delivered values in one call
// (include/rbc_protocol.h, RBC_HAS_WIRE_RECEIVE): rbc_dev_unmarshal_echo and
// rbc_wire_receive, the mirror of rbc_shard_commit_val.  A ring of received
// pb.Message bytes for `count` instances is decoded on the device straight
// into the [count][n][pitch] layout (unmarshal_echo_kernel, wire.hip), proven
// (rbc_dev_verify) and decoded (rbc_dev_interpolate): one submission, one copy
// of the ring, every shard written once.
//
// A translation unit of its own on the public ABI plus kernels.h, like
// wire_rx.cpp, with which it shares the session behind the handle (stream,
// event, staging blocks, tickets: wire_session.h): the host runtime (capi.cpp)
// does not know it.
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/rbc_protocol.h"
#include "kernels.h"
#include "wire_session.h"

using namespace wire;

namespace {

// host-to-device metadata of one call
struct MetaIn {
    size_t offs, lens, inst, idx, roots, slens, bytes;
    MetaIn(size_t count, size_t msgs) {
        Carver c;
        offs = c.take(msgs * 8);
        lens = c.take(msgs * 4);
        inst = c.take(msgs * 4);
        idx = c.take(msgs);
        roots = c.take(count * 32);
        slens = c.take(count * 4);
        bytes = c.o;
    }
};

// the small outputs that cross back in one copy
struct SmallOut {
    size_t mstatus, types, valid, digests, status, bytes;
    SmallOut(size_t count, size_t msgs, size_t n) {
        Carver c;
        mstatus = c.take(msgs * 4);
        types = c.take(msgs);
        valid = c.take(count * n);
        digests = c.take(count * 32);
        status = c.take(count * 4);
        bytes = c.o;
    }
};

}  // namespace

struct rbc_wire_receiver : WireSession {
    rbc_ctx *ctx = nullptr;
    int n = 0, k = 0, depth = 0, max_count = 0, max_msgs = 0;
    size_t max_ring = 0, bslot = 32;
    uint32_t pitch = 0;
    uint8_t *d_ring = nullptr, *d_meta = nullptr, *d_small = nullptr, *d_shards = nullptr, *d_branches = nullptr,
            *d_present = nullptr, *d_leaves = nullptr, *d_values = nullptr;
    uint8_t *h_meta = nullptr, *h_small = nullptr, *h_values = nullptr;  // pinned
    std::vector<uint8_t> seen;  // [max_count][n]: the (inst, idx) pairs of the call being checked
    // the one submission in flight
    struct {
        int count = 0, msgs = 0;
        const uint32_t *inst = nullptr;  // pinned copies (h_meta)
        const uint8_t *idx = nullptr;
        const uint32_t *slens = nullptr;
        size_t vpitch = 0, value_pitch = 0;
        bool values_direct = false;
        uint8_t *verdict = nullptr, *types = nullptr, *valid = nullptr, *values = nullptr, *digests = nullptr;
        int32_t *status = nullptr;
    } cur;

    void copy_out() override {
        const size_t count = (size_t)cur.count, msgs = (size_t)cur.msgs;
        const SmallOut so(count, msgs, (size_t)n);
        const int32_t *ms = reinterpret_cast<const int32_t *>(h_small + so.mstatus);
        const uint8_t *valid = h_small + so.valid;
        for (size_t m = 0; m < msgs; ++m) {
            uint8_t v;
            switch (ms[m]) {
            case WIRE_OK: v = valid[(size_t)cur.inst[m] * n + cur.idx[m]] ? 1 : 0; break;
            case WIRE_OTHER_ROOT: v = 0; break;
            case WIRE_OTHER_LEN: v = 3; break;
            default: v = 2; break;
            }
            cur.verdict[m] = v;
        }
        if (cur.types && msgs) memcpy(cur.types, h_small + so.types, msgs);
        memcpy(cur.valid, valid, count * n);
        if (cur.digests) memcpy(cur.digests, h_small + so.digests, count * 32);
        memcpy(cur.status, h_small + so.status, count * 4);
        for (size_t i = 0; i < count; ++i) {  // k*S_i bytes, then zeros up to value_pitch
            uint8_t *row = cur.values + i * cur.value_pitch;
            const size_t used = (size_t)k * cur.slens[i];
            if (!cur.values_direct) memcpy(row, h_values + i * cur.vpitch, used);
            memset(row + used, 0, cur.value_pitch - used);
        }
    }
};

extern "C" {

int rbc_dev_unmarshal_echo(rbc_ctx *ctx, void *stream, int count, int msgs, const uint8_t *ring,
                           const uint64_t *offs, const uint32_t *lens, const uint32_t *inst, const uint8_t *idx,
                           const uint8_t *roots, const uint32_t *shard_lens, uint32_t uniform_shard_len,
                           uint8_t *shards, uint32_t shard_pitch, uint8_t *branches, uint8_t *present,
                           int32_t *msg_status, uint8_t *types) {
    if (!ctx || count < 0 || msgs < 0 || shard_pitch == 0 || shard_pitch % 64) return RBC_ERR_INVALID_ARG;
    if (!ring || !offs || !lens || !inst || !idx || !roots || !shards || !branches || !present || !msg_status)
        return RBC_ERR_INVALID_ARG;
    if (!shard_lens && (uniform_shard_len == 0 || uniform_shard_len > shard_pitch)) return RBC_ERR_INVALID_ARG;
    if (!aligned16(ring) || !aligned16(roots) || !aligned16(shards) || !aligned16(branches))
        return RBC_ERR_INVALID_ARG;
    if (msgs == 0) return RBC_OK;
    if (count == 0) return RBC_ERR_INVALID_ARG;  // messages of no instance
    int k = 0, p = 0, depth = 0, device = 0;
    if (!wire_geometry(ctx, &k, &p, &depth, &device)) return RBC_ERR_INVALID_ARG;
    WIRE_HIP(hipSetDevice(device));
    WireEchoArgs a{};
    a.count = count;
    a.msgs = msgs;
    a.n = k + p;
    a.depth = depth;
    a.ring = ring;
    a.offs = offs;
    a.lens = lens;
    a.inst = inst;
    a.idx = idx;
    a.roots = roots;
    a.shard_lens = shard_lens;
    a.uniform_len = uniform_shard_len;
    a.shards = shards;
    a.shard_pitch = shard_pitch;
    a.branches = branches;
    a.present = present;
    a.msg_status = msg_status;
    a.types = types;
    if (rbc_ctx_wire_codec(ctx, &a.codec) != RBC_OK) return RBC_ERR_INVALID_ARG;
    WIRE_HIP(rbc_launch_unmarshal_echo(a, reinterpret_cast<hipStream_t>(stream)));
    return RBC_OK;
}

int rbc_wire_receiver_create(rbc_ctx *ctx, int max_count, int max_msgs, size_t max_ring_bytes, uint32_t shard_pitch,
                             rbc_wire_receiver **out) {
    if (!out) return RBC_ERR_INVALID_ARG;
    *out = nullptr;
    if (!ctx || max_count <= 0 || max_msgs <= 0 || max_ring_bytes == 0 || shard_pitch == 0 || shard_pitch % 64)
        return RBC_ERR_INVALID_ARG;
    int k = 0, p = 0, depth = 0, device = 0;
    if (!wire_geometry(ctx, &k, &p, &depth, &device)) return RBC_ERR_INVALID_ARG;
    const size_t n = (size_t)(k + p), c = (size_t)max_count;
    // rbc_dev_interpolate's bounds on one instance and one value row
    if (n * shard_pitch > 0x7fffffffULL || (size_t)k * shard_pitch > 0x7fffffffULL) return RBC_ERR_INVALID_ARG;
    rbc_wire_receiver *r = new rbc_wire_receiver();
    r->ctx = ctx;
    r->n = (int)n;
    r->k = k;
    r->depth = depth;
    r->max_count = max_count;
    r->max_msgs = max_msgs;
    r->max_ring = max_ring_bytes;
    r->pitch = shard_pitch;
    r->bslot = (size_t)(depth > 1 ? depth : 1) * 32;
    r->seen.assign(c * n, 0);
    const size_t meta = MetaIn(c, (size_t)max_msgs).bytes, small = SmallOut(c, (size_t)max_msgs, n).bytes;
    const size_t values = c * k * shard_pitch;
    const bool ok = r->open(device) && r->dev(&r->d_ring, round_up(max_ring_bytes, 16)) && r->dev(&r->d_meta, meta) &&
                    r->dev(&r->d_small, small) && r->dev(&r->d_shards, c * n * shard_pitch) &&
                    r->dev(&r->d_branches, c * n * r->bslot) && r->dev(&r->d_present, c * n) &&
                    r->dev(&r->d_leaves, c * n * 32) && r->dev(&r->d_values, values) && r->pin(&r->h_meta, meta) &&
                    r->pin(&r->h_small, small) && r->pin(&r->h_values, values);
    return session_created(r, ok, out);
}

void rbc_wire_receiver_destroy(rbc_wire_receiver *r) { session_destroy(r); }

int rbc_wire_receive(rbc_wire_receiver *r, int count, int msgs, const uint8_t *ring, size_t ring_bytes,
                     const uint64_t *offs, const uint32_t *lens, const uint32_t *inst, const uint8_t *idx,
                     const uint8_t *roots, const size_t *shard_lens, uint8_t *verdict_out, uint8_t *types_out,
                     uint8_t *valid_out, uint8_t *values_out, size_t value_pitch, uint8_t *digests_out,
                     int32_t *status_out, uint64_t *ticket) {
    if (!r || count < 0 || msgs < 0 || !ticket) return RBC_ERR_INVALID_ARG;
    if (count == 0) {
        if (msgs) return RBC_ERR_INVALID_ARG;  // messages of no instance
        *ticket = 0;
        return RBC_OK;
    }
    if (!roots || !shard_lens || !valid_out || !values_out || !status_out) return RBC_ERR_INVALID_ARG;
    if (msgs > 0 && (!ring || !ring_bytes || !offs || !lens || !inst || !idx || !verdict_out))
        return RBC_ERR_INVALID_ARG;
    if (count > r->max_count || msgs > r->max_msgs || ring_bytes > r->max_ring) return RBC_ERR_INVALID_ARG;
    const size_t n = (size_t)r->n, k = (size_t)r->k;
    size_t Smax = 0;
    for (int i = 0; i < count; ++i) {
        if (shard_lens[i] == 0 || shard_lens[i] > r->pitch) return RBC_ERR_INVALID_ARG;
        Smax = std::max(Smax, shard_lens[i]);
    }
    if (value_pitch < k * Smax) return RBC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(r->mu);
    {
        // every message's 16-byte chunks inside the ring (no wrap-around), its slot inside the
        // batch and its own
        int marked = 0;  // messages [0, marked) have their slot marked in the bitmap
        for (; marked < msgs; ++marked) {
            const int m = marked;
            if (!ring_slot_ok(offs[m], lens[m], ring_bytes, idx[m], n, inst[m], (uint32_t)count)) break;
            uint8_t &s = r->seen[(size_t)inst[m] * n + idx[m]];
            if (s) break;  // two messages for one slot
            s = 1;
        }
        for (int q = 0; q < marked; ++q) r->seen[(size_t)inst[q] * n + idx[q]] = 0;
        if (marked < msgs) return RBC_ERR_INVALID_ARG;
    }
    if (r->begin() != RBC_OK) return RBC_ERR_DEVICE;  // the one in flight keeps its status with its ticket
    hipStream_t st = r->stream;
    const size_t c = (size_t)count, mm = (size_t)msgs;
    const MetaIn mi(c, mm);
    const SmallOut so(c, mm, n);
    if (msgs) {
        memcpy(r->h_meta + mi.offs, offs, mm * 8);
        memcpy(r->h_meta + mi.lens, lens, mm * 4);
        memcpy(r->h_meta + mi.inst, inst, mm * 4);
        memcpy(r->h_meta + mi.idx, idx, mm);
    }
    memcpy(r->h_meta + mi.roots, roots, c * 32);
    uint32_t *h_slens = reinterpret_cast<uint32_t *>(r->h_meta + mi.slens);
    for (int i = 0; i < count; ++i) h_slens[i] = (uint32_t)shard_lens[i];
    WIRE_HIP(hipMemcpyAsync(r->d_meta, r->h_meta, mi.bytes, hipMemcpyHostToDevice, st));
    if (msgs) WIRE_HIP(hipMemcpyAsync(r->d_ring, ring, ring_bytes, hipMemcpyHostToDevice, st));
    WIRE_HIP(hipMemsetAsync(r->d_present, 0, c * n, st));
    WIRE_HIP(hipMemsetAsync(r->d_shards, 0, c * n * r->pitch, st));
    const uint8_t *d_roots = r->d_meta + mi.roots;
    const uint32_t *d_slens = reinterpret_cast<const uint32_t *>(r->d_meta + mi.slens);
    int32_t *d_mstatus = reinterpret_cast<int32_t *>(r->d_small + so.mstatus);
    uint8_t *d_valid = r->d_small + so.valid, *d_digests = r->d_small + so.digests;
    int32_t *d_status = reinterpret_cast<int32_t *>(r->d_small + so.status);
    int rc = rbc_dev_unmarshal_echo(r->ctx, st, count, msgs, r->d_ring,
                                    reinterpret_cast<const uint64_t *>(r->d_meta + mi.offs),
                                    reinterpret_cast<const uint32_t *>(r->d_meta + mi.lens),
                                    reinterpret_cast<const uint32_t *>(r->d_meta + mi.inst), r->d_meta + mi.idx, d_roots,
                                    d_slens, 0, r->d_shards, r->pitch, r->d_branches, r->d_present, d_mstatus,
                                    r->d_small + so.types);
    if (rc) return rc;
    // validateMessage of every decoded row, then interpolate over the proven ones with the leaves it hashed
    rc = rbc_dev_verify(r->ctx, st, count, r->d_shards, r->pitch, d_slens, 0, r->d_branches, d_roots, r->d_present,
                        d_valid, r->d_leaves);
    if (rc) return rc;
    const size_t vpitch = round_up(k * Smax, 16);
    WIRE_HIP(hipMemsetAsync(r->d_values, 0, c * vpitch, st));
    rc = rbc_dev_interpolate(r->ctx, st, count, r->d_shards, r->pitch, d_slens, 0, d_valid, r->d_leaves, 1, d_roots,
                             r->d_values, (uint32_t)vpitch, d_digests, d_status);
    if (rc) return rc;
    // pinned values at the device pitch come back in one copy of their own; else through staging
    const bool direct = value_pitch == vpitch && host_pinned(values_out) &&
                        host_pinned(values_out + (c - 1) * value_pitch + k * Smax - 1);
    const size_t vbytes = (c - 1) * vpitch + k * Smax;
    WIRE_HIP(hipMemcpyAsync(direct ? values_out : r->h_values, r->d_values, vbytes, hipMemcpyDeviceToHost, st));
    WIRE_HIP(hipMemcpyAsync(r->h_small, r->d_small, so.bytes, hipMemcpyDeviceToHost, st));
    WIRE_HIP(hipEventRecord(r->done, st));
    r->cur.count = count;
    r->cur.msgs = msgs;
    r->cur.inst = reinterpret_cast<const uint32_t *>(r->h_meta + mi.inst);
    r->cur.idx = r->h_meta + mi.idx;
    r->cur.slens = h_slens;
    r->cur.vpitch = vpitch;
    r->cur.value_pitch = value_pitch;
    r->cur.values_direct = direct;
    r->cur.verdict = verdict_out;
    r->cur.types = types_out;
    r->cur.valid = valid_out;
    r->cur.values = values_out;
    r->cur.digests = digests_out;
    r->cur.status = status_out;
    *ticket = r->issue();
    return RBC_OK;
}

int rbc_wire_receive_wait(rbc_wire_receiver *r, uint64_t ticket) { return session_wait(r, ticket); }

int rbc_wire_receive_poll(rbc_wire_receiver *r, uint64_t ticket, int *done) { return session_poll(r, ticket, done); }

}  // extern "C"
