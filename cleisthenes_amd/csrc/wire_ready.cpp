// wire_ready.cpp -- READYs from wire bytes to per-instance quorums
// (include/rbc_protocol.h, RBC_HAS_WIRE_READY): rbc_dev_unmarshal_ready,
// rbc_dev_quorum and rbc_wire_quorum.  A ring of received READY pb.Message
// bytes for `count` instances is decoded on the device into the caller's
// [count][n] sender bitmap (unmarshal_ready_kernel, wire.hip), and the bitmap
// is tallied with verify's valid[] and interpolate's status into the counts and
// decisions of rbc_node's advance() (quorum_kernel): one submission, one copy
// of the ring, one copy back.
//
// A translation unit of its own on the public ABI plus kernels.h, like
// wire_rx.cpp and wire_receive.cpp, with which it shares the session behind
// the handle (stream, event, staging blocks, tickets: wire_session.h): the
// host runtime (capi.cpp) does not know it.
#include <string.h>

#include "../../include/rbc_protocol.h"
#include "kernels.h"
#include "wire_session.h"

using namespace wire;

namespace {

// host-to-device metadata of one call; the bitmap behind it goes to SmallOut's place
struct MetaIn {
    size_t offs, lens, inst, idx, roots, valid, status, bytes, ready, total;
    MetaIn(size_t count, size_t msgs, size_t n) {
        Carver c;
        offs = c.take(msgs * 8);
        lens = c.take(msgs * 4);
        inst = c.take(msgs * 4);
        idx = c.take(msgs);
        roots = c.take(count * 32);
        valid = c.take(count * n);
        status = c.take(count * 4);
        bytes = c.o;
        ready = c.take(count * n);
        total = c.o;
    }
};

// everything that crosses back, in one copy
struct SmallOut {
    size_t mstatus, ready, ecounts, rcounts, flags, bytes;
    SmallOut(size_t count, size_t msgs, size_t n) {
        Carver c;
        mstatus = c.take(msgs * 4);
        ready = c.take(count * n);
        ecounts = c.take(count * 4);
        rcounts = c.take(count * 4);
        flags = c.take(count);
        bytes = c.o;
    }
};

// The size of the one canonical READY, from the host encoder itself.
uint32_t ready_message_size() {
    const uint8_t root[32] = {0};
    uint8_t json[128];
    const size_t jl = rbc_json_encode_ready(root, sizeof root, json, sizeof json);
    if (jl == 0 || jl > sizeof json) return 0;
    return (uint32_t)rbc_pb_encode_rbc(RBC_MSG_READY, json, jl, nullptr, 0);
}

// (n, f) and the device of a context: n = k + p, p = 2f
bool geometry(rbc_ctx *ctx, int *n, int *f, int *device) {
    int k = 0, p = 0, depth = 0;
    if (!wire_geometry(ctx, &k, &p, &depth, device)) return false;
    *n = k + p;
    *f = p / 2;
    return true;
}

}  // namespace

struct rbc_wire_quorum_handle : WireSession {
    rbc_ctx *ctx = nullptr;
    int n = 0, max_count = 0, max_msgs = 0;
    size_t max_ring = 0;
    uint8_t *d_ring = nullptr, *d_meta = nullptr, *d_small = nullptr;
    uint8_t *h_meta = nullptr, *h_small = nullptr;  // pinned
    // the one submission in flight
    struct {
        int count = 0, msgs = 0;
        uint8_t *ready = nullptr, *verdict = nullptr, *flags = nullptr;
        uint32_t *ecounts = nullptr, *rcounts = nullptr;
    } cur;

    void copy_out() override {
        const size_t count = (size_t)cur.count, msgs = (size_t)cur.msgs;
        const SmallOut so(count, msgs, (size_t)n);
        const int32_t *ms = reinterpret_cast<const int32_t *>(h_small + so.mstatus);
        for (size_t m = 0; m < msgs; ++m) cur.verdict[m] = (uint8_t)ms[m];
        memcpy(cur.ready, h_small + so.ready, count * n);
        memcpy(cur.ecounts, h_small + so.ecounts, count * 4);
        memcpy(cur.rcounts, h_small + so.rcounts, count * 4);
        memcpy(cur.flags, h_small + so.flags, count);
    }
};

extern "C" {

int rbc_dev_unmarshal_ready(rbc_ctx *ctx, void *stream, int count, int msgs, const uint8_t *ring,
                            const uint64_t *offs, const uint32_t *lens, const uint32_t *inst, const uint8_t *idx,
                            const uint8_t *roots, uint8_t *ready, int32_t *msg_status) {
    if (!ctx || count < 0 || msgs < 0) return RBC_ERR_INVALID_ARG;
    if (!ring || !offs || !lens || !inst || !idx || !roots || !ready || !msg_status) return RBC_ERR_INVALID_ARG;
    if (!aligned16(ring) || !aligned16(roots)) return RBC_ERR_INVALID_ARG;
    if (msgs == 0) return RBC_OK;
    if (count == 0) return RBC_ERR_INVALID_ARG;  // messages of no instance
    int n = 0, f = 0, device = 0;
    if (!geometry(ctx, &n, &f, &device)) return RBC_ERR_INVALID_ARG;
    WIRE_HIP(hipSetDevice(device));
    WireReadyArgs a{};
    a.count = count;
    a.msgs = msgs;
    a.n = n;
    a.msg_len = ready_message_size();
    a.ring = ring;
    a.offs = offs;
    a.lens = lens;
    a.inst = inst;
    a.idx = idx;
    a.roots = roots;
    a.ready = ready;
    a.msg_status = msg_status;
    WIRE_HIP(rbc_launch_unmarshal_ready(a, reinterpret_cast<hipStream_t>(stream)));
    return RBC_OK;
}

int rbc_dev_quorum(rbc_ctx *ctx, void *stream, int count, const uint8_t *valid, uint8_t *ready,
                   const int32_t *status, int self, uint32_t *echo_counts, uint32_t *ready_counts, uint8_t *flags) {
    if (!ctx || count < 0 || !ready || !echo_counts || !ready_counts || !flags) return RBC_ERR_INVALID_ARG;
    int n = 0, f = 0, device = 0;
    if (!geometry(ctx, &n, &f, &device)) return RBC_ERR_INVALID_ARG;
    if (self < -1 || self >= n) return RBC_ERR_INVALID_ARG;
    if (count == 0) return RBC_OK;
    WIRE_HIP(hipSetDevice(device));
    QuorumArgs a{};
    a.count = count;
    a.n = n;
    a.f = f;
    a.self = self;
    a.valid = valid;
    a.ready = ready;
    a.status = status;
    a.echo_counts = echo_counts;
    a.ready_counts = ready_counts;
    a.flags = flags;
    WIRE_HIP(rbc_launch_quorum(a, reinterpret_cast<hipStream_t>(stream)));
    return RBC_OK;
}

int rbc_wire_quorum_create(rbc_ctx *ctx, int max_count, int max_msgs, size_t max_ring_bytes,
                           rbc_wire_quorum_handle **out) {
    if (!out) return RBC_ERR_INVALID_ARG;
    *out = nullptr;
    if (!ctx || max_count <= 0 || max_msgs <= 0 || max_ring_bytes == 0) return RBC_ERR_INVALID_ARG;
    int n = 0, f = 0, device = 0;
    if (!geometry(ctx, &n, &f, &device)) return RBC_ERR_INVALID_ARG;
    rbc_wire_quorum_handle *q = new rbc_wire_quorum_handle();
    q->ctx = ctx;
    q->n = n;
    q->max_count = max_count;
    q->max_msgs = max_msgs;
    q->max_ring = max_ring_bytes;
    const size_t meta = MetaIn((size_t)max_count, (size_t)max_msgs, (size_t)n).total;
    const size_t small = SmallOut((size_t)max_count, (size_t)max_msgs, (size_t)n).bytes;
    const bool ok = q->open(device) && q->dev(&q->d_ring, round_up(max_ring_bytes, 16)) && q->dev(&q->d_meta, meta) &&
                    q->dev(&q->d_small, small) && q->pin(&q->h_meta, meta) && q->pin(&q->h_small, small);
    return session_created(q, ok, out);
}

void rbc_wire_quorum_destroy(rbc_wire_quorum_handle *q) { session_destroy(q); }

int rbc_wire_quorum(rbc_wire_quorum_handle *q, int count, int msgs, const uint8_t *ring, size_t ring_bytes,
                    const uint64_t *offs, const uint32_t *lens, const uint32_t *inst, const uint8_t *idx,
                    const uint8_t *roots, const uint8_t *valid, const int32_t *status, int self,
                    uint8_t *ready_inout, uint8_t *verdict_out, uint32_t *echo_counts_out,
                    uint32_t *ready_counts_out, uint8_t *flags_out, uint64_t *ticket) {
    if (!q || count < 0 || msgs < 0 || !ticket) return RBC_ERR_INVALID_ARG;
    if (self < -1 || self >= q->n) return RBC_ERR_INVALID_ARG;
    if (count == 0) {
        if (msgs) return RBC_ERR_INVALID_ARG;  // messages of no instance
        *ticket = 0;
        return RBC_OK;
    }
    if (!ready_inout || !echo_counts_out || !ready_counts_out || !flags_out) return RBC_ERR_INVALID_ARG;
    if (msgs > 0 && (!ring || !ring_bytes || !offs || !lens || !inst || !idx || !roots || !verdict_out))
        return RBC_ERR_INVALID_ARG;
    if (count > q->max_count || msgs > q->max_msgs || (msgs > 0 && ring_bytes > q->max_ring))
        return RBC_ERR_INVALID_ARG;
    const size_t n = (size_t)q->n;
    // every message's 16-byte chunks inside the ring (no wrap-around), its slot inside the bitmap;
    // two messages for one slot are fine: both can only set it
    for (int m = 0; m < msgs; ++m) {
        if (!ring_slot_ok(offs[m], lens[m], ring_bytes, idx[m], n, inst[m], (uint32_t)count))
            return RBC_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(q->mu);
    if (q->begin() != RBC_OK) return RBC_ERR_DEVICE;  // the one in flight keeps its status with its ticket
    hipStream_t st = q->stream;
    const size_t c = (size_t)count, mm = (size_t)msgs;
    const MetaIn mi(c, mm, n);
    const SmallOut so(c, mm, n);
    if (msgs) {
        memcpy(q->h_meta + mi.offs, offs, mm * 8);
        memcpy(q->h_meta + mi.lens, lens, mm * 4);
        memcpy(q->h_meta + mi.inst, inst, mm * 4);
        memcpy(q->h_meta + mi.idx, idx, mm);
        memcpy(q->h_meta + mi.roots, roots, c * 32);
    }
    if (valid) memcpy(q->h_meta + mi.valid, valid, c * n);
    if (status) memcpy(q->h_meta + mi.status, status, c * 4);
    memcpy(q->h_meta + mi.ready, ready_inout, c * n);
    WIRE_HIP(hipMemcpyAsync(q->d_meta, q->h_meta, mi.bytes, hipMemcpyHostToDevice, st));
    // the bitmap goes where the copy back takes it from
    uint8_t *d_ready = q->d_small + so.ready;
    WIRE_HIP(hipMemcpyAsync(d_ready, q->h_meta + mi.ready, c * n, hipMemcpyHostToDevice, st));
    if (msgs) {
        WIRE_HIP(hipMemcpyAsync(q->d_ring, ring, ring_bytes, hipMemcpyHostToDevice, st));
        const int rc = rbc_dev_unmarshal_ready(
            q->ctx, st, count, msgs, q->d_ring, reinterpret_cast<const uint64_t *>(q->d_meta + mi.offs),
            reinterpret_cast<const uint32_t *>(q->d_meta + mi.lens),
            reinterpret_cast<const uint32_t *>(q->d_meta + mi.inst), q->d_meta + mi.idx, q->d_meta + mi.roots, d_ready,
            reinterpret_cast<int32_t *>(q->d_small + so.mstatus));
        if (rc) return rc;
    }
    const int rc = rbc_dev_quorum(q->ctx, st, count, valid ? q->d_meta + mi.valid : nullptr, d_ready,
                                  status ? reinterpret_cast<const int32_t *>(q->d_meta + mi.status) : nullptr, self,
                                  reinterpret_cast<uint32_t *>(q->d_small + so.ecounts),
                                  reinterpret_cast<uint32_t *>(q->d_small + so.rcounts), q->d_small + so.flags);
    if (rc) return rc;
    WIRE_HIP(hipMemcpyAsync(q->h_small, q->d_small, so.bytes, hipMemcpyDeviceToHost, st));
    WIRE_HIP(hipEventRecord(q->done, st));
    q->cur.count = count;
    q->cur.msgs = msgs;
    q->cur.ready = ready_inout;
    q->cur.verdict = verdict_out;
    q->cur.ecounts = echo_counts_out;
    q->cur.rcounts = ready_counts_out;
    q->cur.flags = flags_out;
    *ticket = q->issue();
    return RBC_OK;
}

int rbc_wire_quorum_wait(rbc_wire_quorum_handle *q, uint64_t ticket) { return session_wait(q, ticket); }

int rbc_wire_quorum_poll(rbc_wire_quorum_handle *q, uint64_t ticket, int *done) {
    return session_poll(q, ticket, done);
}

}  // extern "C"
