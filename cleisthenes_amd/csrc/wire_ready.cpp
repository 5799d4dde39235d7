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
// wire_rx.cpp and wire_receive.cpp: the host runtime (capi.cpp) does not know
// it.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <unordered_map>

#include "../../include/rbc_gpu.h"
#include "../../include/rbc_protocol.h"
#include "kernels.h"

namespace {

constexpr size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// one block of 16-byte aligned pieces
struct Carver {
    size_t o = 0;
    size_t take(size_t n) {
        const size_t at = o;
        o += round_up(n, 16);
        return at;
    }
};

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
    if (rbc_ctx_params(ctx, &k, &p, &depth) != RBC_OK || rbc_ctx_device(ctx, device) != RBC_OK) return false;
    *n = k + p;
    *f = p / 2;
    return true;
}

}  // namespace

struct rbc_wire_quorum_handle {
    rbc_ctx *ctx = nullptr;
    int n = 0, device = 0, max_count = 0, max_msgs = 0;
    size_t max_ring = 0;
    std::mutex mu;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    uint8_t *d_ring = nullptr, *d_meta = nullptr, *d_small = nullptr;
    uint8_t *h_meta = nullptr, *h_small = nullptr;  // pinned
    uint64_t next_ticket = 1;
    // the one submission in flight
    struct {
        uint64_t ticket = 0;
        int count = 0, msgs = 0;
        uint8_t *ready = nullptr, *verdict = nullptr, *flags = nullptr;
        uint32_t *ecounts = nullptr, *rcounts = nullptr;
    } cur;
    std::unordered_map<uint64_t, int> retired;  // completed with an error, not yet waited on

    void release() {
        for (uint8_t *p : {d_ring, d_meta, d_small})
            if (p) (void)hipFree(p);
        for (uint8_t *p : {h_meta, h_small})
            if (p) (void)hipHostFree(p);
        if (stream) (void)hipStreamDestroy(stream);
        if (done) (void)hipEventDestroy(done);
    }

    // completes the submission in flight (caller holds mu)
    int finish() {
        if (!cur.ticket) return RBC_OK;
        const hipError_t e = hipEventSynchronize(done);
        if (e == hipSuccess) {
            const size_t count = (size_t)cur.count, msgs = (size_t)cur.msgs;
            const SmallOut so(count, msgs, (size_t)n);
            const int32_t *ms = reinterpret_cast<const int32_t *>(h_small + so.mstatus);
            for (size_t m = 0; m < msgs; ++m) cur.verdict[m] = (uint8_t)ms[m];
            memcpy(cur.ready, h_small + so.ready, count * n);
            memcpy(cur.ecounts, h_small + so.ecounts, count * 4);
            memcpy(cur.rcounts, h_small + so.rcounts, count * 4);
            memcpy(cur.flags, h_small + so.flags, count);
        } else {
            retired[cur.ticket] = RBC_ERR_DEVICE;
        }
        cur.ticket = 0;
        return e == hipSuccess ? RBC_OK : RBC_ERR_DEVICE;
    }
};

#define RDY_HIP(expr)                                    \
    do {                                                 \
        if ((expr) != hipSuccess) return RBC_ERR_DEVICE; \
    } while (0)

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
    RDY_HIP(hipSetDevice(device));
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
    RDY_HIP(rbc_launch_unmarshal_ready(a, reinterpret_cast<hipStream_t>(stream)));
    return RBC_OK;
}

int rbc_dev_quorum(rbc_ctx *ctx, void *stream, int count, const uint8_t *valid, uint8_t *ready,
                   const int32_t *status, int self, uint32_t *echo_counts, uint32_t *ready_counts, uint8_t *flags) {
    if (!ctx || count < 0 || !ready || !echo_counts || !ready_counts || !flags) return RBC_ERR_INVALID_ARG;
    int n = 0, f = 0, device = 0;
    if (!geometry(ctx, &n, &f, &device)) return RBC_ERR_INVALID_ARG;
    if (self < -1 || self >= n) return RBC_ERR_INVALID_ARG;
    if (count == 0) return RBC_OK;
    RDY_HIP(hipSetDevice(device));
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
    RDY_HIP(rbc_launch_quorum(a, reinterpret_cast<hipStream_t>(stream)));
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
    q->device = device;
    q->max_count = max_count;
    q->max_msgs = max_msgs;
    q->max_ring = max_ring_bytes;
    const size_t meta = MetaIn((size_t)max_count, (size_t)max_msgs, (size_t)n).total;
    const size_t small = SmallOut((size_t)max_count, (size_t)max_msgs, (size_t)n).bytes;
    auto dev = [](uint8_t **p, size_t bytes) { return hipMalloc(reinterpret_cast<void **>(p), bytes) == hipSuccess; };
    auto pin = [](uint8_t **p, size_t bytes) {
        return hipHostMalloc(reinterpret_cast<void **>(p), bytes, hipHostMallocDefault) == hipSuccess;
    };
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&q->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&q->done, hipEventDisableTiming) != hipSuccess ||
        !dev(&q->d_ring, round_up(max_ring_bytes, 16)) || !dev(&q->d_meta, meta) || !dev(&q->d_small, small) ||
        !pin(&q->h_meta, meta) || !pin(&q->h_small, small)) {
        q->release();
        delete q;
        return RBC_ERR_DEVICE;
    }
    *out = q;
    return RBC_OK;
}

void rbc_wire_quorum_destroy(rbc_wire_quorum_handle *q) {
    if (!q) return;
    {
        std::lock_guard<std::mutex> lk(q->mu);
        (void)hipSetDevice(q->device);
        (void)q->finish();
        q->release();
    }
    delete q;
}

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
        if (offs[m] % 16 || offs[m] > ring_bytes || round_up((size_t)lens[m], 16) > ring_bytes - offs[m] ||
            inst[m] >= (uint32_t)count || idx[m] >= n)
            return RBC_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(q->mu);
    RDY_HIP(hipSetDevice(q->device));
    (void)q->finish();  // the staging blocks are free again (its status stays with its ticket)
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
    RDY_HIP(hipMemcpyAsync(q->d_meta, q->h_meta, mi.bytes, hipMemcpyHostToDevice, st));
    // the bitmap goes where the copy back takes it from
    uint8_t *d_ready = q->d_small + so.ready;
    RDY_HIP(hipMemcpyAsync(d_ready, q->h_meta + mi.ready, c * n, hipMemcpyHostToDevice, st));
    if (msgs) {
        RDY_HIP(hipMemcpyAsync(q->d_ring, ring, ring_bytes, hipMemcpyHostToDevice, st));
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
    RDY_HIP(hipMemcpyAsync(q->h_small, q->d_small, so.bytes, hipMemcpyDeviceToHost, st));
    RDY_HIP(hipEventRecord(q->done, st));
    q->cur.ticket = q->next_ticket++;
    q->cur.count = count;
    q->cur.msgs = msgs;
    q->cur.ready = ready_inout;
    q->cur.verdict = verdict_out;
    q->cur.ecounts = echo_counts_out;
    q->cur.rcounts = ready_counts_out;
    q->cur.flags = flags_out;
    *ticket = q->cur.ticket;
    return RBC_OK;
}

int rbc_wire_quorum_wait(rbc_wire_quorum_handle *q, uint64_t ticket) {
    if (!q) return RBC_ERR_INVALID_ARG;
    if (ticket == 0) return RBC_OK;
    std::lock_guard<std::mutex> lk(q->mu);
    if (ticket >= q->next_ticket) return RBC_ERR_INVALID_ARG;
    if (ticket == q->cur.ticket) {
        RDY_HIP(hipSetDevice(q->device));
        (void)q->finish();
    }
    auto it = q->retired.find(ticket);
    if (it == q->retired.end()) return RBC_OK;
    const int rc = it->second;
    q->retired.erase(it);
    return rc;
}

int rbc_wire_quorum_poll(rbc_wire_quorum_handle *q, uint64_t ticket, int *done) {
    if (!q || !done) return RBC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(q->mu);
    if (ticket >= q->next_ticket) return RBC_ERR_INVALID_ARG;
    *done = 1;
    if (ticket && ticket == q->cur.ticket) {
        const hipError_t e = hipEventQuery(q->done);
        if (e == hipErrorNotReady) *done = 0;
        else if (e != hipSuccess) return RBC_ERR_DEVICE;
    }
    return RBC_OK;
}

}  // extern "C"
