// wire_session.h -- what the three handles of the device wire path share
// (wire_rx.cpp, wire_receive.cpp, wire_ready.cpp): the 16-byte carving of
// their staging blocks, the pointer queries, the ring-slot check of one
// message, and WireSession, the one-submission-in-flight machinery behind
// every *_create / *_destroy / *_wait / *_poll.  A header, not a translation
// unit: each of the three files stays a translation unit of its own on the
// public ABI plus kernels.h, and names no launcher but its own.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <mutex>
#include <unordered_map>
#include <vector>

#include "../../include/rbc_gpu.h"

#define WIRE_HIP(expr)                                   \
    do {                                                 \
        if ((expr) != hipSuccess) return RBC_ERR_DEVICE; \
    } while (0)

namespace wire {

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

inline bool pointer_type(const void *p, hipPointerAttribute_t *at) {
    if (hipPointerGetAttributes(at, p) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

inline bool host_pinned(const void *p) {
    hipPointerAttribute_t at;
    return pointer_type(p, &at) && at.type == hipMemoryTypeHost;
}

// device memory of this device
inline bool device_memory(const void *p, int device) {
    hipPointerAttribute_t at;
    return pointer_type(p, &at) && at.type == hipMemoryTypeDevice && at.device == device;
}

// (k, p, depth) and the device of a context
inline bool wire_geometry(rbc_ctx *ctx, int *k, int *p, int *depth, int *device) {
    return rbc_ctx_params(ctx, k, p, depth) == RBC_OK && rbc_ctx_device(ctx, device) == RBC_OK;
}

// One message's place: its 16-byte chunks inside the ring (no wrap-around), its
// leaf inside the tree and, for a batch of `count` instances, its instance.
inline bool ring_slot_ok(uint64_t off, uint32_t len, size_t ring_bytes, uint32_t idx, size_t n, uint32_t inst = 0,
                         uint32_t count = 1) {
    return off % 16 == 0 && off <= ring_bytes && round_up((size_t)len, 16) <= ring_bytes - off && idx < n &&
           inst < count;
}

// A device, a stream and an event with one submission in flight.  The owner
// derives from it, allocates its blocks through dev() and pin(), and at
// submission (mu held) calls begin(), enqueues on `stream` up to the record of
// `done`, and takes its ticket from issue().  copy_out() is the owner's: it
// moves the completed submission's results to where the caller wanted them.
struct WireSession {
    int device = 0;
    std::mutex mu;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    uint64_t next_ticket = 1;
    uint64_t in_flight = 0;                     // the ticket of the one submission in flight
    std::unordered_map<uint64_t, int> retired;  // completed with an error, not yet waited on

    virtual ~WireSession() = default;
    virtual void copy_out() = 0;

    bool open(int dev_id) {
        device = dev_id;
        return hipSetDevice(device) == hipSuccess &&
               hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess &&
               hipEventCreateWithFlags(&done, hipEventDisableTiming) == hipSuccess;
    }
    bool dev(uint8_t **p, size_t bytes) {
        if (hipMalloc(reinterpret_cast<void **>(p), bytes) != hipSuccess) return false;
        dev_blocks.push_back(*p);
        return true;
    }
    bool pin(uint8_t **p, size_t bytes) {
        if (hipHostMalloc(reinterpret_cast<void **>(p), bytes, hipHostMallocDefault) != hipSuccess) return false;
        pinned_blocks.push_back(*p);
        return true;
    }
    void release() {
        for (void *p : dev_blocks) (void)hipFree(p);
        for (void *p : pinned_blocks) (void)hipHostFree(p);
        if (stream) (void)hipStreamDestroy(stream);
        if (done) (void)hipEventDestroy(done);
    }

    // completes the submission in flight; a failure stays with its ticket (caller holds mu)
    void finish() {
        if (!in_flight) return;
        if (hipEventSynchronize(done) == hipSuccess) copy_out();
        else retired[in_flight] = RBC_ERR_DEVICE;
        in_flight = 0;
    }
    // the start of a submission: the staging blocks are free again (caller holds mu)
    int begin() {
        WIRE_HIP(hipSetDevice(device));
        finish();
        return RBC_OK;
    }
    uint64_t issue() { return in_flight = next_ticket++; }

private:
    std::vector<void *> dev_blocks, pinned_blocks;
};

// the end of every *_create: hands the handle over, or unwinds what it allocated
template <class H>
int session_created(H *h, bool ok, H **out) {
    if (ok) {
        *out = h;
        return RBC_OK;
    }
    h->release();
    delete h;
    return RBC_ERR_DEVICE;
}

inline void session_destroy(WireSession *s) {
    if (!s) return;
    {
        std::lock_guard<std::mutex> lk(s->mu);
        (void)hipSetDevice(s->device);
        s->finish();
        s->release();
    }
    delete s;
}

inline int session_wait(WireSession *s, uint64_t ticket) {
    if (!s) return RBC_ERR_INVALID_ARG;
    if (ticket == 0) return RBC_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    if (ticket >= s->next_ticket) return RBC_ERR_INVALID_ARG;
    if (ticket == s->in_flight && s->begin() != RBC_OK) return RBC_ERR_DEVICE;
    auto it = s->retired.find(ticket);
    if (it == s->retired.end()) return RBC_OK;
    const int rc = it->second;
    s->retired.erase(it);
    return rc;
}

inline int session_poll(WireSession *s, uint64_t ticket, int *done) {
    if (!s || !done) return RBC_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(s->mu);
    if (ticket >= s->next_ticket) return RBC_ERR_INVALID_ARG;
    *done = 1;
    if (ticket && ticket == s->in_flight) {
        const hipError_t e = hipEventQuery(s->done);
        if (e == hipErrorNotReady) *done = 0;
        else if (e != hipSuccess) return RBC_ERR_DEVICE;
    }
    return RBC_OK;
}

}  // namespace wire
