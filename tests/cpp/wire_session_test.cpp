// wire_session_test.cpp -- csrc/wire_session.h on its own, no GPU: a
// stand-alone program (own main) that includes the header, defines the HIP
// entry points it uses over host memory, and can make the completion event
// fail, report "not ready", or make the k-th allocation fail.  It pins what
// the three wire handles share and tests/cpp/hip_stub.cpp (which always
// succeeds) cannot reach: a failed completion runs no copy-out and is reported
// by wait() against its own ticket exactly once, and a create whose k-th
// allocation fails frees what it had (the leak check of ASan covers it).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../cleisthenes_amd/csrc/wire_session.h"

namespace {

// ---- the switches -----------------------------------------------------------
bool g_sync_fails = false;      // the next hipEventSynchronize returns an error
bool g_not_ready = false;       // hipEventQuery returns hipErrorNotReady
bool g_set_device_fails = false;
int g_fail_alloc = 0;           // the g_fail_alloc-th allocation from now fails (0: none)
bool g_device_set = false;      // hipSetDevice ran since the test last cleared it
int g_syncs = 0, g_copied = 0, g_checks = 0;

struct Block {
    const uint8_t *base;
    size_t bytes;
    hipMemoryType type;
};
std::vector<Block> g_blocks;

hipError_t allocate(void **p, size_t bytes, hipMemoryType type) {
    if (g_fail_alloc && --g_fail_alloc == 0) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    g_blocks.push_back({static_cast<const uint8_t *>(*p), bytes, type});
    return hipSuccess;
}

hipError_t release(void *p, hipMemoryType type) {
    for (size_t i = 0; i < g_blocks.size(); ++i)
        if (g_blocks[i].base == p && g_blocks[i].type == type) {
            g_blocks.erase(g_blocks.begin() + (long)i);
            free(p);
            return hipSuccess;
        }
    fprintf(stderr, "FAIL: freed %p, which is no live block of that kind\n", p);
    exit(1);
}

#define CHECK(cond)                                                     \
    do {                                                                \
        ++g_checks;                                                     \
        if (!(cond)) {                                                  \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

}  // namespace

// ---- the HIP entry points of wire_session.h ---------------------------------
hipError_t hipSetDevice(int d) {
    if (g_set_device_fails || d != 0) return hipErrorInvalidDevice;
    g_device_set = true;
    return hipSuccess;
}
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipMalloc(void **p, size_t bytes) { return allocate(p, bytes, hipMemoryTypeDevice); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return allocate(p, bytes, hipMemoryTypeHost); }
hipError_t hipFree(void *p) { return release(p, hipMemoryTypeDevice); }
hipError_t hipHostFree(void *p) { return release(p, hipMemoryTypeHost); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int) {
    *s = static_cast<hipStream_t>(malloc(1));
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
    free(s);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned int) {
    *e = static_cast<hipEvent_t>(malloc(1));
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    free(e);
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t) {
    ++g_syncs;
    if (!g_device_set) {
        fprintf(stderr, "FAIL: a completion before hipSetDevice\n");
        exit(1);
    }
    if (g_sync_fails) {
        g_sync_fails = false;
        return hipErrorUnknown;
    }
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t) { return g_not_ready ? hipErrorNotReady : hipSuccess; }
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *a, const void *p) {
    const uint8_t *q = static_cast<const uint8_t *>(p);
    for (const Block &b : g_blocks)
        if (q >= b.base && q < b.base + b.bytes) {
            *a = hipPointerAttribute_t{};
            a->type = b.type;
            a->device = 0;
            return hipSuccess;
        }
    return hipErrorInvalidValue;
}

// ---- the two context queries of wire_geometry() -----------------------------
struct rbc_ctx {
    int k, p, depth, device;
};
extern "C" int rbc_ctx_params(const rbc_ctx *ctx, int *k, int *p, int *depth) {
    if (!ctx) return RBC_ERR_INVALID_ARG;
    *k = ctx->k, *p = ctx->p, *depth = ctx->depth;
    return RBC_OK;
}
extern "C" int rbc_ctx_device(const rbc_ctx *ctx, int *device) {
    if (!ctx) return RBC_ERR_INVALID_ARG;
    *device = ctx->device;
    return RBC_OK;
}

namespace {

using namespace wire;

// a handle in the manner of the three real ones: two device and two pinned blocks
struct Handle : WireSession {
    uint8_t *d_a = nullptr, *d_b = nullptr, *h_a = nullptr, *h_b = nullptr;
    void copy_out() override { ++g_copied; }
};

int create(Handle **out) {
    *out = nullptr;
    Handle *h = new Handle();
    const bool ok = h->open(0) && h->dev(&h->d_a, 64) && h->dev(&h->d_b, 32) && h->pin(&h->h_a, 64) &&
                    h->pin(&h->h_b, 16);
    return session_created(h, ok, out);
}

// a submission: completes the one in flight, "enqueues", takes the ticket
uint64_t submit(Handle *h) {
    std::lock_guard<std::mutex> lk(h->mu);
    g_device_set = false;
    CHECK(h->begin() == RBC_OK);
    return h->issue();
}

int wait_on(Handle *h, uint64_t t) {
    g_device_set = false;
    return session_wait(h, t);
}

void test_helpers() {
    CHECK(round_up(0, 16) == 0 && round_up(1, 16) == 16 && round_up(16, 16) == 16 && round_up(17, 16) == 32);
    alignas(16) uint8_t buf[32];
    CHECK(aligned16(buf) && !aligned16(buf + 1) && aligned16(buf + 16));
    Carver c;
    CHECK(c.take(1) == 0 && c.take(16) == 16 && c.take(17) == 32 && c.take(0) == 64 && c.o == 64);
    // offset and length inside the ring, the leaf inside the tree, the instance inside the batch
    CHECK(ring_slot_ok(0, 64, 64, 3, 4));
    CHECK(ring_slot_ok(64, 0, 64, 0, 4));    // an empty message at the ring's end
    CHECK(!ring_slot_ok(8, 16, 64, 0, 4));   // offset not a multiple of 16
    CHECK(!ring_slot_ok(80, 0, 64, 0, 4));   // offset past the ring
    CHECK(!ring_slot_ok(48, 17, 64, 0, 4));  // the last 16-byte chunk crosses the end
    CHECK(ring_slot_ok(48, 16, 64, 0, 4));
    CHECK(!ring_slot_ok(0, 16, 64, 4, 4));   // idx == n
    CHECK(ring_slot_ok(0, 16, 64, 0, 4, 1, 2) && !ring_slot_ok(0, 16, 64, 0, 4, 2, 2));  // inst < count
    CHECK(!ring_slot_ok(~0ull & ~15ull, 0xffffffffu, 64, 0, 4));  // no wrap-around
    rbc_ctx ctx{3, 2, 3, 0};
    int k = 0, p = 0, depth = 0, device = -1;
    CHECK(wire_geometry(&ctx, &k, &p, &depth, &device) && k == 3 && p == 2 && depth == 3 && device == 0);
    CHECK(!wire_geometry(nullptr, &k, &p, &depth, &device));
}

void test_pointer_queries(Handle *h) {
    uint8_t local = 0;
    CHECK(device_memory(h->d_a, 0) && device_memory(h->d_a + 63, 0) && !device_memory(h->d_a, 1));
    CHECK(!device_memory(h->h_a, 0) && !device_memory(&local, 0));
    CHECK(host_pinned(h->h_a) && host_pinned(h->h_b + 15) && !host_pinned(h->d_a) && !host_pinned(&local));
}

void test_tickets(Handle *h) {
    int done = -1;
    // ticket 0 and tickets not issued yet
    CHECK(wait_on(h, 0) == RBC_OK && session_poll(h, 0, &done) == RBC_OK && done == 1);
    CHECK(wait_on(nullptr, 0) == RBC_ERR_INVALID_ARG && session_poll(nullptr, 0, &done) == RBC_ERR_INVALID_ARG);
    CHECK(session_poll(h, 0, nullptr) == RBC_ERR_INVALID_ARG);
    CHECK(wait_on(h, 1) == RBC_ERR_INVALID_ARG && session_poll(h, 1, &done) == RBC_ERR_INVALID_ARG);
    CHECK(g_syncs == 0 && g_copied == 0);

    // one submission: poll while not ready and afterwards, wait, wait again
    const uint64_t t1 = submit(h);
    CHECK(t1 == 1 && g_syncs == 0);
    g_not_ready = true;
    CHECK(session_poll(h, t1, &done) == RBC_OK && done == 0);
    g_not_ready = false;
    CHECK(session_poll(h, t1, &done) == RBC_OK && done == 1 && g_copied == 0);  // poll completes nothing
    CHECK(wait_on(h, t1 + 1) == RBC_ERR_INVALID_ARG);
    CHECK(wait_on(h, t1) == RBC_OK && g_copied == 1 && g_syncs == 1);
    CHECK(wait_on(h, t1) == RBC_OK && g_copied == 1 && g_syncs == 1);  // already completed
    g_not_ready = true;  // a completed ticket is done whatever the event says
    CHECK(session_poll(h, t1, &done) == RBC_OK && done == 1);
    g_not_ready = false;

    // a failed completion: no copy-out, RBC_ERR_DEVICE exactly once
    const uint64_t t2 = submit(h);
    CHECK(t2 == t1 + 1);
    g_sync_fails = true;
    CHECK(wait_on(h, t2) == RBC_ERR_DEVICE && g_copied == 1);
    CHECK(wait_on(h, t2) == RBC_OK && g_copied == 1);

    // the failure is met by the next submission: it proceeds, gets the next ticket and
    // completes normally; the error stays with its own ticket
    const uint64_t t3 = submit(h);
    g_sync_fails = true;
    const uint64_t t4 = submit(h);
    CHECK(t3 == t2 + 1 && t4 == t3 + 1 && g_copied == 1 && !g_sync_fails);
    CHECK(session_poll(h, t3, &done) == RBC_OK && done == 1);
    CHECK(wait_on(h, t4) == RBC_OK && g_copied == 2);
    CHECK(wait_on(h, t3) == RBC_ERR_DEVICE && wait_on(h, t3) == RBC_OK && g_copied == 2);

    // two tickets retired with errors, each reported against its own number
    const uint64_t t5 = submit(h);
    g_sync_fails = true;
    const uint64_t t6 = submit(h);
    g_sync_fails = true;
    const uint64_t t7 = submit(h);
    CHECK(g_copied == 2 && h->retired.size() == 2);
    CHECK(wait_on(h, t6) == RBC_ERR_DEVICE && h->retired.size() == 1);
    CHECK(wait_on(h, t7) == RBC_OK && g_copied == 3);
    CHECK(wait_on(h, t5) == RBC_ERR_DEVICE && h->retired.empty());
    CHECK(wait_on(h, t5) == RBC_OK && wait_on(h, t6) == RBC_OK && wait_on(h, t7) == RBC_OK && g_copied == 3);

    // hipSetDevice fails: the ticket stays in flight, and completes on the next wait
    const uint64_t t8 = submit(h);
    g_set_device_fails = true;
    CHECK(wait_on(h, t8) == RBC_ERR_DEVICE && g_copied == 3 && h->in_flight == t8);
    g_set_device_fails = false;
    CHECK(wait_on(h, t8) == RBC_OK && g_copied == 4);
}

}  // namespace

int main() {
    test_helpers();
    // a create whose k-th allocation fails frees the k-1 before it, the stream and the event
    for (int k = 1; k <= 4; ++k) {
        Handle *h = reinterpret_cast<Handle *>(1);
        g_fail_alloc = k;
        CHECK(create(&h) == RBC_ERR_DEVICE && h == nullptr && g_blocks.empty() && g_fail_alloc == 0);
    }
    Handle *h = nullptr;
    CHECK(create(&h) == RBC_OK && h && g_blocks.size() == 4);
    test_pointer_queries(h);
    test_tickets(h);
    // destroy completes the submission in flight, after hipSetDevice, and frees every block
    const uint64_t last = submit(h);
    CHECK(last == 9);
    g_device_set = false;
    session_destroy(h);
    CHECK(g_copied == 5 && g_blocks.empty());
    session_destroy(nullptr);
    printf("ok %d checks\n", g_checks);
    return 0;
}
