// parity_args_check.cpp -- the argument checks of the parity-only shard commit
// (rbc_shard_commit_parity, rbc_shard_parity, rbc_split_rows and the
// device-resident rbc_dev_shard_commit_parity), built by
// tests/test_parity_only_host.py with ASan + UBSan from csrc/capi.cpp and the
// host-memory HIP stand-in tests/cpp/hip_stub.cpp.
//
// Every call here must return its documented status before any kernel
// launcher is reached: the stand-in's launchers write the ranges the kernels
// write, and the output buffers passed here are NULL or a few bytes, so a
// launch would be a crash or an ASan report.
#include <stdio.h>
#include <string.h>

#include "../../include/rbc_gpu.h"

#ifndef RBC_HAS_SHARD_COMMIT_PARITY
#error "include/rbc_gpu.h does not declare the parity-only shard commit"
#endif

static int fails = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                          \
        }                                                                     \
    } while (0)

int main() {
    rbc_ctx *ctx = nullptr;
    EXPECT(rbc_ctx_create(4, 1, 0, &ctx) == RBC_OK);  // k = 2, p = 2
    if (!ctx) return 2;
    uint8_t value[100];
    memset(value, 7, sizeof value);
    const uint8_t *values[2] = {value, value};
    const uint8_t *with_null[2] = {value, nullptr};
    size_t lens[2] = {100, 37}, zero_len[2] = {100, 0};  // Smax = 50
    uint8_t parity[8], roots[8], branches[8];            // far too small for any real output
    uint32_t slens[2];
    uint64_t ticket = 99;
    memset(parity, 0xC3, sizeof parity);

    // ---- rbc_shard_commit_parity
    EXPECT(rbc_shard_commit_parity(nullptr, 2, values, lens, parity, 64, slens, roots, branches, &ticket) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(rbc_shard_commit_parity(ctx, -1, values, lens, parity, 64, slens, roots, branches, &ticket) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(rbc_shard_commit_parity(ctx, 2, nullptr, lens, parity, 64, slens, roots, branches, &ticket) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(rbc_shard_commit_parity(ctx, 2, values, nullptr, parity, 64, slens, roots, branches, &ticket) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(rbc_shard_commit_parity(ctx, 2, values, lens, nullptr, 64, slens, roots, branches, &ticket) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(rbc_shard_commit_parity(ctx, 2, values, lens, parity, 64, slens, nullptr, branches, &ticket) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(rbc_shard_commit_parity(ctx, 2, with_null, lens, parity, 64, slens, roots, branches, &ticket) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(rbc_shard_commit_parity(ctx, 2, values, zero_len, parity, 64, slens, roots, branches, &ticket) ==
           RBC_ERR_SHORT_DATA);  // Split: len(data) == 0
    EXPECT(rbc_shard_commit_parity(ctx, 2, values, lens, parity, 49, slens, roots, branches, &ticket) ==
           RBC_ERR_INVALID_ARG);  // pitch below Smax
    EXPECT(rbc_shard_commit_parity(ctx, 2, values, lens, parity, 0, slens, roots, branches, &ticket) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(ticket == 99);
    EXPECT(rbc_shard_commit_parity(ctx, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, &ticket) == RBC_OK);
    EXPECT(ticket == 0);  // count == 0: nothing submitted
    EXPECT(rbc_shard_commit_parity(ctx, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == RBC_OK);

    // ---- rbc_shard_parity
    size_t S = 77;
    EXPECT(rbc_shard_parity(nullptr, value, 100, parity, 100, &S, roots, branches) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_shard_parity(ctx, value, 100, nullptr, 100, &S, roots, branches) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_shard_parity(ctx, value, 100, parity, 100, &S, nullptr, branches) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_shard_parity(ctx, value, 0, parity, 100, &S, roots, branches) == RBC_ERR_SHORT_DATA);
    EXPECT(rbc_shard_parity(ctx, nullptr, 100, parity, 100, &S, roots, branches) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_shard_parity(ctx, value, 100, parity, 99, &S, roots, branches) == RBC_ERR_INVALID_ARG);  // p*S = 100
    EXPECT(S == 77);

    // ---- rbc_split_rows / rbc_split_tail_bytes (the exported forms)
    const uint8_t *rows[2] = {nullptr, nullptr};
    uint8_t tail[64];
    size_t used = 5;
    EXPECT(rbc_split_tail_bytes(2, 99) == 50 && rbc_split_tail_bytes(2, 100) == 0 && rbc_split_tail_bytes(2, 0) == 0);
    EXPECT(rbc_split_rows(2, value, 0, tail, 64, rows, &S, &used) == RBC_ERR_SHORT_DATA);
    EXPECT(rbc_split_rows(0, value, 99, tail, 64, rows, &S, &used) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_split_rows(2, nullptr, 99, tail, 64, rows, &S, &used) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_split_rows(2, value, 99, tail, 64, nullptr, &S, &used) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_split_rows(2, value, 99, tail, 49, rows, &S, &used) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_split_rows(2, value, 99, nullptr, 64, rows, &S, &used) == RBC_ERR_INVALID_ARG);
    EXPECT(S == 77 && used == 5 && !rows[0] && !rows[1]);
    EXPECT(rbc_split_rows(2, value, 99, tail, 50, rows, &S, &used) == RBC_OK);
    EXPECT(S == 50 && used == 50 && rows[0] == value && rows[1] == tail && tail[48] == 7 && tail[49] == 0);

    // ---- rbc_dev_shard_commit_parity: rbc_dev_shard_commit's rules
    uint8_t dev[8];
    memset(dev, 0xC3, sizeof dev);
    uint32_t u32[2] = {100, 100};
    EXPECT(rbc_dev_shard_commit_parity(nullptr, nullptr, 1, dev, 256, nullptr, 100, dev, dev, 64, nullptr, dev, dev, dev) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_shard_commit_parity(ctx, nullptr, 1, dev, 256, u32, 0, dev, dev, 64, nullptr, dev, dev, dev) ==
           RBC_ERR_INVALID_ARG);  // per-instance value lengths need per-instance shard lengths
    EXPECT(rbc_dev_shard_commit_parity(ctx, nullptr, 1, dev, 256, nullptr, 0, dev, dev, 64, nullptr, dev, dev, dev) ==
           RBC_ERR_SHORT_DATA);
    EXPECT(rbc_dev_shard_commit_parity(ctx, nullptr, 1, dev, 256, nullptr, 100, dev, dev, 50, nullptr, dev, dev, dev) ==
           RBC_ERR_INVALID_ARG);  // pitch % 64
    EXPECT(rbc_dev_shard_commit_parity(ctx, nullptr, 1, dev, 256, nullptr, 200, dev, dev, 64, nullptr, dev, dev, dev) ==
           RBC_ERR_INVALID_ARG);  // S = 100 > pitch
    EXPECT(rbc_dev_shard_commit_parity(ctx, nullptr, 1, dev, 100, nullptr, 100, dev, dev, 64, nullptr, dev, dev, dev) ==
           RBC_ERR_INVALID_ARG);  // value_pitch < round_up(k*S, 16) + 16
    EXPECT(rbc_dev_shard_commit_parity(ctx, nullptr, 1, nullptr, 256, nullptr, 100, dev, dev, 64, nullptr, dev, dev, dev) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_shard_commit_parity(ctx, nullptr, 1, dev, 256, nullptr, 100, nullptr, dev, 64, nullptr, dev, dev, dev) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_shard_commit_parity(ctx, nullptr, 1, dev, 256, nullptr, 100, dev, nullptr, 64, nullptr, dev, dev, dev) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_shard_commit_parity(ctx, nullptr, 1, dev, 256, nullptr, 100, dev, dev, 64, nullptr, nullptr, dev, dev) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_shard_commit_parity(ctx, nullptr, 1, dev, 256, nullptr, 100, dev, dev, 64, nullptr, dev, nullptr, dev) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_shard_commit_parity(ctx, nullptr, -1, dev, 256, nullptr, 100, dev, dev, 64, nullptr, dev, dev, dev) ==
           RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_shard_commit_parity(ctx, nullptr, 0, nullptr, 256, nullptr, 100, nullptr, nullptr, 64, nullptr, nullptr,
                                       nullptr, nullptr) == RBC_OK);
    for (uint8_t b : dev) EXPECT(b == 0xC3);  // never written
    for (uint8_t b : parity) EXPECT(b == 0xC3);
    rbc_ctx_destroy(ctx);
    if (fails) {
        printf("FAIL %d\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}
