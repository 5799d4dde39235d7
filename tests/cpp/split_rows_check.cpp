// split_rows_check.cpp -- stand-alone driver of rbc_split_rows' body
// (csrc/host_shared.h: rbc_split_rows_impl / rbc_split_tail_bytes_impl), built
// by tests/test_parity_only_host.py with ASan + UBSan from that header alone.
//
// For every k in {1, 2, 13, 44, 86} and len in [1, 3k + 2], plus a few large
// lengths, against a plain padded copy of the value (klauspost Split):
//   * rows wholly inside the value point into `data` itself, at j*S;
//   * every other row lies in the tail and holds the padded copy's bytes;
//   * *tail_used == rbc_split_tail_bytes(k, len), a tail of exactly that many
//     bytes (a heap block of that size: one byte more is an ASan report) is
//     enough, and a tail one byte smaller is rejected with nothing written.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cleisthenes_amd/csrc/host_shared.h"

static int fails = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                          \
        }                                                                     \
    } while (0)

static void one(int k, size_t len) {
    const size_t S = (len + k - 1) / k;
    std::vector<uint8_t> data(len);
    for (size_t i = 0; i < len; ++i) data[i] = (uint8_t)(1 + (i * 131 + (size_t)k) % 255);  // never zero
    std::vector<uint8_t> padded((size_t)k * S, 0);
    memcpy(padded.data(), data.data(), len);

    const size_t need = rbc_split_tail_bytes_impl(k, len);
    EXPECT(need == ((size_t)k - len / S) * S);
    // exactly `need` bytes on the heap (malloc(0) may be NULL: the contract allows a NULL tail then)
    uint8_t *tail = need ? (uint8_t *)malloc(need) : nullptr;
    if (need) memset(tail, 0xEE, need);
    std::vector<const uint8_t *> rows((size_t)k, nullptr);
    size_t s_out = 0, used = ~(size_t)0;
    EXPECT(rbc_split_rows_impl(k, data.data(), len, tail, need, rows.data(), &s_out, &used) == 0);
    EXPECT(s_out == S);
    EXPECT(used == need);
    size_t in_tail = 0;
    for (int j = 0; j < k; ++j) {
        if (((size_t)j + 1) * S <= len) {
            EXPECT(rows[j] == data.data() + (size_t)j * S);
        } else {
            EXPECT(rows[j] == tail + in_tail * S);
            ++in_tail;
        }
        EXPECT(rows[j] && memcmp(rows[j], padded.data() + (size_t)j * S, S) == 0);
    }
    EXPECT(in_tail * S == need);

    if (need) {  // one byte short: rejected, nothing written
        memset(tail, 0xEE, need);
        std::vector<const uint8_t *> r2((size_t)k, nullptr);
        size_t s2 = 12345, u2 = 12345;
        EXPECT(rbc_split_rows_impl(k, data.data(), len, tail, need - 1, r2.data(), &s2, &u2) == -10);
        EXPECT(s2 == 12345 && u2 == 12345);
        for (size_t b = 0; b < need; ++b) EXPECT(tail[b] == 0xEE);
        for (int j = 0; j < k; ++j) EXPECT(r2[j] == nullptr);
        EXPECT(rbc_split_rows_impl(k, data.data(), len, nullptr, need, r2.data(), nullptr, nullptr) == -10);
    }
    free(tail);
}

int main() {
    const int ks[] = {1, 2, 13, 44, 86};
    long cases = 0;
    for (int k : ks) {
        for (size_t len = 1; len <= (size_t)3 * k + 2; ++len, ++cases) one(k, len);
        for (size_t len : {(size_t)k * 600 + 7, (size_t)k * 1024, (size_t)k * 1024 - 1, (size_t)1 << 20,
                           ((size_t)1 << 20) + 1, (size_t)k * 4096 + 1}) {
            one(k, len);
            ++cases;
        }
    }
    // argument errors
    uint8_t d[4] = {1, 2, 3, 4}, t[8];
    const uint8_t *rows[2];
    EXPECT(rbc_split_rows_impl(2, d, 0, t, 8, rows, nullptr, nullptr) == -6);    // RBC_ERR_SHORT_DATA
    EXPECT(rbc_split_rows_impl(0, d, 4, t, 8, rows, nullptr, nullptr) == -10);   // RBC_ERR_INVALID_ARG
    EXPECT(rbc_split_rows_impl(2, nullptr, 4, t, 8, rows, nullptr, nullptr) == -10);
    EXPECT(rbc_split_rows_impl(2, d, 4, t, 8, nullptr, nullptr, nullptr) == -10);
    EXPECT(rbc_split_tail_bytes_impl(0, 4) == 0 && rbc_split_tail_bytes_impl(2, 0) == 0);
    EXPECT(rbc_split_rows_impl(2, d, 4, nullptr, 0, rows, nullptr, nullptr) == 0);  // no tail needed
    if (fails) {
        printf("FAIL %d\n", fails);
        return 1;
    }
    printf("ok %ld cases\n", cases);
    return 0;
}
