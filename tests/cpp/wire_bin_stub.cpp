// wire_bin_stub.cpp -- scalar host restatements of the two binary receive
// kernels (csrc/wire.hip: unmarshal_val_bin_kernel, unmarshal_echo_bin_kernel)
// over host memory, the companion of hip_stub.cpp for
// tests/cpp/wire_bin_fuzz.cpp (tests/test_wire_bin_host.py).
//
// Test infrastructure only.  Written from the format table in
// include/rbc_protocol.h, front to back like a parser, not from the kernels'
// length-derived candidates and chunked copies: a pb.Message{rbc} with minimal
// varints, then magic, version, L, the reserved byte, S, root, branch, shard
// and nothing behind it.  Only the binary codec lives here: codec 0 is
// hipErrorNotSupported.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>

#include "../../cleisthenes_amd/csrc/kernels.h"

namespace {

struct Cursor {
    const uint8_t *p, *e;
    bool byte(uint8_t want) { return p < e && *p == want ? (++p, true) : false; }
    // a varint in its shortest form
    bool varint(uint64_t *v) {
        uint64_t r = 0;
        for (int sh = 0; sh < 35; sh += 7) {
            if (p >= e) return false;
            const uint8_t b = *p++;
            r |= (uint64_t)(b & 0x7f) << sh;
            if (!(b & 0x80)) {
                if (sh && b == 0) return false;  // a zero last byte: not minimal
                *v = r;
                return true;
            }
        }
        return false;
    }
};

struct Fields {
    int type = 0;
    size_t L = 0, S = 0;
    const uint8_t *root = nullptr, *branch = nullptr, *block = nullptr;
};

bool parse(const uint8_t *m, size_t len, Fields &f) {
    Cursor c{m, m + len};
    uint64_t R, J;
    if (!c.byte(0x1a) || !c.varint(&R) || R != (uint64_t)(c.e - c.p)) return false;
    if (!c.byte(0x0a) || !c.varint(&J) || J > (uint64_t)(c.e - c.p)) return false;
    const uint8_t *pl = c.p;
    c.p += J;
    if (c.p == c.e) f.type = 0;
    else if (c.byte(0x10) && c.byte(0x01) && c.p == c.e) f.type = 1;
    else return false;
    if (J < 40 || pl[0] != 0xB1 || pl[1] != 0x01 || pl[3] != 0x00) return false;
    f.L = pl[2];
    f.S = (size_t)pl[4] | (size_t)pl[5] << 8 | (size_t)pl[6] << 16 | (size_t)pl[7] << 24;
    if (J != 40 + 32 * f.L + f.S) return false;
    f.root = pl + 8;
    f.branch = pl + 40;
    f.block = f.branch + 32 * f.L;
    return true;
}

size_t vlen(uint64_t v) {
    size_t n = 1;
    while (v >= 0x80) v >>= 7, ++n;
    return n;
}

size_t message_bytes(size_t S, size_t L, int type) {
    const size_t J = 40 + 32 * L + S, R = 1 + vlen(J) + J + (type ? 2 : 0);
    return 1 + vlen(R) + R;
}

// the shard length a message of `total` bytes and this type has, 0 if none
size_t shard_len_of(size_t total, size_t L, int type) {
    const size_t least = message_bytes(1, L, type);
    if (total < least) return 0;
    // the overhead beyond S is that of S = 1 plus at most four more varint bytes each for R and J
    const size_t top = total - least + 1;
    for (size_t S = top; S + 10 > top && S >= 1; --S)
        if (message_bytes(S, L, type) == total) return S;
    return 0;
}

void store(uint8_t *row, uint8_t *slot, const Fields &f, bool empty0, int depth) {
    if (empty0 || depth == 0) memset(slot, 0, 32);
    if (f.L) memcpy(slot + (empty0 ? 32 : 0), f.branch, 32 * f.L);
    memcpy(row, f.block, f.S);
    memset(row + f.S, 0, (f.S + 63) / 64 * 64 - f.S);
}

}  // namespace

hipError_t rbc_launch_unmarshal_val(const WireRxArgs &a, hipStream_t) {
    if (a.codec != 1) return hipErrorNotSupported;
    const size_t bslot = (size_t)(a.depth > 1 ? a.depth : 1) * 32;
    for (int i = 0; i < a.count; ++i) {
        const uint32_t j = a.idx[i];
        const bool empty0 = a.depth > 0 && (int)(j ^ 1u) >= a.n;
        Fields f;
        const bool ok = j < (uint32_t)a.n && parse(a.msgs + a.offs[i], a.lens[i], f) &&
                        f.L == (size_t)(a.depth - (empty0 ? 1 : 0)) && f.S >= 1 && f.S <= a.row_pitch;
        a.status[i] = ok ? WIRE_OK : WIRE_FALLBACK;
        a.types[i] = ok ? (uint8_t)f.type : 0;
        a.shard_lens[i] = ok ? (uint32_t)f.S : 0;
        if (!ok) continue;
        memcpy(a.roots + (size_t)i * 32, f.root, 32);
        store(a.rows + (size_t)i * a.row_pitch, a.branches + (size_t)i * bslot, f, empty0, a.depth);
    }
    return hipSuccess;
}

hipError_t rbc_launch_unmarshal_echo(const WireEchoArgs &a, hipStream_t) {
    if (a.codec != 1) return hipErrorNotSupported;
    const size_t bslot = (size_t)(a.depth > 1 ? a.depth : 1) * 32;
    for (int m = 0; m < a.msgs; ++m) {
        const uint32_t j = a.idx[m], in = a.inst[m];
        const bool empty0 = a.depth > 0 && (int)(j ^ 1u) >= a.n;
        const size_t L = (size_t)(a.depth - (empty0 ? 1 : 0));
        if (a.types) a.types[m] = 0;
        // 1. a shape, from the length and the leaf alone: one per type at most
        size_t cand[2] = {0, 0};
        if (j < (uint32_t)a.n && in < (uint32_t)a.count && a.lens[m] <= 0x7fffffffu)
            for (int t = 0; t < 2; ++t) {
                cand[t] = shard_len_of(a.lens[m], L, t);
                if (cand[t] > a.shard_pitch) cand[t] = 0;
            }
        if (!cand[0] && !cand[1]) {
            a.msg_status[m] = WIRE_FALLBACK;
            continue;
        }
        // 2. the instance's length picks the candidate
        const size_t S = a.shard_lens ? a.shard_lens[in] : a.uniform_len;
        if (S == 0 || (cand[0] != S && cand[1] != S)) {
            a.msg_status[m] = WIRE_OTHER_LEN;
            continue;
        }
        // 3. every byte, front to back
        Fields f;
        if (!parse(a.ring + a.offs[m], a.lens[m], f) || f.L != L || f.S != S) {
            a.msg_status[m] = WIRE_FALLBACK;
            continue;
        }
        if (a.types) a.types[m] = (uint8_t)f.type;
        const size_t r = (size_t)in * a.n + j;
        // the slot is written whatever the root says (its bytes are unspecified for OTHER_ROOT)
        store(a.shards + r * a.shard_pitch, a.branches + r * bslot, f, empty0, a.depth);
        // 4. / 5.
        if (memcmp(f.root, a.roots + (size_t)in * 32, 32)) {
            a.msg_status[m] = WIRE_OTHER_ROOT;
            continue;
        }
        a.msg_status[m] = WIRE_OK;
        a.present[r] = 1;
    }
    return hipSuccess;
}
