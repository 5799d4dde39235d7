// wire_rx_stub.cpp -- a scalar host restatement of rbc_launch_unmarshal_val
// (csrc/wire.hip) over host memory, the companion of hip_stub.cpp for
// csrc/wire_rx.cpp (tests/cpp/wire_rx_fuzz.cpp, tests/test_wire_rx_host.py).
//
// Test infrastructure only.  Written from the format description in
// include/rbc_protocol.h, front to back like a parser, not from the kernel's
// length-derived layout and chunked decode: a pb.Message{rbc} with minimal
// varints, the Go-JSON request with its keys in struct order and no
// whitespace, standard base64 with '=' only as the final padding.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../cleisthenes_amd/csrc/kernels.h"

namespace {

struct Cursor {
    const uint8_t *p, *e;
    bool byte(uint8_t want) { return p < e && *p == want ? (++p, true) : false; }
    bool text(const char *s) {
        const size_t n = strlen(s);
        if ((size_t)(e - p) < n || memcmp(p, s, n)) return false;
        p += n;
        return true;
    }
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

int sextet(uint8_t c) {
    if (c >= 'A' && c <= 'Z') return c - 'A';
    if (c >= 'a' && c <= 'z') return c - 'a' + 26;
    if (c >= '0' && c <= '9') return c - '0' + 52;
    return c == '+' ? 62 : c == '/' ? 63 : -1;
}

// the base64 string up to the closing quote: whole quanta, '=' only as the
// last one or two characters; the quote is consumed
bool b64_string(Cursor &c, std::vector<uint8_t> &out) {
    const uint8_t *q = c.p;
    while (q < c.e && *q != '"') ++q;
    if (q >= c.e) return false;
    const size_t n = (size_t)(q - c.p);
    if (n % 4) return false;
    out.clear();
    for (size_t i = 0; i < n; i += 4) {
        const uint8_t *g = c.p + i;
        int pad = 0;
        if (i + 4 == n && g[3] == '=') pad = g[2] == '=' ? 2 : 1;
        uint32_t w = 0;
        for (int k = 0; k < 4; ++k) {
            int v = 0;
            if (k < 4 - pad && (v = sextet(g[k])) < 0) return false;
            w = w << 6 | (uint32_t)v;
        }
        out.push_back((uint8_t)(w >> 16));
        if (pad < 2) out.push_back((uint8_t)(w >> 8));
        if (pad < 1) out.push_back((uint8_t)w);
    }
    c.p = q + 1;
    return true;
}

struct Fields {
    int type = 0;
    std::vector<uint8_t> root, branch, block;
};

bool parse(const uint8_t *m, size_t len, Fields &f) {
    Cursor c{m, m + len};
    uint64_t R, J;
    if (!c.byte(0x1a) || !c.varint(&R) || R != (uint64_t)(c.e - c.p)) return false;
    if (!c.byte(0x0a) || !c.varint(&J) || J > (uint64_t)(c.e - c.p)) return false;
    Cursor j{c.p, c.p + J};
    c.p += J;
    if (c.p == c.e) f.type = 0;
    else if (c.byte(0x10) && c.byte(0x01) && c.p == c.e) f.type = 1;
    else return false;
    if (!j.text("{\"RootHash\":\"") || !b64_string(j, f.root) || !j.text(",\"Branch\":")) return false;
    f.branch.clear();
    if (!j.text("null") && !(j.byte('"') && b64_string(j, f.branch) && !f.branch.empty())) return false;
    return j.text(",\"Block\":[\"") && b64_string(j, f.block) && j.text("]}") && j.p == j.e;
}

}  // namespace

hipError_t rbc_launch_unmarshal_val(const WireRxArgs &a, hipStream_t) {
    const size_t bslot = (size_t)(a.depth > 1 ? a.depth : 1) * 32;
    for (int i = 0; i < a.count; ++i) {
        const uint32_t j = a.idx[i];
        const bool empty0 = a.depth > 0 && (int)(j ^ 1u) >= a.n;
        const size_t br_len = 32u * (size_t)(a.depth - (empty0 ? 1 : 0));
        Fields f;
        const bool ok = j < (uint32_t)a.n && parse(a.msgs + a.offs[i], a.lens[i], f) && f.root.size() == 32 &&
                        f.branch.size() == br_len && !f.block.empty() && f.block.size() <= a.row_pitch;
        a.status[i] = ok ? WIRE_OK : WIRE_FALLBACK;
        a.types[i] = ok ? (uint8_t)f.type : 0;
        a.shard_lens[i] = ok ? (uint32_t)f.block.size() : 0;
        if (!ok) continue;
        memcpy(a.roots + (size_t)i * 32, f.root.data(), 32);
        uint8_t *slot = a.branches + (size_t)i * bslot;
        if (empty0 || a.depth == 0) memset(slot, 0, 32);
        if (br_len) memcpy(slot + (empty0 ? 32 : 0), f.branch.data(), br_len);
        uint8_t *row = a.rows + (size_t)i * a.row_pitch;
        const size_t S = f.block.size();
        memcpy(row, f.block.data(), S);
        memset(row + S, 0, (S + 63) / 64 * 64 - S);
    }
    return hipSuccess;
}
