// wire_receive_stub.cpp -- a scalar host restatement of
// rbc_launch_unmarshal_echo (csrc/wire.hip) over host memory, the companion of
// hip_stub.cpp for csrc/wire_receive.cpp (tests/cpp/wire_receive_fuzz.cpp,
// tests/test_wire_receive_host.py).
//
// Test infrastructure only.  Written from the format description in
// include/rbc_protocol.h: the size of a canonical message as a function of its
// shard length (for the "shape from the length" rule), then a front-to-back
// parse of a pb.Message{rbc} with minimal varints, the Go-JSON request with
// its keys in struct order and no whitespace, standard base64 with '=' only as
// the final padding -- not the kernel's chunked decode.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../cleisthenes_amd/csrc/kernels.h"

namespace {

size_t varint_size(uint64_t v) {
    size_t l = 1;
    while (v >= 0x80) v >>= 7, ++l;
    return l;
}

// bytes of the canonical message carrying `groups` base64 quanta of block, a
// br_len-byte branch and the type
size_t message_size(size_t groups, size_t br_len, int type) {
    const size_t root = 44, block = 4 * groups, branch = (br_len + 2) / 3 * 4;
    // {"RootHash":"<root>","Branch":"<branch>","Block":["<block>"]}  /  ...,"Branch":null,...
    const size_t J = br_len ? 13 + root + 12 + branch + 12 + block + 3 : 13 + root + 26 + block + 3;
    const size_t R = 1 + varint_size(J) + J + (type ? 2 : 0);
    return 1 + varint_size(R) + R;
}

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

// the shard length and type a canonical message of `len` bytes would have:
// VAL before ECHO, the '=' count from the two bytes in front of the closing '"]}'
bool shape(const uint8_t *m, size_t len, size_t br_len, size_t *S, int *type) {
    for (int t = 0; t < 2; ++t)
        for (size_t g = 1; message_size(g, br_len, t) <= len; ++g) {
            if (message_size(g, br_len, t) != len) continue;
            const size_t end = len - (t ? 2 : 0) - 3;  // one past the block's base64
            const size_t pad = m[end - 1] == '=' ? (m[end - 2] == '=' ? 2 : 1) : 0;
            *S = 3 * g - pad;
            *type = t;
            return true;
        }
    return false;
}

}  // namespace

hipError_t rbc_launch_unmarshal_echo(const WireEchoArgs &a, hipStream_t) {
    const size_t bslot = (size_t)(a.depth > 1 ? a.depth : 1) * 32;
    for (int i = 0; i < a.msgs; ++i) {
        const uint32_t j = a.idx[i], in = a.inst[i];
        const uint8_t *m = a.ring + a.offs[i];
        const size_t len = a.lens[i];
        const bool empty0 = a.depth > 0 && (int)(j ^ 1u) >= a.n;
        const size_t br_len = 32u * (size_t)(a.depth - (empty0 ? 1 : 0));
        size_t S = 0;
        int type = 0;
        // 1. the shape, from the length and the leaf
        if (j >= (uint32_t)a.n || in >= (uint32_t)a.count || !shape(m, len, br_len, &S, &type) ||
            S > a.shard_pitch) {
            a.msg_status[i] = WIRE_FALLBACK;
            if (a.types) a.types[i] = 0;
            continue;
        }
        // 2. the instance's length
        if (S != (a.shard_lens ? a.shard_lens[in] : a.uniform_len)) {
            a.msg_status[i] = WIRE_OTHER_LEN;
            if (a.types) a.types[i] = (uint8_t)type;
            continue;
        }
        if (a.types) a.types[i] = (uint8_t)type;
        // 3. every byte canonical
        Fields f;
        if (!parse(m, len, f) || f.type != type || f.root.size() != 32 || f.branch.size() != br_len ||
            f.block.size() != S) {
            a.msg_status[i] = WIRE_FALLBACK;
            continue;
        }
        // 4. the instance's root
        if (memcmp(f.root.data(), a.roots + (size_t)in * 32, 32)) {
            a.msg_status[i] = WIRE_OTHER_ROOT;
            continue;
        }
        const size_t r = (size_t)in * a.n + j;
        uint8_t *slot = a.branches + r * bslot;
        if (empty0 || a.depth == 0) memset(slot, 0, 32);
        if (br_len) memcpy(slot + (empty0 ? 32 : 0), f.branch.data(), br_len);
        uint8_t *row = a.shards + r * a.shard_pitch;
        memcpy(row, f.block.data(), S);
        memset(row + S, 0, (S + 63) / 64 * 64 - S);
        a.present[r] = 1;
        a.msg_status[i] = WIRE_OK;
    }
    return hipSuccess;
}
