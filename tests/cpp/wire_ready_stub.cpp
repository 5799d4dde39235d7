// wire_ready_stub.cpp -- a scalar host restatement of rbc_launch_unmarshal_ready
// and rbc_launch_quorum (csrc/wire.hip) over host memory, the companion of
// hip_stub.cpp for csrc/wire_ready.cpp (tests/cpp/wire_ready_fuzz.cpp,
// tests/test_wire_ready_host.py).
//
// Test infrastructure only.  Written from the text of include/rbc_protocol.h:
// a front-to-back parse of a pb.Message{rbc} with minimal varints whose
// payload is the Go-JSON ReadyRequest with no whitespace and whose type is
// READY, standard base64 with '=' only as the final padding -- not the
// kernel's chunked decode -- and the four lines of the quorum rule as they
// stand there.
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

// 0x1a varint(R) { 0x0a varint(J) {"RootHash":"<base64>"} 0x10 0x02 }
bool parse_ready(const uint8_t *m, size_t len, std::vector<uint8_t> &root) {
    Cursor c{m, m + len};
    uint64_t R, J;
    if (!c.byte(0x1a) || !c.varint(&R) || R != (uint64_t)(c.e - c.p)) return false;
    if (!c.byte(0x0a) || !c.varint(&J) || J > (uint64_t)(c.e - c.p)) return false;
    Cursor j{c.p, c.p + J};
    c.p += J;
    if (!c.byte(0x10) || !c.byte(0x02) || c.p != c.e) return false;
    return j.text("{\"RootHash\":\"") && b64_string(j, root) && j.text("}") && j.p == j.e;
}

}  // namespace

hipError_t rbc_launch_unmarshal_ready(const WireReadyArgs &a, hipStream_t) {
    if (a.msg_len == 0 || a.n < 1 || a.n > 256) return hipErrorInvalidValue;
    std::vector<uint8_t> root;
    for (int m = 0; m < a.msgs; ++m) {
        const uint32_t in = a.inst[m], j = a.idx[m];
        // 1. length, instance and leaf, before a byte of the message is looked at
        if (a.lens[m] != a.msg_len || in >= (uint32_t)a.count || j >= (uint32_t)a.n) {
            a.msg_status[m] = WIRE_FALLBACK;
            continue;
        }
        // 2. every byte canonical
        if (!parse_ready(a.ring + a.offs[m], a.lens[m], root) || root.size() != 32) {
            a.msg_status[m] = WIRE_FALLBACK;
            continue;
        }
        // 3. the instance's root
        if (memcmp(root.data(), a.roots + (size_t)in * 32, 32)) {
            a.msg_status[m] = WIRE_OTHER_ROOT;
            continue;
        }
        a.ready[(size_t)in * a.n + j] = 1;
        a.msg_status[m] = WIRE_OK;
    }
    return hipSuccess;
}

hipError_t rbc_launch_quorum(const QuorumArgs &a, hipStream_t) {
    if (a.n < 1 || a.f < 0 || a.self < -1 || a.self >= a.n) return hipErrorInvalidValue;
    const int n = a.n, f = a.f;
    for (int i = 0; i < a.count; ++i) {
        uint8_t *ready = a.ready + (size_t)i * n;
        int E = 0, R = 0;
        for (int t = 0; t < n; ++t) {
            if (a.valid && a.valid[(size_t)i * n + t]) ++E;
            if (ready[t]) ++R;
        }
        const bool ok = a.status && a.status[i] == 0;
        const bool have = ok && (E >= n - f || (R >= 2 * f + 1 && E >= n - 2 * f));
        const bool amplify = R >= f + 1;
        const bool send_ready = amplify || have;
        if (send_ready && a.self >= 0 && !ready[a.self]) {
            ready[a.self] = 1;
            ++R;
        }
        const bool deliver = ok && R >= 2 * f + 1 && E >= n - 2 * f;
        a.echo_counts[i] = (uint32_t)E;
        a.ready_counts[i] = (uint32_t)R;
        a.flags[i] = (uint8_t)((E >= n - f ? QUORUM_ECHO : 0) | (amplify ? QUORUM_AMPLIFY : 0) |
                               (send_ready ? QUORUM_SEND_READY : 0) | (deliver ? QUORUM_DELIVER : 0));
    }
    return hipSuccess;
}
