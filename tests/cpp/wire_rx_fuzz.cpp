// wire_rx_fuzz.cpp -- the host side of the wire receive path
// (csrc/wire_rx.cpp: rbc_dev_unmarshal_val, rbc_wire_validate), built by
// tests/test_wire_rx_host.py with ASan + UBSan from csrc/capi.cpp,
// batcher.cpp, rbc_node.cpp, wire_rx.cpp, the host-memory HIP stand-in
// tests/cpp/hip_stub.cpp and the scalar unmarshal restatement
// tests/cpp/wire_rx_stub.cpp.
//
//  1. rbc_wire_validate's argument checks: every rejected call returns
//     RBC_ERR_INVALID_ARG before any "device" work, and a good call after it
//     still works.
//  2. A seeded corpus of canonical VAL / ECHO messages (n = 7, S in {5, 64,
//     100}) under hostile mutations, one call per message with every buffer
//     sized exactly to the contract (ASan finds an overrun): status OK implies
//     that the host decoder (rbc_pb_decode_rbc + rbc_json_decode_val) accepts
//     the same bytes and every field is byte-equal; every canonical message and
//     every in-alphabet substitution off the padding is status OK.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../../include/rbc_gpu.h"
#include "../../include/rbc_protocol.h"

#ifndef RBC_HAS_WIRE_RX
#error "include/rbc_protocol.h does not declare the wire receive path"
#endif

static int fails = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            if (fails < 20) fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                          \
        }                                                                     \
    } while (0)

typedef std::vector<uint8_t> Bytes;
static const char kAlphabet[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";

static size_t rup(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct Dev {  // "device" memory of exactly `bytes` bytes
    uint8_t *p = nullptr;
    size_t bytes;
    explicit Dev(size_t n, int fill = 0xA5) : bytes(n) {
        void *v = nullptr;
        if (rbc_dev_malloc(0, n, &v) != RBC_OK) abort();
        p = (uint8_t *)v;
        memset(p, fill, n);
    }
    ~Dev() { rbc_dev_free(p); }
    Dev(const Dev &) = delete;
};

static Bytes encode(int type, const Bytes &root, const Bytes &branch, const Bytes &block) {
    Bytes json(rbc_json_encode_val(root.data(), root.size(), branch.data(), branch.size(), block.data(), block.size(),
                                   nullptr, 0));
    rbc_json_encode_val(root.data(), root.size(), branch.data(), branch.size(), block.data(), block.size(),
                        json.data(), json.size());
    Bytes msg(rbc_pb_encode_rbc(type, json.data(), json.size(), nullptr, 0));
    rbc_pb_encode_rbc(type, json.data(), json.size(), msg.data(), msg.size());
    return msg;
}

struct Geometry {
    int n, depth;
};

// One message through rbc_dev_unmarshal_val with exactly sized buffers, against the host decoder.
// Returns the status (or -1 when the call itself failed).
static int run_one(rbc_ctx *ctx, Geometry g, const Bytes &msg, uint8_t idx, uint32_t row_pitch) {
    const size_t bslot = (size_t)(g.depth > 1 ? g.depth : 1) * 32;
    Dev arena(rup(msg.size() ? msg.size() : 1, 16), 0), offs(8, 0), lens(4, 0), ix(1, 0);
    Dev rows(row_pitch), slens(4), branches(bslot), roots(32), types(1), status(4);
    if (!msg.empty()) memcpy(arena.p, msg.data(), msg.size());
    const uint32_t len = (uint32_t)msg.size();
    memcpy(lens.p, &len, 4);
    ix.p[0] = idx;
    const int rc = rbc_dev_unmarshal_val(ctx, nullptr, 1, arena.p, (const uint64_t *)offs.p, (const uint32_t *)lens.p,
                                         ix.p, rows.p, row_pitch, (uint32_t *)slens.p, branches.p, roots.p, types.p,
                                         (int32_t *)status.p);
    EXPECT(rc == RBC_OK);
    if (rc != RBC_OK) return -1;
    int32_t st;
    memcpy(&st, status.p, 4);
    EXPECT(st == RBC_WIRE_OK || st == RBC_WIRE_FALLBACK);
    if (st != RBC_WIRE_OK) return st;
    // status OK: the host decoder accepts the same bytes and returns the same fields
    int type = -1;
    const uint8_t *payload = nullptr;
    size_t plen = 0, blen = 0, klen = 0;
    Bytes root(32), branch(msg.size() + 1), block(msg.size() + 1);
    const bool host_ok = rbc_pb_decode_rbc(msg.data(), msg.size(), &type, &payload, &plen) == RBC_OK &&
                         rbc_json_decode_val(payload, plen, root.data(), branch.data(), branch.size(), &blen,
                                             block.data(), block.size(), &klen) == RBC_OK;
    EXPECT(host_ok);
    if (!host_ok) return st;
    uint32_t S;
    memcpy(&S, slens.p, 4);
    EXPECT(types.p[0] == type && (type == RBC_MSG_VAL || type == RBC_MSG_ECHO));
    EXPECT(!memcmp(roots.p, root.data(), 32));
    EXPECT(S == klen && S >= 1 && S <= row_pitch);
    if (S == klen && S <= row_pitch) {
        EXPECT(!memcmp(rows.p, block.data(), S));
        for (size_t b = S; b < rup(S, 64); ++b) EXPECT(rows.p[b] == 0);
        for (size_t b = rup(S, 64); b < row_pitch; ++b) EXPECT(rows.p[b] == 0xA5);  // the rest of the slot
    }
    const bool empty0 = g.depth > 0 && (int)(idx ^ 1u) >= g.n;
    EXPECT(blen == 32u * (size_t)(g.depth - (empty0 ? 1 : 0)));
    if (blen == 32u * (size_t)(g.depth - (empty0 ? 1 : 0))) {  // flat branch -> device form
        Bytes want(bslot, 0);
        memcpy(want.data() + (empty0 ? 32 : 0), branch.data(), blen);
        EXPECT(!memcmp(branches.p, want.data(), bslot));
    }
    return st;
}

struct Runs {  // the three base64 runs of a canonical message: [begin, end) offsets
    size_t b[3], e[3];
};
static Runs find_runs(const Bytes &m) {
    std::vector<size_t> q;
    for (size_t i = 0; i < m.size(); ++i)
        if (m[i] == '"') q.push_back(i);
    Runs r{};
    if (q.size() != 12) abort();  // "RootHash" root "Branch" branch "Block" block
    for (int k = 0; k < 3; ++k) r.b[k] = q[4 * k + 2] + 1, r.e[k] = q[4 * k + 3];
    return r;
}

static void args_checks(rbc_ctx *ctx, Geometry g) {
    std::mt19937_64 rng(7);
    const uint32_t pitch = 128;
    rbc_wire_rx *rx = nullptr;
    EXPECT(rbc_wire_rx_create(nullptr, 4, 4096, pitch, &rx) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_rx_create(ctx, 0, 4096, pitch, &rx) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_rx_create(ctx, 4, 0, pitch, &rx) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_rx_create(ctx, 4, 4096, 100, &rx) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_rx_create(ctx, 4, 4096, pitch, nullptr) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_rx_create(ctx, 4, 4096, pitch, &rx) == RBC_OK && rx);
    if (!rx) return;
    // three good ECHOs and one with whitespace, laid out at 16-byte offsets
    std::vector<Bytes> msgs;
    Bytes ring;
    uint64_t offs[5];
    uint32_t lens[5];
    uint8_t idx[5] = {0, 3, 6, 1, 0};
    for (int i = 0; i < 4; ++i) {
        const bool empty0 = (idx[i] ^ 1) >= g.n;
        Bytes root(32), br(32 * (g.depth - empty0)), blk(i == 1 ? 64 : 5 + 40 * i);
        for (Bytes *v : {&root, &br, &blk})
            for (uint8_t &b : *v) b = (uint8_t)rng();
        Bytes m = encode(RBC_MSG_ECHO, root, br, blk);
        if (i == 3) m.insert(m.begin() + (m.size() - 5), ' ');  // inside the JSON object
        offs[i] = ring.size();
        lens[i] = (uint32_t)m.size();
        ring.insert(ring.end(), m.begin(), m.end());
        ring.resize(rup(ring.size(), 16), 0);
    }
    offs[4] = offs[0], lens[4] = lens[0];
    const size_t rb = ring.size();
    Dev keep(4 * pitch);
    uint8_t verdict[4], types[4], roots[4 * 32], leaves[4 * 32], host_keep[4 * 128];
    uint32_t slens[4];
    uint64_t t = 77;
    memset(verdict, 9, sizeof verdict);
#define CALL(count, rbytes, of, ln, ix, kd, kb) \
    rbc_wire_validate(rx, count, ring.data(), rbytes, of, ln, ix, verdict, types, roots, slens, leaves, kd, kb, &t)
    uint64_t bad_offs[4] = {offs[0], offs[1] + 8, offs[2], offs[3]};
    EXPECT(CALL(4, rb, bad_offs, lens, idx, keep.p, keep.bytes) == RBC_ERR_INVALID_ARG);  // misaligned offs
    EXPECT(CALL(4, rb - 16, offs, lens, idx, keep.p, keep.bytes) == RBC_ERR_INVALID_ARG);  // past ring_bytes
    uint64_t wrap_offs[4] = {offs[0], ~(uint64_t)0 - 15, offs[2], offs[3]};
    EXPECT(CALL(4, rb, wrap_offs, lens, idx, keep.p, keep.bytes) == RBC_ERR_INVALID_ARG);  // wrap-around
    uint32_t long_lens[4] = {lens[0], lens[1], lens[2], 0xfffffff9u};
    EXPECT(CALL(4, rb, offs, long_lens, idx, keep.p, keep.bytes) == RBC_ERR_INVALID_ARG);
    uint8_t bad_idx[4] = {0, 3, (uint8_t)g.n, 1};
    EXPECT(CALL(4, rb, offs, lens, bad_idx, keep.p, keep.bytes) == RBC_ERR_INVALID_ARG);  // idx >= n
    EXPECT(CALL(4, rb, offs, lens, idx, keep.p, 4 * pitch - 1) == RBC_ERR_INVALID_ARG);   // keep_bytes too small
    EXPECT(CALL(5, rb, offs, lens, idx, keep.p, keep.bytes) == RBC_ERR_INVALID_ARG);      // count > max_msgs
    EXPECT(CALL(4, 4096 + 16, offs, lens, idx, keep.p, keep.bytes) == RBC_ERR_INVALID_ARG);  // ring > max_ring_bytes
    EXPECT(CALL(4, rb, offs, lens, idx, host_keep, sizeof host_keep) == RBC_ERR_INVALID_ARG);  // not device memory
    EXPECT(CALL(4, rb, offs, lens, idx, nullptr, keep.bytes) == RBC_ERR_INVALID_ARG);
    EXPECT(CALL(-1, rb, offs, lens, idx, keep.p, keep.bytes) == RBC_ERR_INVALID_ARG);
    EXPECT(CALL(4, rb, nullptr, lens, idx, keep.p, keep.bytes) == RBC_ERR_INVALID_ARG);
    EXPECT(t == 77);
    for (uint8_t v : verdict) EXPECT(v == 9);  // nothing was enqueued
    for (size_t b = 0; b < keep.bytes; ++b) EXPECT(keep.p[b] == 0xA5);
    // a good call still works: the stand-in's verify touches (zeroes) the verdicts, so a
    // decoded message reads 0 and a fallback 2
    EXPECT(CALL(4, rb, offs, lens, idx, keep.p, keep.bytes) == RBC_OK && t != 77 && t != 0);
    int done = 0;
    EXPECT(rbc_wire_poll(rx, t, &done) == RBC_OK && done == 1);
    EXPECT(rbc_wire_wait(rx, t) == RBC_OK);
    EXPECT(verdict[0] == 0 && verdict[1] == 0 && verdict[2] == 0 && verdict[3] == 2);
    EXPECT(slens[0] == 5 && slens[1] == 64 && slens[2] == 85 && slens[3] == 0);
    EXPECT(types[0] == RBC_MSG_ECHO);
    EXPECT(rbc_wire_wait(rx, t) == RBC_OK && rbc_wire_wait(rx, t + 1) == RBC_ERR_INVALID_ARG);
    EXPECT(CALL(0, 0, nullptr, nullptr, nullptr, nullptr, 0) == RBC_OK && t == 0);
#undef CALL
    rbc_wire_rx_destroy(rx);
    rbc_wire_rx_destroy(nullptr);
    // the device ABI's own checks
    Dev d(256);
    EXPECT(rbc_dev_unmarshal_val(ctx, nullptr, 1, d.p, (uint64_t *)d.p, (uint32_t *)d.p, d.p, d.p, 100, (uint32_t *)d.p,
                                 d.p, d.p, d.p, (int32_t *)d.p) == RBC_ERR_INVALID_ARG);  // row_pitch % 64
    EXPECT(rbc_dev_unmarshal_val(ctx, nullptr, -1, d.p, (uint64_t *)d.p, (uint32_t *)d.p, d.p, d.p, 64, (uint32_t *)d.p,
                                 d.p, d.p, d.p, (int32_t *)d.p) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_unmarshal_val(ctx, nullptr, 1, d.p, (uint64_t *)d.p, (uint32_t *)d.p, d.p, nullptr, 64,
                                 (uint32_t *)d.p, d.p, d.p, d.p, (int32_t *)d.p) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_unmarshal_val(nullptr, nullptr, 1, d.p, (uint64_t *)d.p, (uint32_t *)d.p, d.p, d.p, 64,
                                 (uint32_t *)d.p, d.p, d.p, d.p, (int32_t *)d.p) == RBC_ERR_INVALID_ARG);
    for (size_t b = 0; b < d.bytes; ++b) EXPECT(d.p[b] == 0xA5);
}

static Bytes put_varint(uint64_t v, int extra) {  // extra: redundant continuation bytes
    Bytes o;
    while (v >= 0x80) o.push_back((uint8_t)(v | 0x80)), v >>= 7;
    o.push_back((uint8_t)v);
    for (int i = 0; i < extra; ++i) o.back() |= 0x80, o.push_back(0);
    return o;
}

int main() {
    const Geometry g{7, 3};
    rbc_ctx *ctx = nullptr;
    EXPECT(rbc_ctx_create(g.n, 2, 0, &ctx) == RBC_OK);
    if (!ctx) return 2;
    args_checks(ctx, g);

    std::mt19937_64 rng(20261019);
    auto below = [&rng](size_t n) { return (size_t)(rng() % n); };
    const uint32_t row_pitch = 192;
    size_t total = 0, ok_count = 0, must_ok = 0;
    for (int base = 0; base < 42; ++base) {
        static const uint32_t kS[3] = {5, 64, 100};
        const uint32_t S = kS[base % 3];
        const uint8_t idx = (uint8_t)((base / 3) % g.n);
        const int type = (base / 21) % 2;
        const bool empty0 = (idx ^ 1) >= g.n;
        Bytes root(32), br(32 * (g.depth - empty0)), blk(S);
        for (Bytes *v : {&root, &br, &blk})
            for (uint8_t &b : *v) b = (uint8_t)rng();
        const Bytes canon = encode(type, root, br, blk);
        const Runs runs = find_runs(canon);
        auto run = [&](const Bytes &m, uint8_t ix, bool expect_ok) {
            const int st = run_one(ctx, g, m, ix, row_pitch);
            ++total;
            ok_count += st == RBC_WIRE_OK;
            if (expect_ok) {
                ++must_ok;
                EXPECT(st == RBC_WIRE_OK);
            }
        };
        run(canon, idx, true);
        // the S bound: a pitch of exactly round_up(S, 64) decodes, one 64 below falls back
        EXPECT(run_one(ctx, g, canon, idx, (uint32_t)rup(S, 64)) == RBC_WIRE_OK);
        if (S > 64) EXPECT(run_one(ctx, g, canon, idx, (uint32_t)rup(S, 64) - 64) == RBC_WIRE_FALLBACK);
        for (int rep = 0; rep < 6; ++rep) {
            const int k = (int)below(3);
            const size_t rb = runs.b[k], re = runs.e[k];
            size_t npad = 0;
            while (canon[re - 1 - npad] == '=') ++npad;
            Bytes m;
            // another alphabet character anywhere off the padding
            m = canon;
            m[rb + below(re - rb - npad)] = (uint8_t)kAlphabet[below(64)];
            run(m, idx, true);
            // the last characters before the padding too: trailing bits may be anything
            m = canon;
            m[re - npad - 1] = (uint8_t)kAlphabet[below(64)];
            run(m, idx, true);
            // a non-alphabet byte
            m = canon;
            m[rb + below(re - rb)] = (uint8_t)("-_ .,\\\x7f\x80\xff\x00@[`{"[below(14)]);
            run(m, idx, false);
            // '=' in the middle
            m = canon;
            m[rb + below(re - rb - npad)] = '=';
            run(m, idx, false);
            // a bit flip anywhere
            m = canon;
            m[below(m.size())] ^= (uint8_t)(1u << below(8));
            run(m, idx, false);
            // truncation and extension
            m = canon;
            m.resize(below(m.size()));
            run(m, idx, false);
            m = canon;
            for (size_t x = 1 + below(5); x; --x) m.push_back((uint8_t)rng());
            run(m, idx, false);
            // whitespace inserted somewhere in the JSON, a newline inside a run
            m = canon;
            m.insert(m.begin() + (long)(runs.b[0] - 13 + below(m.size() - runs.b[0] + 13)), (uint8_t)" \t\n\r"[below(4)]);
            run(m, idx, false);
            m = canon;
            m.insert(m.begin() + (long)(rb + below(re - rb)), (uint8_t)'\n');
            run(m, idx, false);
            // a wrong idx
            run(canon, (uint8_t)((idx + 1 + below(g.n - 1)) % g.n), false);
        }
        // the JSON re-wrapped: fixed lengths (whitespace, lower-cased or reordered keys, an unknown
        // key, an escape) and wrong or non-minimal varints
        const size_t j0 = runs.b[0] - 13, j1 = runs.e[2] + 3;  // the JSON object
        const std::string json(canon.begin() + (long)j0, canon.begin() + (long)j1);
        std::vector<std::string> js;
        js.push_back(" " + json);
        js.push_back(json + "\n");
        {
            std::string s = json;
            s.replace(s.find("RootHash"), 8, "roothash");
            js.push_back(s);
            s = json;
            s.replace(s.find("Block"), 5, "BLOCK");
            js.push_back(s);
            s = json;
            s.insert(s.size() - 1, ",\"Extra\":\"AAAA\"");
            js.push_back(s);
            s = json;
            s.insert(1, "\"Extra\":[1,{\"a\":null}],");
            js.push_back(s);
            s = json;
            s.replace(s.find("RootHash"), 8, "Root\\u0048ash");
            js.push_back(s);
            // Block first
            const size_t bpos = json.find(",\"Block\":");
            js.push_back("{" + json.substr(bpos + 1, json.size() - bpos - 2) + "," + json.substr(1, bpos - 1) + "}");
            // an escaped character inside the shard's base64
            s = json;
            const size_t at = runs.b[2] - j0;
            char esc[8];
            snprintf(esc, sizeof esc, "\\u%04x", (unsigned)(uint8_t)s[at]);
            s.replace(at, 1, esc);
            js.push_back(s);
            // CR / LF inside the shard's base64 (escaped: the host decoder skips them), a space after a colon
            s = json;
            s.insert(at + 4, "\\n");
            js.push_back(s);
            s = json;
            s.insert(s.find(':') + 1, " ");
            js.push_back(s);
        }
        for (const std::string &s : js) {
            Bytes m(rbc_pb_encode_rbc(type, (const uint8_t *)s.data(), s.size(), nullptr, 0));
            rbc_pb_encode_rbc(type, (const uint8_t *)s.data(), s.size(), m.data(), m.size());
            run(m, idx, false);
        }
        for (int variant = 0; variant < 6; ++variant) {
            const uint64_t J = json.size(), tb = type ? 2 : 0;
            const int extraR = variant == 0, extraJ = variant == 1;
            const uint64_t Jw = variant == 2 ? J + 1 : variant == 3 ? J - 1 : J;
            Bytes vj = put_varint(Jw, extraJ);
            const uint64_t R = 1 + vj.size() + J + tb + (variant == 4 ? 1 : 0) - (variant == 5 ? 1 : 0);
            Bytes m{0x1a}, vr = put_varint(R, extraR);
            m.insert(m.end(), vr.begin(), vr.end());
            m.push_back(0x0a);
            m.insert(m.end(), vj.begin(), vj.end());
            m.insert(m.end(), json.begin(), json.end());
            if (type) m.push_back(0x10), m.push_back((uint8_t)type);
            run(m, idx, false);
        }
        // READY type, a type field of another value, and the fields in the other order
        {
            Bytes m = canon;
            if (type) {
                m.back() = RBC_MSG_READY;
                run(m, idx, false);
                m.back() = 0x81;
                run(m, idx, false);
            }
        }
    }
    // degenerate lengths: nothing is read past a short message
    for (size_t len = 0; len < 200; ++len) {
        Bytes m(len);
        for (uint8_t &b : m) b = (uint8_t)rng();
        if (len) m[0] = 0x1a;
        EXPECT(run_one(ctx, g, m, 0, row_pitch) == RBC_WIRE_FALLBACK);
    }
    EXPECT(total > 2500 && must_ok > 500 && ok_count >= must_ok);
    rbc_ctx_destroy(ctx);
    if (fails) {
        printf("FAIL %d\n", fails);
        return 1;
    }
    printf("ok %zu messages, %zu decoded on the device path, %zu of them required\n", total, ok_count, must_ok);
    return 0;
}
