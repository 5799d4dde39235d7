// wire_bin_fuzz.cpp -- the host side of the binary VAL / ECHO payload codec
// (RBC_HAS_WIRE_BINARY), built by tests/test_wire_bin_host.py with ASan + UBSan
// from csrc/capi.cpp, batcher.cpp, rbc_node.cpp (the host codec), wire_rx.cpp,
// wire_receive.cpp, the host-memory HIP stand-in tests/cpp/hip_stub.cpp and
// tests/cpp/wire_bin_stub.cpp, the scalar restatement of the two binary
// receive kernels.  A stand-alone program with its own main.
//
//  1. rbc_bin_decode_val over random and truncated payloads, in buffers of
//     exactly the payload's size; the size query; rbc_payload_decode_val's
//     dispatch.
//  2. A corpus of valid messages for n in {4, 5, 7, 16} under mutation -- every
//     single-byte substitution in the first hdr + 40 bytes and the last 4,
//     lengths truncated and extended by 1..3, totals no message has, the JSON
//     form, a wrong idx -- one rbc_dev_unmarshal_val call per message in a
//     binary-mode context, every ring and output buffer sized exactly to the
//     contract.  Status OK implies that rbc_pb_decode_rbc + rbc_bin_decode_val
//     accept the bytes with byte-equal fields; and every message the host
//     accepts whose bytes equal the re-encoding of its fields, whose L is the
//     leaf's and whose S is in 1..pitch is OK.  No exceptions either way.
//  3. The same corpus at n = 7 through rbc_dev_unmarshal_echo under three
//     instance settings, by the documented status order.
//  4. rbc_wire_validate / rbc_wire_receive in binary mode: a rejected call
//     enqueues nothing and a good call after it works; a JSON-mode context's
//     call is refused by the stand-in (it owns the binary codec only).
// The binary marshal is covered on the GPU: hip_stub.cpp owns that launcher.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../include/rbc_gpu.h"
#include "../../include/rbc_protocol.h"

#ifndef RBC_HAS_WIRE_BINARY
#error "include/rbc_protocol.h does not declare the binary payload codec"
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
static const uint8_t kCanary = 0xA5;

static size_t rup(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct Dev {  // "device" memory of exactly `bytes` bytes
    uint8_t *p = nullptr;
    size_t bytes;
    explicit Dev(size_t n, int fill = kCanary) : bytes(n) {
        void *v = nullptr;
        if (rbc_dev_malloc(0, n, &v) != RBC_OK) abort();
        p = (uint8_t *)v;
        memset(p, fill, n);
    }
    ~Dev() { rbc_dev_free(p); }
    Dev(const Dev &) = delete;
};

struct Geometry {
    int n, depth;
    size_t flat(uint8_t idx) const { return (size_t)(depth - ((depth > 0 && (int)(idx ^ 1u) >= n) ? 1 : 0)); }
};

static Bytes wrap(int type, const Bytes &payload) {
    Bytes msg(rbc_pb_encode_rbc(type, payload.data(), payload.size(), nullptr, 0));
    rbc_pb_encode_rbc(type, payload.data(), payload.size(), msg.data(), msg.size());
    return msg;
}

static Bytes bin_payload(const Bytes &root, const Bytes &branch, const Bytes &block) {
    Bytes p(rbc_bin_encode_val(root.data(), root.size(), branch.data(), branch.size(), block.data(), block.size(),
                               nullptr, 0));
    rbc_bin_encode_val(root.data(), root.size(), branch.data(), branch.size(), block.data(), block.size(), p.data(),
                       p.size());
    return p;
}

static Bytes json_payload(const Bytes &root, const Bytes &branch, const Bytes &block) {
    Bytes p(rbc_json_encode_val(root.data(), root.size(), branch.data(), branch.size(), block.data(), block.size(),
                                nullptr, 0));
    rbc_json_encode_val(root.data(), root.size(), branch.data(), branch.size(), block.data(), block.size(), p.data(),
                        p.size());
    return p;
}

// What the host decoder says about a message from leaf idx.
struct Host {
    bool accepted = false;   // rbc_pb_decode_rbc + rbc_bin_decode_val take it
    bool canonical = false;  // and: VAL / ECHO, its bytes are the re-encoding, L is the leaf's, 1 <= S <= pitch
    int type = 0;
    Bytes root, branch, block;
};
static Host host_decode(Geometry g, const Bytes &msg, uint8_t idx, size_t pitch) {
    Host h;
    int type = -1;
    const uint8_t *payload = nullptr;
    size_t plen = 0, blen = 0, klen = 0;
    if (msg.empty() || rbc_pb_decode_rbc(msg.data(), msg.size(), &type, &payload, &plen) != RBC_OK) return h;
    Bytes root(32), branch(msg.size() + 1), block(msg.size() + 1);
    if (rbc_bin_decode_val(payload, plen, root.data(), branch.data(), branch.size(), &blen, block.data(),
                           block.size(), &klen) != RBC_OK)
        return h;
    branch.resize(blen);
    block.resize(klen);
    h.accepted = true;
    h.type = type;
    h.root = root, h.branch = branch, h.block = block;
    h.canonical = (type == RBC_MSG_VAL || type == RBC_MSG_ECHO) && idx < g.n &&
                  wrap(type, bin_payload(root, branch, block)) == msg && blen == 32 * g.flat(idx) && klen >= 1 &&
                  klen <= pitch;
    return h;
}

// ---- 1. the host decoder ---------------------------------------------------
static void decoder_checks(std::mt19937_64 &rng) {
    uint8_t root[32];
    size_t bl = 0, kl = 0;
    EXPECT(rbc_bin_decode_val(nullptr, 0, root, nullptr, 0, &bl, nullptr, 0, &kl) == RBC_ERR_PROTOCOL);
    EXPECT(rbc_bin_decode_val(nullptr, 4, root, nullptr, 0, &bl, nullptr, 0, &kl) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_bin_encode_val(root, 31, nullptr, 0, nullptr, 0, nullptr, 0) == 0);   // root_len != 32
    EXPECT(rbc_bin_encode_val(root, 32, root, 31, nullptr, 0, nullptr, 0) == 0);     // branch_len % 32
    EXPECT(rbc_bin_encode_val(root, 32, nullptr, 0, nullptr, 0, nullptr, 0) == 40);  // S = 0 is allowed here
    for (int rep = 0; rep < 4000; ++rep) {
        const size_t L = rng() % 9, S = rng() % 3 ? rng() % 70 : rng() % 1100;
        Bytes r(32), b(32 * L), k(S);
        for (Bytes *v : {&r, &b, &k})
            for (uint8_t &x : *v) x = (uint8_t)rng();
        const Bytes good = bin_payload(r, b, k);
        EXPECT(good.size() == 40 + 32 * L + S);
        // heap copies of exactly the payload's size: a read past the end is an ASan report
        auto decode = [&](const Bytes &p, Bytes &ro, Bytes &bo, Bytes &ko) {
            uint8_t *q = (uint8_t *)malloc(p.size() ? p.size() : 1);
            if (!p.empty()) memcpy(q, p.data(), p.size());
            ro.assign(32, 0);
            size_t bn = 0, kn = 0;
            int rc = rbc_bin_decode_val(q, p.size(), ro.data(), nullptr, 0, &bn, nullptr, 0, &kn);  // the size query
            if (rc == RBC_OK || rc == RBC_ERR_INVALID_ARG) {
                EXPECT((rc == RBC_OK) == (bn == 0 && kn == 0));
                bo.assign(bn, 0), ko.assign(kn, 0);
                rc = rbc_bin_decode_val(q, p.size(), ro.data(), bo.data(), bn, &bn, ko.data(), kn, &kn);
                EXPECT(rc == RBC_OK && bn == bo.size() && kn == ko.size());
                if (kn) {  // a buffer one byte short: the lengths, nothing written past it
                    Bytes ks(kn - 1);
                    size_t b2 = 0, k2 = 0;
                    EXPECT(rbc_bin_decode_val(q, p.size(), ro.data(), bo.data(), bn, &b2, ks.data(), kn - 1, &k2) ==
                           RBC_ERR_INVALID_ARG && b2 == bn && k2 == kn);
                }
            }
            Bytes r2(32), b2(p.size() + 1), k2(p.size() + 1);
            size_t bn2 = 0, kn2 = 0;
            EXPECT(rbc_payload_decode_val(q, p.size(), r2.data(), b2.data(), b2.size(), &bn2, k2.data(), k2.size(),
                                          &kn2) == (rc == RBC_OK ? RBC_OK : RBC_ERR_PROTOCOL));
            free(q);
            return rc;
        };
        Bytes ro, bo, ko;
        EXPECT(decode(good, ro, bo, ko) == RBC_OK && ro == r && bo == b && ko == k);
        Bytes m = good;
        m.resize(rng() % good.size());  // truncated anywhere
        EXPECT(decode(m, ro, bo, ko) == RBC_ERR_PROTOCOL);
        m = good;
        m.push_back((uint8_t)rng());  // a byte behind the shard
        EXPECT(decode(m, ro, bo, ko) == RBC_ERR_PROTOCOL);
        for (int at : {0, 1, 3}) {  // magic, version, the reserved byte
            m = good;
            m[at] ^= (uint8_t)(1u << (rng() % 8));
            EXPECT(decode(m, ro, bo, ko) == RBC_ERR_PROTOCOL);
        }
        m = good;
        m[2 + rng() % 6] ^= (uint8_t)(1u << (rng() % 8));  // L or S: the length no longer adds up
        EXPECT(decode(m, ro, bo, ko) == RBC_ERR_PROTOCOL);
        Bytes noise(rng() % 120);
        for (uint8_t &x : noise) x = (uint8_t)rng();
        if (!noise.empty() && rng() % 2) noise[0] = RBC_BIN_MAGIC;
        (void)decode(noise, ro, bo, ko);  // whatever it says, it stays inside the payload
        // the JSON form through the dispatcher
        if (S) {
            const Bytes js = json_payload(r, b, k);
            Bytes r2(32), b2(b.size() + 1), k2(k.size());
            size_t bn = 0, kn = 0;
            EXPECT(rbc_payload_decode_val(js.data(), js.size(), r2.data(), b2.data(), b2.size(), &bn, k2.data(),
                                          k2.size(), &kn) == RBC_OK && r2 == r && bn == b.size() && k2 == k);
            EXPECT(rbc_bin_decode_val(js.data(), js.size(), r2.data(), b2.data(), b2.size(), &bn, k2.data(), k2.size(),
                                      &kn) == RBC_ERR_PROTOCOL);
            EXPECT(rbc_json_decode_val(good.data(), good.size(), r2.data(), b2.data(), b2.size(), &bn, k2.data(),
                                       k2.size(), &kn) == RBC_ERR_PROTOCOL);
        }
    }
}

// ---- 2. one message through rbc_dev_unmarshal_val --------------------------
static size_t n_ok = 0, n_runs = 0;
static void run_val(rbc_ctx *ctx, Geometry g, const Bytes &msg, uint8_t idx, uint32_t pitch) {
    const Host h = host_decode(g, msg, idx, pitch);
    const size_t bslot = (size_t)(g.depth > 1 ? g.depth : 1) * 32;
    Dev arena(rup(msg.size() ? msg.size() : 1, 16), 0), offs(8, 0), lens(4, 0), ix(1, 0);
    Dev rows(pitch), slens(4), branches(bslot), roots(32), types(1), status(4);
    if (!msg.empty()) memcpy(arena.p, msg.data(), msg.size());
    const uint32_t len = (uint32_t)msg.size();
    memcpy(lens.p, &len, 4);
    ix.p[0] = idx;
    const int rc = rbc_dev_unmarshal_val(ctx, nullptr, 1, arena.p, (const uint64_t *)offs.p, (const uint32_t *)lens.p,
                                         ix.p, rows.p, pitch, (uint32_t *)slens.p, branches.p, roots.p, types.p,
                                         (int32_t *)status.p);
    EXPECT(rc == RBC_OK);
    ++n_runs;
    if (rc != RBC_OK) return;
    int32_t st;
    uint32_t S;
    memcpy(&st, status.p, 4);
    memcpy(&S, slens.p, 4);
    EXPECT(st == (h.canonical ? RBC_WIRE_OK : RBC_WIRE_FALLBACK));  // both implications, no exceptions
    if (st != RBC_WIRE_OK) {
        EXPECT(S == 0);
        return;
    }
    ++n_ok;
    EXPECT(h.accepted);
    if (!h.accepted) return;
    EXPECT(types.p[0] == h.type && S == h.block.size() && !memcmp(roots.p, h.root.data(), 32));
    EXPECT(!memcmp(rows.p, h.block.data(), h.block.size()));
    for (size_t b = S; b < rup(S, 64); ++b) EXPECT(rows.p[b] == 0);
    for (size_t b = rup(S, 64); b < pitch; ++b) EXPECT(rows.p[b] == kCanary);
    Bytes want(bslot, 0);
    if (!h.canonical) return;  // already counted as a failure above
    memcpy(want.data() + (g.flat(idx) < (size_t)g.depth ? 32 : 0), h.branch.data(), h.branch.size());
    EXPECT(!memcmp(branches.p, want.data(), bslot));
}

// ---- 3. one message through rbc_dev_unmarshal_echo -------------------------
enum Setting { OWN = 0, OTHER_ROOT = 1, OTHER_LEN = 2 };
static size_t seen[4] = {0, 0, 0, 0};
static void run_echo(rbc_ctx *ctx, Geometry g, const Bytes &msg, uint8_t idx, uint32_t pitch, Setting setting) {
    const Host h = host_decode(g, msg, idx, pitch);
    const int count = 2;
    const uint32_t in = 1;
    const size_t n = (size_t)g.n, bslot = (size_t)(g.depth > 1 ? g.depth : 1) * 32;
    Dev arena(rup(msg.size() ? msg.size() : 1, 16), 0), offs(8, 0), lens(4, 0), inst(4, 0), ix(1, 0);
    Dev roots(count * 32, 0x11), slens(count * 4, 0);
    Dev shards(count * n * pitch), branches(count * n * bslot), present(count * n), status(4), types(1);
    if (!msg.empty()) memcpy(arena.p, msg.data(), msg.size());
    const uint32_t len = (uint32_t)msg.size();
    memcpy(lens.p, &len, 4);
    memcpy(inst.p, &in, 4);
    ix.p[0] = idx;
    uint32_t want_len[2] = {7, h.canonical ? (uint32_t)h.block.size() : 64u};
    if (h.canonical) memcpy(roots.p + 32, h.root.data(), 32);
    if (setting == OTHER_ROOT) roots.p[32 + 31] ^= 0x40;
    // never two off: (S, ECHO) and (S + 2, VAL) share a total, and the instance's length picks the candidate
    if (setting == OTHER_LEN) want_len[1] = want_len[1] == 1 ? 2 : want_len[1] - 1;
    memcpy(slens.p, want_len, sizeof want_len);
    const int rc = rbc_dev_unmarshal_echo(ctx, nullptr, count, 1, arena.p, (const uint64_t *)offs.p,
                                          (const uint32_t *)lens.p, (const uint32_t *)inst.p, ix.p, roots.p,
                                          (const uint32_t *)slens.p, 0, shards.p, pitch, branches.p, present.p,
                                          (int32_t *)status.p, types.p);
    EXPECT(rc == RBC_OK);
    ++n_runs;
    if (rc != RBC_OK) return;
    int32_t st;
    memcpy(&st, status.p, 4);
    if (st >= 0 && st < 4) ++seen[st];
    if (h.canonical) {  // the documented order, over the host decoder
        const int want = h.block.size() != want_len[1] ? RBC_WIRE_OTHER_LEN
                         : setting == OTHER_ROOT       ? RBC_WIRE_OTHER_ROOT
                                                       : RBC_WIRE_OK;
        EXPECT(st == want);
    } else {
        EXPECT(st == RBC_WIRE_FALLBACK || st == RBC_WIRE_OTHER_LEN);  // by its length alone
    }
    const size_t r = idx < g.n ? in * n + idx : (size_t)-1;
    const bool slot_free = st == RBC_WIRE_OTHER_LEN || r == (size_t)-1;
    for (size_t q = 0; q < count * n; ++q) {
        if (q == r && !slot_free) continue;
        bool intact = present.p[q] == kCanary;
        for (size_t b = 0; b < pitch && intact; ++b) intact = shards.p[q * pitch + b] == kCanary;
        for (size_t b = 0; b < bslot && intact; ++b) intact = branches.p[q * bslot + b] == kCanary;
        EXPECT(intact);
    }
    if (st != RBC_WIRE_OK) {
        if (r != (size_t)-1) EXPECT(present.p[r] == kCanary);
        return;
    }
    if (!h.canonical) return;  // already counted as a failure above
    const size_t S = h.block.size();
    EXPECT(present.p[r] == 1 && types.p[0] == h.type);
    const uint8_t *row = shards.p + r * pitch;
    EXPECT(!memcmp(row, h.block.data(), S));
    for (size_t b = S; b < rup(S, 64); ++b) EXPECT(row[b] == 0);
    for (size_t b = rup(S, 64); b < pitch; ++b) EXPECT(row[b] == kCanary);
    Bytes want(bslot, 0);
    memcpy(want.data() + (g.flat(idx) < (size_t)g.depth ? 32 : 0), h.branch.data(), h.branch.size());
    EXPECT(!memcmp(branches.p + r * bslot, want.data(), bslot));
}

static size_t header_len(const Bytes &m) {  // 0x1a varint(R) 0x0a varint(J)
    size_t p = 1;
    while (m[p] & 0x80) ++p;
    p += 2;
    while (m[p] & 0x80) ++p;
    return p + 1;
}

template <class F>
static void corpus(Geometry g, std::mt19937_64 &rng, F &&run) {
    static const uint32_t kS[4] = {1, 5, 64, 100};
    for (int base = 0; base < 8; ++base) {
        const uint32_t S = kS[base % 4];
        const uint8_t idx = (uint8_t)(base < 4 ? (base * 5) % g.n : g.n - 1 - (base % 2));
        const int type = (base / 2) % 2;
        Bytes root(32), br(32 * g.flat(idx)), blk(S);
        for (Bytes *v : {&root, &br, &blk})
            for (uint8_t &b : *v) b = (uint8_t)rng();
        const Bytes canon = wrap(type, bin_payload(root, br, blk));
        run(canon, idx);
        const size_t hdr = header_len(canon);
        // every single-byte substitution in the first hdr + 40 bytes and the last 4
        for (size_t at = 0; at < canon.size(); ++at) {
            if (at >= hdr + 40 && at + 4 < canon.size()) continue;
            for (int v = 0; v < 256; ++v) {
                if (v == canon[at]) continue;
                if (base >= 2 && at >= hdr + 8 && at < hdr + 40 && v % 16) continue;  // the root: any byte is as good
                Bytes m = canon;
                m[at] = (uint8_t)v;
                run(m, idx);
            }
        }
        for (size_t k = 1; k <= 3; ++k) {  // lengths off by a little
            Bytes m(canon.begin(), canon.end() - (long)k);
            run(m, idx);
            m = canon;
            for (size_t x = 0; x < k; ++x) m.push_back((uint8_t)rng());
            run(m, idx);
            m = canon;
            m.resize(canon.size() + k, 0);
            run(m, idx);
        }
        for (int j = 0; j < g.n; ++j)  // a wrong idx (a leaf with a branch of the same length decodes: any bytes prove later)
            if (j != idx) run(canon, (uint8_t)j);
        run(wrap(type, json_payload(root, br, blk)), idx);  // the JSON form in a binary-mode context
        run(wrap(type, bin_payload(root, br, Bytes())), idx);  // S = 0: the host takes it, the device does not
        run(wrap(RBC_MSG_READY, bin_payload(root, br, blk)), idx);
        {  // a branch of another length, well-formed
            Bytes br2(br.size() + 32, 7);
            run(wrap(type, bin_payload(root, br2, blk)), idx);
        }
    }
    for (size_t total : {(size_t)130, (size_t)16387, (size_t)0, (size_t)1, (size_t)39, (size_t)45, (size_t)60}) {
        Bytes m(total);  // totals no message has, or below the smallest
        for (uint8_t &b : m) b = (uint8_t)rng();
        if (total) m[0] = 0x1a;
        run(m, 0);
    }
}

// ---- 4. the one-call entry points in binary mode ---------------------------
static void one_call_checks(rbc_ctx *ctx, rbc_ctx *json_ctx, Geometry g, std::mt19937_64 &rng) {
    const uint32_t pitch = 128;
    int kk = 0, pp = 0, dd = 0;
    EXPECT(rbc_ctx_params(ctx, &kk, &pp, &dd) == RBC_OK && kk + pp == g.n);
    const size_t n = (size_t)g.n, k = (size_t)kk;
    Bytes ring, roots(2 * 32);
    for (uint8_t &b : roots) b = (uint8_t)rng();
    uint64_t offs[4];
    uint32_t lens[4], inst[4] = {0, 0, 0, 1};
    uint8_t idx[4] = {0, 3, 6, 1};
    const size_t slens[2] = {45, 64};
    for (int i = 0; i < 4; ++i) {
        Bytes root(roots.begin() + 32 * inst[i], roots.begin() + 32 * inst[i] + 32), br(32 * g.flat(idx[i])),
            blk(i == 2 ? 46 : slens[inst[i]]);
        for (Bytes *v : {&br, &blk})
            for (uint8_t &b : *v) b = (uint8_t)rng();
        Bytes m = wrap(RBC_MSG_ECHO, i == 3 ? json_payload(root, br, blk) : bin_payload(root, br, blk));
        offs[i] = ring.size();
        lens[i] = (uint32_t)m.size();
        ring.insert(ring.end(), m.begin(), m.end());
        ring.resize(rup(ring.size(), 16), 0);
    }
    const size_t rb = ring.size(), vp = k * 64;
    // rbc_wire_receive
    rbc_wire_receiver *rcv = nullptr;
    EXPECT(rbc_wire_receiver_create(ctx, 2, 4, 4096, pitch, &rcv) == RBC_OK && rcv);
    if (rcv) {
        Bytes verdict(4, 9), types(4, 9), valid(2 * n, 9), values(2 * vp, 9), digests(64, 9);
        int32_t status[2] = {99, 99};
        uint64_t t = 77;
        auto untouched = [&] {
            for (const Bytes *v : {&verdict, &types, &valid, &values, &digests})
                for (uint8_t b : *v)
                    if (b != 9) return false;
            return status[0] == 99 && status[1] == 99 && t == 77;
        };
#define RCV(count, msgs, rbytes, of, ix, sl)                                                                   \
    rbc_wire_receive(rcv, count, msgs, ring.data(), rbytes, of, lens, inst, ix, roots.data(), sl, verdict.data(), \
                     types.data(), valid.data(), values.data(), vp, digests.data(), status, &t)
        uint64_t bad_offs[4] = {offs[0], offs[1] + 8, offs[2], offs[3]};
        uint8_t bad_idx[4] = {0, 3, (uint8_t)g.n, 1};
        const size_t long_len[2] = {pitch + 1, 64};
        EXPECT(RCV(2, 4, rb, bad_offs, idx, slens) == RBC_ERR_INVALID_ARG && untouched());
        EXPECT(RCV(2, 4, rb - 16, offs, idx, slens) == RBC_ERR_INVALID_ARG && untouched());
        EXPECT(RCV(2, 4, rb, offs, bad_idx, slens) == RBC_ERR_INVALID_ARG && untouched());
        EXPECT(RCV(2, 4, rb, offs, idx, long_len) == RBC_ERR_INVALID_ARG && untouched());
        EXPECT(RCV(3, 4, rb, offs, idx, slens) == RBC_ERR_INVALID_ARG && untouched());
        EXPECT(RCV(2, 5, rb, offs, idx, slens) == RBC_ERR_INVALID_ARG && untouched());
        // a good call still works.  The stand-in's verify zeroes valid[]: a decoded message reads 0,
        // another length 3, and the JSON message 2 or 3 by its length alone
        EXPECT(RCV(2, 4, rb, offs, idx, slens) == RBC_OK && t != 77 && t != 0);
        EXPECT(rbc_wire_receive_wait(rcv, t) == RBC_OK);
        EXPECT(verdict[0] == 0 && verdict[1] == 0 && verdict[2] == 3 && (verdict[3] == 2 || verdict[3] == 3));
        EXPECT(types[0] == RBC_MSG_ECHO);
#undef RCV
        rbc_wire_receiver_destroy(rcv);
    }
    // rbc_wire_validate
    rbc_wire_rx *rx = nullptr;
    EXPECT(rbc_wire_rx_create(ctx, 4, 4096, pitch, &rx) == RBC_OK && rx);
    if (rx) {
        Dev keep(4 * pitch);
        uint8_t verdict[4], types[4], vroots[4 * 32], leaves[4 * 32];
        uint32_t sl[4];
        uint64_t t = 77;
#define RXV(count, rbytes, of, ix, kb) \
    rbc_wire_validate(rx, count, ring.data(), rbytes, of, lens, ix, verdict, types, vroots, sl, leaves, keep.p, kb, &t)
        uint64_t bad_offs[4] = {offs[0], offs[1] + 8, offs[2], offs[3]};
        uint8_t bad_idx[4] = {0, 3, (uint8_t)g.n, 1};
        EXPECT(RXV(4, rb, bad_offs, idx, keep.bytes) == RBC_ERR_INVALID_ARG);
        EXPECT(RXV(4, rb - 16, offs, idx, keep.bytes) == RBC_ERR_INVALID_ARG);
        EXPECT(RXV(4, rb, offs, bad_idx, keep.bytes) == RBC_ERR_INVALID_ARG);
        EXPECT(RXV(4, rb, offs, idx, 4 * pitch - 1) == RBC_ERR_INVALID_ARG);
        EXPECT(RXV(5, rb, offs, idx, keep.bytes) == RBC_ERR_INVALID_ARG);
        EXPECT(t == 77);
        for (size_t b = 0; b < keep.bytes; ++b) EXPECT(keep.p[b] == kCanary);  // nothing was enqueued
        EXPECT(RXV(4, rb, offs, idx, keep.bytes) == RBC_OK && t != 77 && t != 0);
        EXPECT(rbc_wire_wait(rx, t) == RBC_OK);
        EXPECT(verdict[0] != 2 && verdict[1] != 2 && verdict[2] != 2 && verdict[3] == 2);  // the JSON one falls back
        EXPECT(sl[0] == 45 && sl[2] == 46 && !memcmp(vroots, roots.data(), 32));
#undef RXV
        rbc_wire_rx_destroy(rx);
    }
    // the switch itself
    int codec = -1;
    EXPECT(rbc_ctx_wire_codec(json_ctx, &codec) == RBC_OK && codec == RBC_WIRE_CODEC_JSON);  // the default
    EXPECT(rbc_ctx_wire_codec(ctx, &codec) == RBC_OK && codec == RBC_WIRE_CODEC_BINARY);
    EXPECT(rbc_ctx_set_wire_codec(ctx, 2) == RBC_ERR_INVALID_ARG && rbc_ctx_set_wire_codec(nullptr, 1) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_ctx_wire_codec(ctx, nullptr) == RBC_ERR_INVALID_ARG && rbc_ctx_wire_codec(nullptr, &codec) == RBC_ERR_INVALID_ARG);
    {  // a JSON-mode call reaches the launcher with codec 0, which this stand-in refuses
        Dev d(256, 0);
        EXPECT(rbc_dev_unmarshal_val(json_ctx, nullptr, 1, d.p, (const uint64_t *)d.p, (const uint32_t *)d.p, d.p, d.p,
                                     64, (uint32_t *)d.p, d.p, d.p, d.p, (int32_t *)d.p) == RBC_ERR_DEVICE);
    }
}

int main() {
    std::mt19937_64 rng(20261019);
    decoder_checks(rng);
    static const Geometry kG[4] = {{4, 2}, {5, 3}, {7, 3}, {16, 4}};
    for (const Geometry &g : kG) {
        rbc_ctx *ctx = nullptr;
        EXPECT(rbc_ctx_create(g.n, (g.n - 1) / 3, 0, &ctx) == RBC_OK);
        if (!ctx) return 2;
        EXPECT(rbc_ctx_set_wire_codec(ctx, RBC_WIRE_CODEC_BINARY) == RBC_OK);
        corpus(g, rng, [&](const Bytes &m, uint8_t idx) { run_val(ctx, g, m, idx, 128); });
        if (g.n == 7) {
            corpus(g, rng, [&](const Bytes &m, uint8_t idx) {
                for (Setting s : {OWN, OTHER_ROOT, OTHER_LEN}) run_echo(ctx, g, m, idx, 128, s);
            });
            rbc_ctx *json_ctx = nullptr;
            EXPECT(rbc_ctx_create(g.n, 2, 0, &json_ctx) == RBC_OK);
            if (json_ctx) one_call_checks(ctx, json_ctx, g, rng);
            rbc_ctx_destroy(json_ctx);
        }
        rbc_ctx_destroy(ctx);
    }
    EXPECT(n_runs > 100000 && n_ok > 10000);
    EXPECT(seen[RBC_WIRE_OK] > 1000 && seen[RBC_WIRE_FALLBACK] > 1000 && seen[RBC_WIRE_OTHER_ROOT] > 1000 &&
           seen[RBC_WIRE_OTHER_LEN] > 1000);
    if (fails) {
        printf("FAIL %d\n", fails);
        return 1;
    }
    printf("ok %zu runs: %zu decoded by rbc_dev_unmarshal_val; echo %zu decoded, %zu fallback, %zu other root, "
           "%zu other length\n", n_runs, n_ok, seen[0], seen[1], seen[2], seen[3]);
    return 0;
}
