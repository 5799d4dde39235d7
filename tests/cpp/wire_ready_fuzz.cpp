// wire_ready_fuzz.cpp -- the host side of the READY path (csrc/wire_ready.cpp:
// rbc_dev_unmarshal_ready, rbc_dev_quorum, rbc_wire_quorum), built by
// tests/test_wire_ready_host.py with ASan + UBSan from csrc/capi.cpp,
// batcher.cpp, rbc_node.cpp (the host decoder), wire_ready.cpp, the
// host-memory HIP stand-in tests/cpp/hip_stub.cpp and the scalar restatement
// of the two new launchers tests/cpp/wire_ready_stub.cpp.
//
//  1. rbc_wire_quorum's argument checks: every rejected call returns
//     RBC_ERR_INVALID_ARG before any "device" work (canary outputs, the bitmap
//     and the ticket untouched), random arguments never overrun a buffer sized
//     exactly to the contract, and a good call after them still works, equals
//     the rbc_dev_* pair, accumulates over calls and re-tallies with no
//     messages.
//  2. Every single-byte mutation of a canonical READY, its truncations and
//     extensions by 1..16 bytes, and the READYs of a 31- and a 33-byte root
//     (the same length), in one rbc_dev_unmarshal_ready call over buffers sized
//     exactly to the contract: the status must be the one the host decoder
//     (rbc_pb_decode_rbc + rbc_json_decode_ready + the re-encode canonicality
//     test) gives by the documented order, the bitmap holds exactly the OK
//     slots on top of its 0 / 1 pattern, and RBC_WIRE_OK implies the host
//     decoder accepts the message as a READY of the same root.
//  3. The quorum table over every (E, R, status, own bit) at (n, f) = (4, 1),
//     (7, 2) and (4, 0), against the four lines of include/rbc_protocol.h.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../include/rbc_gpu.h"
#include "../../include/rbc_protocol.h"

#ifndef RBC_HAS_WIRE_READY
#error "include/rbc_protocol.h does not declare the READY path"
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
        if (rbc_dev_malloc(0, n ? n : 1, &v) != RBC_OK) abort();
        p = (uint8_t *)v;
        memset(p, fill, n);
    }
    ~Dev() { rbc_dev_free(p); }
    Dev(const Dev &) = delete;
    template <class T> T *as() { return reinterpret_cast<T *>(p); }
};

static Bytes encode_ready(const Bytes &root) {
    Bytes json(rbc_json_encode_ready(root.data(), root.size(), nullptr, 0));
    rbc_json_encode_ready(root.data(), root.size(), json.data(), json.size());
    Bytes msg(rbc_pb_encode_rbc(RBC_MSG_READY, json.data(), json.size(), nullptr, 0));
    rbc_pb_encode_rbc(RBC_MSG_READY, json.data(), json.size(), msg.data(), msg.size());
    return msg;
}

// What the host decoder says: a READY it accepts (root), and whether the message is canonical -- it
// re-encodes to the same bytes, but for the trailing bits of the padded last quantum, which the
// device decoder ignores as the host decoder does (include/rbc_protocol.h).
struct Host {
    bool accepted = false, canonical = false;
    Bytes root;
};
static Host host_decode(const Bytes &msg) {
    Host h;
    int type = -1;
    const uint8_t *payload = nullptr;
    size_t plen = 0;
    Bytes root(32);
    if (msg.empty() || rbc_pb_decode_rbc(msg.data(), msg.size(), &type, &payload, &plen) != RBC_OK) return h;
    if (type != RBC_MSG_READY || rbc_json_decode_ready(payload, plen, root.data()) != RBC_OK) return h;
    h.accepted = true;
    h.root = root;
    const Bytes again = encode_ready(root);
    if (again.size() != msg.size()) return h;
    size_t e = again.size();  // one past the base64: in front of '"}' and the two bytes of the type field
    while (e > 0 && again[e - 1] != '=') --e;
    const size_t free_at = e >= 2 ? e - 2 : (size_t)-1;  // the last character in front of the one '='
    for (size_t at = 0; at < msg.size(); ++at)
        if (again[at] != msg[at] && at != free_at) return h;
    h.canonical = true;
    return h;
}

struct Batch {
    std::vector<Bytes> msgs;
    std::vector<uint32_t> inst;
    std::vector<uint8_t> idx;
    void add(const Bytes &m, uint32_t in, uint8_t ix) { msgs.push_back(m), inst.push_back(in), idx.push_back(ix); }
};

// All of a batch through one rbc_dev_unmarshal_ready call, every buffer sized exactly.
static std::vector<int32_t> run(rbc_ctx *ctx, int n, int count, const Batch &b, const Bytes &roots, Bytes &ready) {
    const size_t mm = b.msgs.size();
    std::vector<uint64_t> offs(mm);
    std::vector<uint32_t> lens(mm);
    size_t at = 0;
    for (size_t m = 0; m < mm; ++m) {
        offs[m] = at;
        lens[m] = (uint32_t)b.msgs[m].size();
        at += rup(b.msgs[m].size(), 16);
    }
    Dev arena(at, 0), doffs(mm * 8), dlens(mm * 4), dinst(mm * 4), didx(mm), droots((size_t)count * 32),
        dready((size_t)count * n), dstatus(mm * 4);
    for (size_t m = 0; m < mm; ++m)
        if (lens[m]) memcpy(arena.p + offs[m], b.msgs[m].data(), lens[m]);
    memcpy(doffs.p, offs.data(), mm * 8);
    memcpy(dlens.p, lens.data(), mm * 4);
    memcpy(dinst.p, b.inst.data(), mm * 4);
    memcpy(didx.p, b.idx.data(), mm);
    memcpy(droots.p, roots.data(), (size_t)count * 32);
    memcpy(dready.p, ready.data(), (size_t)count * n);
    const int rc = rbc_dev_unmarshal_ready(ctx, nullptr, count, (int)mm, arena.p, doffs.as<uint64_t>(),
                                           dlens.as<uint32_t>(), dinst.as<uint32_t>(), didx.p, droots.p, dready.p,
                                           dstatus.as<int32_t>());
    EXPECT(rc == RBC_OK);
    std::vector<int32_t> st(mm);
    memcpy(st.data(), dstatus.p, mm * 4);
    memcpy(ready.data(), dready.p, (size_t)count * n);
    return st;
}

static size_t corpus(rbc_ctx *ctx, int n) {
    std::mt19937_64 rng(20261019);
    const int count = 61;  // a prime: the messages walk over every (instance, leaf)
    Bytes roots((size_t)count * 32);
    Bytes A(32), B(32);
    for (Bytes *v : {&A, &B})
        for (uint8_t &x : *v) x = (uint8_t)rng();
    for (int i = 0; i < count; ++i) memcpy(roots.data() + 32 * i, (i % 5 == 0 ? B : A).data(), 32);  // every fifth: another root
    const Bytes canon = encode_ready(A);
    EXPECT(host_decode(canon).canonical);
    Batch b;
    auto add = [&](const Bytes &m) {
        const size_t q = b.msgs.size();
        b.add(m, (uint32_t)(q % count), (uint8_t)((q / count) % n));
    };
    for (int rep = 0; rep < 12; ++rep) add(canon);  // instances 0, 5 and 10 collect for the other root
    for (size_t at = 0; at < canon.size(); ++at)  // every single-byte mutation
        for (int v = 0; v < 256; ++v) {
            if (v == canon[at]) continue;
            Bytes m = canon;
            m[at] = (uint8_t)v;
            add(m);
        }
    for (size_t d = 1; d <= 16; ++d) {  // truncation and extension
        Bytes m(canon.begin(), canon.end() - (long)d);
        add(m);
        m = canon;
        for (size_t x = 0; x < d; ++x) m.push_back((uint8_t)rng());
        add(m);
    }
    for (size_t len : {31u, 33u}) {  // as many characters, the same total length
        Bytes r(len);
        for (uint8_t &x : r) x = (uint8_t)rng();
        const Bytes m = encode_ready(r);
        EXPECT(m.size() == canon.size());
        EXPECT(!host_decode(m).accepted);
        add(m);
    }
    add(Bytes());  // an empty message
    const size_t plain = b.msgs.size();
    // an instance or a leaf out of range: nothing of the message is looked at, nothing is written
    b.add(canon, (uint32_t)count, 0);
    b.add(canon, 0xffffffffu, 0);
    b.add(canon, 1, (uint8_t)n);
    b.add(canon, 1, 255);
    Bytes ready((size_t)count * n), want;
    for (uint8_t &x : ready) x = (uint8_t)(rng() % 4 == 0);  // a pattern of 0 and 1
    want = ready;
    const std::vector<int32_t> st = run(ctx, n, count, b, roots, ready);
    size_t seen[3] = {0, 0, 0};
    for (size_t q = 0; q < b.msgs.size(); ++q) {
        const Host h = host_decode(b.msgs[q]);
        int expect = RBC_WIRE_FALLBACK;
        if (q < plain && h.canonical)
            expect = memcmp(h.root.data(), roots.data() + 32 * b.inst[q], 32) ? RBC_WIRE_OTHER_ROOT : RBC_WIRE_OK;
        EXPECT(st[q] == expect);
        if (st[q] == RBC_WIRE_OK) {
            EXPECT(h.accepted && q < plain && !memcmp(h.root.data(), roots.data() + 32 * b.inst[q], 32));
            if (q < plain) want[(size_t)b.inst[q] * n + b.idx[q]] = 1;
        }
        if (h.canonical && q < plain) EXPECT(st[q] == RBC_WIRE_OK || st[q] == RBC_WIRE_OTHER_ROOT);
        if (st[q] >= 0 && st[q] < 3) ++seen[st[q]];
    }
    EXPECT(ready == want);
    EXPECT(seen[RBC_WIRE_OK] >= 9 &&seen[RBC_WIRE_OTHER_ROOT] > 1000 && seen[RBC_WIRE_FALLBACK] > 1000);
    EXPECT(st[0] == RBC_WIRE_OTHER_ROOT);  // instance 0 collects for the other root
    return b.msgs.size();
}

// the four lines of the header over counts
struct Verdict {
    uint32_t E, R;
    uint8_t flags;
    bool own_written;
};
static Verdict model(int n, int f, int E, int R, bool known, int st, int self, bool own_bit) {
    const bool ok = known && st == RBC_OK;
    const bool have = ok && (E >= n - f || (R >= 2 * f + 1 && E >= n - 2 * f));
    const bool amplify = R >= f + 1;
    const bool send_ready = amplify || have;
    bool wrote = false;
    if (send_ready && self >= 0 && !own_bit) wrote = true, R += 1;
    const bool deliver = ok && R >= 2 * f + 1 && E >= n - 2 * f;
    return {(uint32_t)E, (uint32_t)R,
            (uint8_t)((E >= n - f ? RBC_QUORUM_ECHO : 0) | (amplify ? RBC_QUORUM_AMPLIFY : 0) |
                      (send_ready ? RBC_QUORUM_SEND_READY : 0) | (deliver ? RBC_QUORUM_DELIVER : 0)),
            wrote};
}

static size_t quorum_table(int n, int f) {
    rbc_ctx *ctx = nullptr;
    EXPECT(rbc_ctx_create(n, f, 0, &ctx) == RBC_OK);
    if (!ctx) return 0;
    std::mt19937_64 rng(n * 100 + f);
    size_t rows = 0;
    static const int kStatus[3] = {RBC_OK, RBC_ERR_TOO_FEW_SHARDS, RBC_ERR_ROOT_MISMATCH};
    // self: none, a member whose bit is clear, a member whose bit is set
    for (int mode = 0; mode < 3; ++mode)
        for (int known = 0; known < 2; ++known)
            for (int with_valid = 0; with_valid < 2; ++with_valid) {
                struct Row {
                    int E, R, st;
                };
                std::vector<Row> table;
                for (int E = 0; E <= n; ++E)
                    for (int R = (mode == 2 ? 1 : 0); R <= (mode == 1 ? n - 1 : n); ++R)
                        for (int s = 0; s < 3; ++s) table.push_back({E, R, kStatus[s]});
                const size_t count = table.size();
                const int self = mode == 0 ? -1 : (int)(rng() % n);
                Dev valid(count * n, 0), ready(count * n, 0), status(count * 4), ec(count * 4), rcn(count * 4),
                    fl(count);
                for (size_t i = 0; i < count; ++i) {
                    // E and R members at random places; the own bit as the mode says
                    std::vector<int> order(n);
                    for (int t = 0; t < n; ++t) order[t] = t;
                    for (int t = n - 1; t > 0; --t) std::swap(order[t], order[rng() % (t + 1)]);
                    for (int t = 0; t < table[i].E; ++t) valid.p[i * n + order[t]] = (uint8_t)(1 + rng() % 255);
                    for (int t = n - 1; t > 0; --t) std::swap(order[t], order[rng() % (t + 1)]);
                    if (mode) {  // self last (clear) or first (set)
                        const size_t at = std::find(order.begin(), order.end(), self) - order.begin();
                        std::swap(order[at], order[mode == 1 ? n - 1 : 0]);
                    }
                    for (int t = 0; t < table[i].R; ++t) ready.p[i * n + order[t]] = (uint8_t)(1 + rng() % 255);
                    memcpy(status.p + 4 * i, &table[i].st, 4);
                }
                const Bytes before(ready.p, ready.p + count * n);
                const int rc = rbc_dev_quorum(ctx, nullptr, (int)count, with_valid ? valid.p : nullptr, ready.p,
                                              known ? status.as<int32_t>() : nullptr, self, ec.as<uint32_t>(),
                                              rcn.as<uint32_t>(), fl.p);
                EXPECT(rc == RBC_OK);
                for (size_t i = 0; i < count; ++i) {
                    const Verdict v = model(n, f, with_valid ? table[i].E : 0, table[i].R, known, table[i].st, self,
                                            mode == 2);
                    EXPECT(ec.as<uint32_t>()[i] == v.E && rcn.as<uint32_t>()[i] == v.R && fl.p[i] == v.flags);
                    for (int t = 0; t < n; ++t)  // only the own bit is ever written
                        EXPECT(ready.p[i * n + t] == (v.own_written && t == self ? 1 : before[i * n + t]));
                    ++rows;
                }
            }
    // the ABI's own checks
    Dev d(64);
    uint32_t *d32 = d.as<uint32_t>();
    EXPECT(rbc_dev_quorum(nullptr, nullptr, 1, d.p, d.p, d.as<int32_t>(), -1, d32, d32, d.p) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_quorum(ctx, nullptr, -1, d.p, d.p, d.as<int32_t>(), -1, d32, d32, d.p) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_quorum(ctx, nullptr, 1, d.p, nullptr, d.as<int32_t>(), -1, d32, d32, d.p) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_quorum(ctx, nullptr, 1, d.p, d.p, d.as<int32_t>(), -1, nullptr, d32, d.p) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_quorum(ctx, nullptr, 1, d.p, d.p, d.as<int32_t>(), -1, d32, nullptr, d.p) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_quorum(ctx, nullptr, 1, d.p, d.p, d.as<int32_t>(), -1, d32, d32, nullptr) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_quorum(ctx, nullptr, 1, d.p, d.p, d.as<int32_t>(), n, d32, d32, d.p) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_quorum(ctx, nullptr, 1, d.p, d.p, d.as<int32_t>(), -2, d32, d32, d.p) == RBC_ERR_INVALID_ARG);
    for (size_t b = 0; b < d.bytes; ++b) EXPECT(d.p[b] == kCanary);
    rbc_ctx_destroy(ctx);
    return rows;
}

// Host outputs of one rbc_wire_quorum call, sized exactly to the contract and canary-filled.
struct Outs {
    Bytes ready, verdict, flags;
    std::vector<uint32_t> ec, rcn;
    uint64_t ticket = 77;
    Outs(size_t count, size_t msgs, size_t n)
        : ready(count * n, 9), verdict(msgs, 9), flags(count, 9), ec(count, 99), rcn(count, 99) {}
    bool untouched() const {
        for (const Bytes *v : {&ready, &verdict, &flags})
            for (uint8_t b : *v)
                if (b != 9) return false;
        for (const std::vector<uint32_t> *v : {&ec, &rcn})
            for (uint32_t s : *v)
                if (s != 99) return false;
        return ticket == 77;
    }
};

static void args_checks(rbc_ctx *ctx, int n, int f) {
    std::mt19937_64 rng(7);
    rbc_wire_quorum_handle *q = nullptr;
    EXPECT(rbc_wire_quorum_create(nullptr, 2, 5, 4096, &q) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_quorum_create(ctx, 0, 5, 4096, &q) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_quorum_create(ctx, 2, 0, 4096, &q) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_quorum_create(ctx, 2, 5, 0, &q) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_quorum_create(ctx, 2, 5, 4096, nullptr) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_quorum_create(ctx, 2, 5, 4096, &q) == RBC_OK && q);
    if (!q) return;
    // instance 0: READYs from 0, 3 and (twice) 5; instance 1: one with whitespace.  16-byte offsets.
    Bytes ring, roots(2 * 32);
    for (uint8_t &b : roots) b = (uint8_t)rng();
    uint64_t offs[6];
    uint32_t lens[6], inst[6] = {0, 0, 0, 1, 0, 0};
    uint8_t idx[6] = {0, 3, 5, 1, 5, 0};
    for (int i = 0; i < 5; ++i) {
        Bytes m = encode_ready(Bytes(roots.begin() + 32 * inst[i], roots.begin() + 32 * inst[i] + 32));
        if (i == 3) m.insert(m.end() - 3, ' ');  // in front of the closing brace
        offs[i] = ring.size();
        lens[i] = (uint32_t)m.size();
        ring.insert(ring.end(), m.begin(), m.end());
        ring.resize(rup(ring.size(), 16), 0);
    }
    offs[5] = offs[0], lens[5] = lens[0];
    const size_t rb = ring.size();
    const Bytes valid((size_t)2 * n, 1);
    const int32_t status[2] = {RBC_OK, RBC_OK};
    Outs o(2, 5, n);
#define CALL(count, msgs, rng_, rbytes, of, ln, in, ix, rt, va, st, self, rd, vd, ec, rc, fl, tk) \
    rbc_wire_quorum(q, count, msgs, rng_, rbytes, of, ln, in, ix, rt, va, st, self, rd, vd, ec, rc, fl, tk)
#define BAD(...)                                          \
    do {                                                  \
        EXPECT(CALL(__VA_ARGS__) == RBC_ERR_INVALID_ARG); \
        EXPECT(o.untouched());                            \
    } while (0)
    uint8_t *rd = o.ready.data(), *vd = o.verdict.data(), *fl = o.flags.data();
    uint32_t *ec = o.ec.data(), *rc = o.rcn.data();
    const uint8_t *rg = ring.data(), *rt = roots.data(), *va = valid.data();
    // null pointers
    BAD(2, 5, nullptr, rb, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);
    BAD(2, 5, rg, rb, nullptr, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);
    BAD(2, 5, rg, rb, offs, nullptr, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);
    BAD(2, 5, rg, rb, offs, lens, nullptr, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);
    BAD(2, 5, rg, rb, offs, lens, inst, nullptr, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);
    BAD(2, 5, rg, rb, offs, lens, inst, idx, nullptr, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);
    BAD(2, 5, rg, rb, offs, lens, inst, idx, rt, va, status, 2, nullptr, vd, ec, rc, fl, &o.ticket);
    BAD(2, 5, rg, rb, offs, lens, inst, idx, rt, va, status, 2, rd, nullptr, ec, rc, fl, &o.ticket);
    BAD(2, 5, rg, rb, offs, lens, inst, idx, rt, va, status, 2, rd, vd, nullptr, rc, fl, &o.ticket);
    BAD(2, 5, rg, rb, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, nullptr, fl, &o.ticket);
    BAD(2, 5, rg, rb, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, nullptr, &o.ticket);
    BAD(2, 5, rg, rb, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, nullptr);
    BAD(2, 5, rg, 0, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);
    EXPECT(rbc_wire_quorum(nullptr, 2, 5, rg, rb, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl,
                           &o.ticket) == RBC_ERR_INVALID_ARG);
    // the limits of the handle, and self
    BAD(3, 5, rg, rb, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);  // count > max_count
    BAD(2, 6, rg, rb, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);  // msgs > max_msgs
    BAD(2, 5, rg, 4096 + 16, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);
    BAD(-1, 5, rg, rb, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);
    BAD(2, -1, rg, rb, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);
    BAD(0, 5, rg, rb, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);  // messages of no instance
    BAD(2, 5, rg, rb, offs, lens, inst, idx, rt, va, status, n, rd, vd, ec, rc, fl, &o.ticket);  // self >= n
    BAD(2, 5, rg, rb, offs, lens, inst, idx, rt, va, status, -2, rd, vd, ec, rc, fl, &o.ticket);
    BAD(2, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, va, status, n, rd, nullptr, ec, rc, fl, &o.ticket);
    // the messages
    uint64_t bad_offs[5] = {offs[0], offs[1] + 8, offs[2], offs[3], offs[4]};
    BAD(2, 5, rg, rb, bad_offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);  // misaligned offs
    BAD(2, 5, rg, rb - 16, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);  // past ring_bytes
    uint64_t wrap_offs[5] = {offs[0], ~(uint64_t)0 - 15, offs[2], offs[3], offs[4]};
    BAD(2, 5, rg, rb, wrap_offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);  // wrap-around
    uint32_t long_lens[5] = {lens[0], lens[1], lens[2], 0xfffffff9u, lens[4]};
    BAD(2, 5, rg, rb, offs, long_lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);
    uint32_t bad_inst[5] = {0, 0, 2, 1, 0};
    BAD(2, 5, rg, rb, offs, lens, bad_inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);  // inst >= count
    uint32_t huge_inst[5] = {0, 0xffffffffu, 0, 1, 0};
    BAD(2, 5, rg, rb, offs, lens, huge_inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);
    BAD(1, 5, rg, rb, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);  // inst 1 of count 1
    uint8_t bad_idx[5] = {0, 3, (uint8_t)n, 1, 5};
    BAD(2, 5, rg, rb, offs, lens, inst, bad_idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket);  // idx >= n
    // random arguments: whatever the answer, nothing overruns (ASan), and a rejected call writes nothing
    for (int rep = 0; rep < 300; ++rep) {
        uint64_t ro[5];
        uint32_t rl[5], ri[5];
        uint8_t rx[5];
        for (int m = 0; m < 5; ++m) {
            ro[m] = rng() % 3 ? offs[m] : (rng() % 2 ? rng() : rng() % (rb + 64));
            rl[m] = rng() % 3 ? lens[m] : (uint32_t)(rng() % 2 ? rng() : rng() % 100);
            ri[m] = rng() % 3 ? inst[m] : (uint32_t)(rng() % 2 ? rng() : rng() % 3);
            rx[m] = rng() % 3 ? idx[m] : (uint8_t)(rng() % 9);
        }
        const int rcount = rng() % 8 ? 2 : (int)(rng() % 4), rmsgs = rng() % 8 ? 5 : (int)(rng() % 7);
        const size_t rrb = rng() % 4 ? rb : (size_t)(rng() % (rb + 1));
        const int rself = rng() % 4 ? 2 : (int)(rng() % (n + 3)) - 2;
        Outs t(2, 5, n);
        const int got = rbc_wire_quorum(q, rcount, rmsgs, rg, rrb, ro, rl, ri, rx, rt, rng() % 2 ? va : nullptr,
                                        rng() % 2 ? status : nullptr, rself, t.ready.data(), t.verdict.data(),
                                        t.ec.data(), t.rcn.data(), t.flags.data(), &t.ticket);
        EXPECT(got == RBC_OK || got == RBC_ERR_INVALID_ARG);
        if (got == RBC_OK) EXPECT(rbc_wire_quorum_wait(q, t.ticket) == RBC_OK);
        else EXPECT(t.untouched());
    }
    // a good call still works: duplicates allowed, the whitespace READY falls back, the own bit is set
    memset(rd, 0, o.ready.size());
    EXPECT(CALL(2, 5, rg, rb, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &o.ticket) == RBC_OK);
    EXPECT(o.ticket != 77 && o.ticket != 0);
    int done = 0;
    EXPECT(rbc_wire_quorum_poll(q, o.ticket, &done) == RBC_OK && done == 1);
    EXPECT(rbc_wire_quorum_wait(q, o.ticket) == RBC_OK);
    EXPECT(vd[0] == RBC_WIRE_OK && vd[1] == RBC_WIRE_OK && vd[2] == RBC_WIRE_OK && vd[3] == RBC_WIRE_FALLBACK &&
           vd[4] == RBC_WIRE_OK);
    Bytes want((size_t)2 * n, 0);
    want[0] = want[3] = want[5] = 1;
    want[2] = want[n + 2] = 1;  // all n ECHOs valid and status OK: both instances send READY, so self = 2 is set
    EXPECT(o.ready == want);
    EXPECT(ec[0] == (uint32_t)n && ec[1] == (uint32_t)n && rc[0] == 4 && rc[1] == 1);
    const uint8_t all = RBC_QUORUM_ECHO | RBC_QUORUM_AMPLIFY | RBC_QUORUM_SEND_READY;
    EXPECT(fl[0] == (all | (4 >= 2 * f + 1 ? RBC_QUORUM_DELIVER : 0)));
    EXPECT(fl[1] == (RBC_QUORUM_ECHO | RBC_QUORUM_SEND_READY | (1 >= 2 * f + 1 ? RBC_QUORUM_DELIVER : 0)));
    EXPECT(rbc_wire_quorum_wait(q, o.ticket) == RBC_OK);
    EXPECT(rbc_wire_quorum_wait(q, o.ticket + 1) == RBC_ERR_INVALID_ARG);
    // the bitmap accumulates: one more READY for instance 1 in a second call, on top of what came back
    uint64_t t2 = 0;
    uint32_t inst1[1] = {1};
    uint8_t idx1[1] = {6};
    uint8_t v1[1] = {9};
    const Bytes r1 = encode_ready(Bytes(roots.begin() + 32, roots.end()));
    Bytes ring1(rup(r1.size(), 16), 0);
    memcpy(ring1.data(), r1.data(), r1.size());
    uint64_t off1[1] = {0};
    uint32_t len1[1] = {(uint32_t)r1.size()};
    EXPECT(rbc_wire_quorum(q, 2, 1, ring1.data(), ring1.size(), off1, len1, inst1, idx1, rt, va, status, 2, rd, v1, ec,
                           rc, fl, &t2) == RBC_OK && rbc_wire_quorum_wait(q, t2) == RBC_OK);
    want[n + 6] = 1;
    EXPECT(v1[0] == RBC_WIRE_OK && o.ready == want && rc[0] == 4 && rc[1] == 2);
    // no messages at all: only the tally (without valid and status nothing is known: E = 0, no DELIVER)
    EXPECT(rbc_wire_quorum(q, 2, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, -1, rd,
                           nullptr, ec, rc, fl, &t2) == RBC_OK && rbc_wire_quorum_wait(q, t2) == RBC_OK);
    EXPECT(o.ready == want && ec[0] == 0 && ec[1] == 0 && rc[0] == 4 && rc[1] == 2);
    EXPECT(fl[0] == (4 >= f + 1 ? RBC_QUORUM_AMPLIFY | RBC_QUORUM_SEND_READY : 0));
    // no instances at all
    EXPECT(rbc_wire_quorum(q, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, -1,
                           nullptr, nullptr, nullptr, nullptr, nullptr, &t2) == RBC_OK && t2 == 0);
    // a second submission completes the one before it
    Outs o2(2, 5, n);
    memset(o2.ready.data(), 0, o2.ready.size());
    uint64_t ta = 0, tb = 0;
    EXPECT(CALL(2, 5, rg, rb, offs, lens, inst, idx, rt, va, status, 2, rd, vd, ec, rc, fl, &ta) == RBC_OK);
    EXPECT(rbc_wire_quorum(q, 2, 5, rg, rb, offs, lens, inst, idx, rt, va, status, -1, o2.ready.data(),
                           o2.verdict.data(), o2.ec.data(), o2.rcn.data(), o2.flags.data(), &tb) == RBC_OK);
    EXPECT(tb == ta + 1 && rbc_wire_quorum_wait(q, tb) == RBC_OK && rbc_wire_quorum_wait(q, ta) == RBC_OK);
    EXPECT(o2.verdict[3] == RBC_WIRE_FALLBACK && o2.rcn[0] == 3 && o2.ready[2] == 0);
#undef BAD
#undef CALL
    rbc_wire_quorum_destroy(q);
    rbc_wire_quorum_destroy(nullptr);
    // the device ABI's own checks
    Dev d(256);
    uint64_t *d64 = d.as<uint64_t>();
    uint32_t *d32 = d.as<uint32_t>();
    int32_t *i32 = d.as<int32_t>();
    EXPECT(rbc_dev_unmarshal_ready(nullptr, nullptr, 1, 1, d.p, d64, d32, d32, d.p, d.p, d.p, i32) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_unmarshal_ready(ctx, nullptr, -1, 1, d.p, d64, d32, d32, d.p, d.p, d.p, i32) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_unmarshal_ready(ctx, nullptr, 1, -1, d.p, d64, d32, d32, d.p, d.p, d.p, i32) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_unmarshal_ready(ctx, nullptr, 0, 1, d.p, d64, d32, d32, d.p, d.p, d.p, i32) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_unmarshal_ready(ctx, nullptr, 1, 1, nullptr, d64, d32, d32, d.p, d.p, d.p, i32) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_unmarshal_ready(ctx, nullptr, 1, 1, d.p, d64, d32, d32, d.p, d.p, nullptr, i32) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_unmarshal_ready(ctx, nullptr, 1, 1, d.p, d64, d32, d32, d.p, d.p, d.p, nullptr) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_unmarshal_ready(ctx, nullptr, 1, 1, d.p + 8, d64, d32, d32, d.p, d.p, d.p, i32) ==
           RBC_ERR_INVALID_ARG);  // ring not 16-byte aligned
    EXPECT(rbc_dev_unmarshal_ready(ctx, nullptr, 1, 1, d.p, d64, d32, d32, d.p, d.p + 8, d.p, i32) ==
           RBC_ERR_INVALID_ARG);  // roots not 16-byte aligned
    for (size_t b = 0; b < d.bytes; ++b) EXPECT(d.p[b] == kCanary);
}

int main() {
    const int n = 7, f = 2;
    rbc_ctx *ctx = nullptr;
    EXPECT(rbc_ctx_create(n, f, 0, &ctx) == RBC_OK);
    if (!ctx) return 2;
    args_checks(ctx, n, f);
    const size_t total = corpus(ctx, n);
    EXPECT(total > 16000);
    // the READY is the same under the binary payload codec
    EXPECT(rbc_ctx_set_wire_codec(ctx, RBC_WIRE_CODEC_BINARY) == RBC_OK);
    EXPECT(corpus(ctx, n) == total);
    rbc_ctx_destroy(ctx);
    size_t rows = 0;
    rows += quorum_table(4, 1);
    rows += quorum_table(7, 2);
    rows += quorum_table(4, 0);
    EXPECT(rows > 3000);
    if (fails) {
        printf("FAIL %d\n", fails);
        return 1;
    }
    printf("ok %zu messages, %zu quorum rows\n", total, rows);
    return 0;
}
