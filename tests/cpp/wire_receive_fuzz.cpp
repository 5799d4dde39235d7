// wire_receive_fuzz.cpp -- the host side of the wire receiver
// (csrc/wire_receive.cpp: rbc_dev_unmarshal_echo, rbc_wire_receive), built by
// tests/test_wire_receive_host.py with ASan + UBSan from csrc/capi.cpp,
// batcher.cpp, rbc_node.cpp (the host decoder), wire_receive.cpp, the
// host-memory HIP stand-in tests/cpp/hip_stub.cpp and the scalar restatement
// of the new kernel tests/cpp/wire_receive_stub.cpp.
//
//  1. rbc_wire_receive's argument checks: every rejected call returns
//     RBC_ERR_INVALID_ARG before any "device" work (canary outputs and the
//     ticket untouched), random arguments never overrun a buffer sized exactly
//     to the contract, and a good call after them still works.
//  2. A seeded corpus of canonical VAL / ECHO messages (n = 7, S in {5, 64,
//     100}) under hostile mutations, one rbc_dev_unmarshal_echo call per
//     message and per instance setting (its root and length, another root,
//     another length), every buffer sized exactly to the contract: the status
//     must be the one the host decoder (rbc_pb_decode_rbc + rbc_json_decode_val
//     + the re-encode canonicality test) gives by the documented order, status
//     OK means byte-equal fields at the message's slot, and no byte outside
//     the slot changes.
// hip_stub.cpp's verify and interpolate launchers only touch their outputs,
// so values are not checked here.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../../include/rbc_gpu.h"
#include "../../include/rbc_protocol.h"

#ifndef RBC_HAS_WIRE_RECEIVE
#error "include/rbc_protocol.h does not declare the wire receiver"
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

// What the host decoder says about a message from leaf idx: canonical (decodes, re-encodes to the
// same bytes, VAL or ECHO, a 32-byte root, the branch length of the leaf, a non-empty block) or not.
struct Host {
    bool canonical = false;
    int type = 0;
    Bytes root, branch, block;
};
static Host host_decode(Geometry g, const Bytes &msg, uint8_t idx) {
    Host h;
    int type = -1;
    const uint8_t *payload = nullptr;
    size_t plen = 0, blen = 0, klen = 0;
    Bytes root(32), branch(msg.size() + 1), block(msg.size() + 1);
    if (msg.empty() || rbc_pb_decode_rbc(msg.data(), msg.size(), &type, &payload, &plen) != RBC_OK) return h;
    if (rbc_json_decode_val(payload, plen, root.data(), branch.data(), branch.size(), &blen, block.data(),
                            block.size(), &klen) != RBC_OK)
        return h;
    branch.resize(blen);
    block.resize(klen);
    const bool empty0 = g.depth > 0 && (int)(idx ^ 1u) >= g.n;
    if ((type != RBC_MSG_VAL && type != RBC_MSG_ECHO) || idx >= g.n || klen == 0 ||
        blen != 32u * (size_t)(g.depth - (empty0 ? 1 : 0)))
        return h;
    // canonical: the re-encoding is the message itself -- but for the trailing bits of a padded last
    // quantum, which the device decoder ignores as the host decoder does (include/rbc_protocol.h)
    const Bytes again = encode(type, root, branch, block);
    if (again.size() != msg.size()) return h;
    if (again != msg) {
        const Runs runs = find_runs(again);
        for (size_t at = 0; at < msg.size(); ++at) {
            if (again[at] == msg[at]) continue;
            bool last_of_padded = false;
            for (int k = 0; k < 3; ++k)
                last_of_padded |= again[runs.e[k] - 1] == '=' &&
                                  at == runs.e[k] - 2 - (again[runs.e[k] - 2] == '=' ? 1 : 0);
            if (!last_of_padded) return h;
        }
    }
    h.canonical = true;
    h.type = type;
    h.root = root, h.branch = branch, h.block = block;
    return h;
}

enum Setting { OWN = 0, OTHER_ROOT = 1, OTHER_LEN = 2 };

// One message through rbc_dev_unmarshal_echo as instance 1 of 2, with exactly sized buffers.
// Returns the status (or -1 when the call itself failed).
static int run_one(rbc_ctx *ctx, Geometry g, const Bytes &msg, uint8_t idx, uint32_t pitch, const Host &h,
                   Setting setting) {
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
    // the instance's root and length: the message's own, unless the setting says otherwise
    uint32_t want_len[2] = {7, h.canonical ? (uint32_t)h.block.size() : 64u};
    if (h.canonical) memcpy(roots.p + 32, h.root.data(), 32);
    if (setting == OTHER_ROOT) roots.p[32 + 31] ^= 0x40;
    if (setting == OTHER_LEN) want_len[1] = want_len[1] == 5 ? 6 : want_len[1] - 1;
    memcpy(slens.p, want_len, sizeof want_len);
    const int rc = rbc_dev_unmarshal_echo(ctx, nullptr, count, 1, arena.p, (const uint64_t *)offs.p,
                                          (const uint32_t *)lens.p, (const uint32_t *)inst.p, ix.p, roots.p,
                                          (const uint32_t *)slens.p, 0, shards.p, pitch, branches.p, present.p,
                                          (int32_t *)status.p, types.p);
    EXPECT(rc == RBC_OK);
    if (rc != RBC_OK) return -1;
    int32_t st;
    memcpy(&st, status.p, 4);
    // the documented order, over the host decoder
    if (h.canonical && h.block.size() <= pitch) {
        const int want = h.block.size() != want_len[1] ? RBC_WIRE_OTHER_LEN
                         : setting == OTHER_ROOT       ? RBC_WIRE_OTHER_ROOT
                                                       : RBC_WIRE_OK;
        EXPECT(st == want);
    } else {
        EXPECT(st == RBC_WIRE_FALLBACK || st == RBC_WIRE_OTHER_LEN);  // by its length alone
    }
    // nothing outside the message's own slot changes; for OTHER_LEN (and a shapeless message) nothing at all
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
        return st;
    }
    if (!h.canonical) return st;  // already counted as a failure above
    const size_t S = h.block.size();
    EXPECT(present.p[r] == 1 && types.p[0] == h.type);
    const uint8_t *row = shards.p + r * pitch;
    EXPECT(!memcmp(row, h.block.data(), S));
    for (size_t b = S; b < rup(S, 64); ++b) EXPECT(row[b] == 0);
    for (size_t b = rup(S, 64); b < pitch; ++b) EXPECT(row[b] == kCanary);  // the rest of the slot
    const bool empty0 = g.depth > 0 && (int)(idx ^ 1u) >= g.n;
    Bytes want(bslot, 0);
    memcpy(want.data() + (empty0 ? 32 : 0), h.branch.data(), h.branch.size());
    EXPECT(!memcmp(branches.p + r * bslot, want.data(), bslot));
    return st;
}

// Host outputs of one rbc_wire_receive call, sized exactly to the contract and canary-filled.
struct Outs {
    Bytes verdict, types, valid, values, digests;
    std::vector<int32_t> status;
    uint64_t ticket = 77;
    Outs(size_t count, size_t msgs, size_t n, size_t value_pitch)
        : verdict(msgs, 9), types(msgs, 9), valid(count * n, 9), values(count * value_pitch, 9),
          digests(count * 32, 9), status(count, 99) {}
    bool untouched() const {
        for (const Bytes *v : {&verdict, &types, &valid, &values, &digests})
            for (uint8_t b : *v)
                if (b != 9) return false;
        for (int32_t s : status)
            if (s != 99) return false;
        return ticket == 77;
    }
};

static void args_checks(rbc_ctx *ctx, Geometry g) {
    std::mt19937_64 rng(7);
    const uint32_t pitch = 128;
    int kk = 0, pp = 0, dd = 0;
    EXPECT(rbc_ctx_params(ctx, &kk, &pp, &dd) == RBC_OK && kk + pp == g.n && dd == g.depth);
    const size_t n = (size_t)g.n, k = (size_t)kk;
    rbc_wire_receiver *rcv = nullptr;
    EXPECT(rbc_wire_receiver_create(nullptr, 2, 4, 4096, pitch, &rcv) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_receiver_create(ctx, 0, 4, 4096, pitch, &rcv) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_receiver_create(ctx, 2, 0, 4096, pitch, &rcv) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_receiver_create(ctx, 2, 4, 0, pitch, &rcv) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_receiver_create(ctx, 2, 4, 4096, 100, &rcv) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_receiver_create(ctx, 2, 4, 4096, pitch, nullptr) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_wire_receiver_create(ctx, 2, 4, 4096, pitch, &rcv) == RBC_OK && rcv);
    if (!rcv) return;
    // instance 0 (S = 45): two good ECHOs and one of another length; instance 1 (S = 64): one with
    // whitespace.  16-byte offsets.
    Bytes ring, roots(2 * 32);
    for (uint8_t &b : roots) b = (uint8_t)rng();
    uint64_t offs[5];
    uint32_t lens[5], inst[5] = {0, 0, 0, 1, 0};
    uint8_t idx[5] = {0, 3, 6, 1, 0};
    const size_t slens[2] = {45, 64};
    for (int i = 0; i < 4; ++i) {
        const bool empty0 = (idx[i] ^ 1) >= g.n;
        Bytes root(roots.begin() + 32 * inst[i], roots.begin() + 32 * inst[i] + 32), br(32 * (g.depth - empty0)),
            blk(i == 2 ? 46 : slens[inst[i]]);
        for (Bytes *v : {&br, &blk})
            for (uint8_t &b : *v) b = (uint8_t)rng();
        Bytes m = encode(RBC_MSG_ECHO, root, br, blk);
        if (i == 3) m.insert(m.begin() + (m.size() - 5), ' ');  // inside the JSON object
        offs[i] = ring.size();
        lens[i] = (uint32_t)m.size();
        ring.insert(ring.end(), m.begin(), m.end());
        ring.resize(rup(ring.size(), 16), 0);
    }
    offs[4] = offs[0], lens[4] = lens[0];
    const size_t rb = ring.size(), vp = k * 64;
    Outs o(2, 4, n, vp);
#define CALL(count, msgs, rng_, rbytes, of, ln, in, ix, rt, sl, vd, va, vl, vpitch, st, tk)                       \
    rbc_wire_receive(rcv, count, msgs, rng_, rbytes, of, ln, in, ix, rt, sl, vd, o.types.data(), va, vl, vpitch, \
                     o.digests.data(), st, tk)
#define BAD(...)                                               \
    do {                                                       \
        EXPECT(CALL(__VA_ARGS__) == RBC_ERR_INVALID_ARG);      \
        EXPECT(o.untouched());                                 \
    } while (0)
    uint8_t *vd = o.verdict.data(), *va = o.valid.data(), *vl = o.values.data();
    int32_t *st = o.status.data();
    const uint8_t *rg = ring.data(), *rt = roots.data();
    // null pointers
    BAD(2, 4, nullptr, rb, offs, lens, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);
    BAD(2, 4, rg, rb, nullptr, lens, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);
    BAD(2, 4, rg, rb, offs, nullptr, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);
    BAD(2, 4, rg, rb, offs, lens, nullptr, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);
    BAD(2, 4, rg, rb, offs, lens, inst, nullptr, rt, slens, vd, va, vl, vp, st, &o.ticket);
    BAD(2, 4, rg, rb, offs, lens, inst, idx, nullptr, slens, vd, va, vl, vp, st, &o.ticket);
    BAD(2, 4, rg, rb, offs, lens, inst, idx, rt, nullptr, vd, va, vl, vp, st, &o.ticket);
    BAD(2, 4, rg, rb, offs, lens, inst, idx, rt, slens, nullptr, va, vl, vp, st, &o.ticket);
    BAD(2, 4, rg, rb, offs, lens, inst, idx, rt, slens, vd, nullptr, vl, vp, st, &o.ticket);
    BAD(2, 4, rg, rb, offs, lens, inst, idx, rt, slens, vd, va, nullptr, vp, st, &o.ticket);
    BAD(2, 4, rg, rb, offs, lens, inst, idx, rt, slens, vd, va, vl, vp, nullptr, &o.ticket);
    BAD(2, 4, rg, rb, offs, lens, inst, idx, rt, slens, vd, va, vl, vp, st, nullptr);
    EXPECT(rbc_wire_receive(nullptr, 2, 4, rg, rb, offs, lens, inst, idx, rt, slens, vd, nullptr, va, vl, vp, nullptr,
                            st, &o.ticket) == RBC_ERR_INVALID_ARG);
    // the limits of the receiver
    BAD(3, 4, rg, rb, offs, lens, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);  // count > max_count
    BAD(2, 5, rg, rb, offs, lens, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);  // msgs > max_msgs
    BAD(2, 4, rg, 4096 + 16, offs, lens, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);  // ring > max_ring_bytes
    BAD(-1, 4, rg, rb, offs, lens, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);
    BAD(2, -1, rg, rb, offs, lens, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);
    BAD(0, 4, rg, rb, offs, lens, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);  // messages of no instance
    // the messages
    uint64_t bad_offs[4] = {offs[0], offs[1] + 8, offs[2], offs[3]};
    BAD(2, 4, rg, rb, bad_offs, lens, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);  // misaligned offs
    BAD(2, 4, rg, rb - 16, offs, lens, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);  // past ring_bytes
    uint64_t wrap_offs[4] = {offs[0], ~(uint64_t)0 - 15, offs[2], offs[3]};
    BAD(2, 4, rg, rb, wrap_offs, lens, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);  // wrap-around
    uint32_t long_lens[4] = {lens[0], lens[1], lens[2], 0xfffffff9u};
    BAD(2, 4, rg, rb, offs, long_lens, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);
    uint32_t bad_inst[4] = {0, 0, 2, 1};
    BAD(2, 4, rg, rb, offs, lens, bad_inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);  // inst >= count
    uint32_t huge_inst[4] = {0, 0xffffffffu, 0, 1};
    BAD(2, 4, rg, rb, offs, lens, huge_inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);
    BAD(1, 4, rg, rb, offs, lens, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket);      // inst 1 of count 1
    uint8_t bad_idx[4] = {0, 3, (uint8_t)g.n, 1};
    BAD(2, 4, rg, rb, offs, lens, inst, bad_idx, rt, slens, vd, va, vl, vp, st, &o.ticket);  // idx >= n
    uint8_t dup_idx[4] = {0, 3, 0, 1};
    BAD(2, 4, rg, rb, offs, lens, inst, dup_idx, rt, slens, vd, va, vl, vp, st, &o.ticket);  // (0, 0) twice
    uint32_t dup_inst[4] = {0, 0, 0, 0};
    uint8_t dup_idx2[4] = {0, 3, 6, 6};
    BAD(2, 4, rg, rb, offs, lens, dup_inst, dup_idx2, rt, slens, vd, va, vl, vp, st, &o.ticket);  // the last two
    // the lengths
    const size_t zero_len[2] = {45, 0}, long_len[2] = {pitch + 1, 64};
    BAD(2, 4, rg, rb, offs, lens, inst, idx, rt, zero_len, vd, va, vl, vp, st, &o.ticket);
    BAD(2, 4, rg, rb, offs, lens, inst, idx, rt, long_len, vd, va, vl, vp, st, &o.ticket);
    BAD(2, 4, rg, rb, offs, lens, inst, idx, rt, slens, vd, va, vl, vp - 1, st, &o.ticket);  // value_pitch < k*Smax
    // random arguments: whatever the answer, nothing overruns (ASan), and a rejected call writes nothing
    for (int rep = 0; rep < 300; ++rep) {
        uint64_t ro[4];
        uint32_t rl[4], ri[4];
        uint8_t rx[4];
        for (int m = 0; m < 4; ++m) {
            ro[m] = rng() % 3 ? offs[m] : (rng() % 2 ? rng() : rng() % (rb + 64));
            rl[m] = rng() % 3 ? lens[m] : (uint32_t)(rng() % 2 ? rng() : rng() % 400);
            ri[m] = rng() % 3 ? inst[m] : (uint32_t)(rng() % 2 ? rng() : rng() % 3);
            rx[m] = rng() % 3 ? idx[m] : (uint8_t)(rng() % 9);
        }
        const size_t rs[2] = {rng() % 4 ? slens[0] : (size_t)(rng() % (pitch + 2)), slens[1]};
        const int rcount = rng() % 8 ? 2 : (int)(rng() % 4), rmsgs = rng() % 8 ? 4 : (int)(rng() % 6);
        const size_t rrb = rng() % 4 ? rb : (size_t)(rng() % (rb + 1));
        Outs q(2, 4, n, vp);
        const int rc = rbc_wire_receive(rcv, rcount, rmsgs, rg, rrb, ro, rl, ri, rx, rt, rs, q.verdict.data(),
                                        q.types.data(), q.valid.data(), q.values.data(), vp, q.digests.data(),
                                        q.status.data(), &q.ticket);
        EXPECT(rc == RBC_OK || rc == RBC_ERR_INVALID_ARG);
        if (rc == RBC_OK) EXPECT(rbc_wire_receive_wait(rcv, q.ticket) == RBC_OK);
        else EXPECT(q.untouched());
    }
    // a good call still works.  The stand-in's verify zeroes valid[], so a decoded message reads 0,
    // another length 3 and a fallback 2
    EXPECT(CALL(2, 4, rg, rb, offs, lens, inst, idx, rt, slens, vd, va, vl, vp, st, &o.ticket) == RBC_OK);
    EXPECT(o.ticket != 77 && o.ticket != 0);
    int done = 0;
    EXPECT(rbc_wire_receive_poll(rcv, o.ticket, &done) == RBC_OK && done == 1);
    EXPECT(rbc_wire_receive_wait(rcv, o.ticket) == RBC_OK);
    EXPECT(vd[0] == 0 && vd[1] == 0 && vd[2] == 3 && vd[3] == 2);
    EXPECT(o.types[0] == RBC_MSG_ECHO);
    for (size_t i = 0; i < 2; ++i)  // k*S_i bytes, then zeros
        for (size_t b = k * slens[i]; b < vp; ++b) EXPECT(vl[i * vp + b] == 0);
    EXPECT(rbc_wire_receive_wait(rcv, o.ticket) == RBC_OK);
    EXPECT(rbc_wire_receive_wait(rcv, o.ticket + 1) == RBC_ERR_INVALID_ARG);
    // nullable outputs, no messages at all, no instances at all
    uint64_t t2 = 0;
    EXPECT(rbc_wire_receive(rcv, 2, 4, rg, rb, offs, lens, inst, idx, rt, slens, vd, nullptr, va, vl, vp, nullptr, st,
                            &t2) == RBC_OK && rbc_wire_receive_wait(rcv, t2) == RBC_OK);
    EXPECT(rbc_wire_receive(rcv, 2, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, rt, slens, nullptr, nullptr,
                            va, vl, vp, nullptr, st, &t2) == RBC_OK && rbc_wire_receive_wait(rcv, t2) == RBC_OK);
    EXPECT(rbc_wire_receive(rcv, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr, 0, nullptr, nullptr, &t2) == RBC_OK && t2 == 0);
    // a second submission completes the one before it
    Outs o2(2, 4, n, vp);
    uint64_t ta = 0, tb = 0;
    EXPECT(CALL(2, 4, rg, rb, offs, lens, inst, idx, rt, slens, vd, va, vl, vp, st, &ta) == RBC_OK);
    EXPECT(rbc_wire_receive(rcv, 2, 4, rg, rb, offs, lens, inst, idx, rt, slens, o2.verdict.data(), o2.types.data(),
                            o2.valid.data(), o2.values.data(), vp, o2.digests.data(), o2.status.data(), &tb) == RBC_OK);
    EXPECT(tb == ta + 1 && rbc_wire_receive_wait(rcv, tb) == RBC_OK && rbc_wire_receive_wait(rcv, ta) == RBC_OK);
    EXPECT(o2.verdict[2] == 3 && o2.verdict[3] == 2);
#undef BAD
#undef CALL
    rbc_wire_receiver_destroy(rcv);
    rbc_wire_receiver_destroy(nullptr);
    // the device ABI's own checks
    Dev d(256);
    uint64_t *d64 = (uint64_t *)d.p;
    uint32_t *d32 = (uint32_t *)d.p;
    int32_t *i32 = (int32_t *)d.p;
    EXPECT(rbc_dev_unmarshal_echo(ctx, nullptr, 1, 1, d.p, d64, d32, d32, d.p, d.p, d32, 0, d.p, 100, d.p, d.p, i32,
                                  d.p) == RBC_ERR_INVALID_ARG);  // shard_pitch % 64
    EXPECT(rbc_dev_unmarshal_echo(ctx, nullptr, -1, 1, d.p, d64, d32, d32, d.p, d.p, d32, 0, d.p, 64, d.p, d.p, i32,
                                  d.p) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_unmarshal_echo(ctx, nullptr, 1, 1, d.p, d64, d32, d32, d.p, d.p, d32, 0, nullptr, 64, d.p, d.p, i32,
                                  d.p) == RBC_ERR_INVALID_ARG);
    EXPECT(rbc_dev_unmarshal_echo(ctx, nullptr, 1, 1, d.p, d64, d32, d32, d.p, d.p, nullptr, 0, d.p, 64, d.p, d.p, i32,
                                  d.p) == RBC_ERR_INVALID_ARG);  // neither lengths nor a uniform length
    EXPECT(rbc_dev_unmarshal_echo(ctx, nullptr, 1, 1, d.p + 8, d64, d32, d32, d.p, d.p, d32, 0, d.p, 64, d.p, d.p, i32,
                                  d.p) == RBC_ERR_INVALID_ARG);  // ring not 16-byte aligned
    EXPECT(rbc_dev_unmarshal_echo(nullptr, nullptr, 1, 1, d.p, d64, d32, d32, d.p, d.p, d32, 0, d.p, 64, d.p, d.p, i32,
                                  d.p) == RBC_ERR_INVALID_ARG);
    for (size_t b = 0; b < d.bytes; ++b) EXPECT(d.p[b] == kCanary);
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
    const uint32_t pitch = 192;
    size_t total = 0, seen[4] = {0, 0, 0, 0}, must_ok = 0;
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
            const Host h = host_decode(g, m, ix);
            for (Setting s : {OWN, OTHER_ROOT, OTHER_LEN}) {
                const int st = run_one(ctx, g, m, ix, pitch, h, s);
                ++total;
                if (st >= 0 && st < 4) ++seen[st];
                if (expect_ok && s == OWN) {
                    ++must_ok;
                    EXPECT(st == RBC_WIRE_OK);
                }
            }
        };
        run(canon, idx, true);
        // the S bound: a pitch of exactly round_up(S, 64) decodes, one 64 below falls back
        const Host hc = host_decode(g, canon, idx);
        EXPECT(run_one(ctx, g, canon, idx, (uint32_t)rup(S, 64), hc, OWN) == RBC_WIRE_OK);
        if (S > 64) EXPECT(run_one(ctx, g, canon, idx, (uint32_t)rup(S, 64) - 64, hc, OWN) == RBC_WIRE_FALLBACK);
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
        // the JSON re-wrapped: forms the host decoder accepts but that are not canonical, and wrong
        // or non-minimal varints
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
            s.insert(s.size() - 1, ",\"Extra\":\"AAAA\"");
            js.push_back(s);
            const size_t bpos = json.find(",\"Block\":");  // Block first
            js.push_back("{" + json.substr(bpos + 1, json.size() - bpos - 2) + "," + json.substr(1, bpos - 1) + "}");
            s = json;
            s.insert(runs.b[2] - j0 + 4, "\\n");
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
        if (type) {  // READY, a type field of another value
            Bytes m = canon;
            m.back() = RBC_MSG_READY;
            run(m, idx, false);
            m.back() = 0x81;
            run(m, idx, false);
        }
    }
    // degenerate lengths: nothing is read past a short message
    for (size_t len = 0; len < 200; ++len) {
        Bytes m(len);
        for (uint8_t &b : m) b = (uint8_t)rng();
        if (len) m[0] = 0x1a;
        const Host h = host_decode(g, m, 0);
        const int st = run_one(ctx, g, m, 0, pitch, h, OWN);
        EXPECT(st == RBC_WIRE_FALLBACK || st == RBC_WIRE_OTHER_LEN);
        ++total;
    }
    EXPECT(total > 6000 && must_ok > 250);
    EXPECT(seen[RBC_WIRE_OK] >= must_ok && seen[RBC_WIRE_FALLBACK] && seen[RBC_WIRE_OTHER_ROOT] >= must_ok &&
           seen[RBC_WIRE_OTHER_LEN] >= must_ok);
    rbc_ctx_destroy(ctx);
    if (fails) {
        printf("FAIL %d\n", fails);
        return 1;
    }
    printf("ok %zu runs: %zu decoded, %zu fallback, %zu other root, %zu other length\n", total, seen[0], seen[1],
           seen[2], seen[3]);
    return 0;
}
