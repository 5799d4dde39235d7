// wire.hip -- per-recipient VAL / ECHO marshaling in HBM (SURVEY §8f ranks 2
// and 4: the pb payload codec and the proposer's send path).
//
// A proposer's VAL fan-out is N messages per instance, each carrying one
// shard as base64 inside the Go-JSON request (rbc/request.go:9-17) inside a
// pb.Message (pb/message.proto:11-35): 4/3 of the committed shard bytes,
// i.e. ~4.3 GB per C2 batch of 1024 proposals.  Serialising that on the host
// costs seconds of CPU per batch; here one wave per message writes the exact
// bytes of rbc_pb_encode_rbc(type, rbc_json_encode_val(...)) (csrc/rbc_node.cpp)
// straight from the device-resident shards, branches and roots, so the host
// only copies finished messages out (or hands device buffers to a
// GPU-direct transport).
//
// Byte work, HBM-bound: every lane produces one aligned 16-byte chunk of its
// message per step.  Chunks wholly inside a base64 run (the shard, the
// branch) take the fast path: 3 dword loads' worth of source (5 dwords, one
// funnel shift), 5 base64 groups as packed sextets, SWAR ASCII mapping, one
// funnel shift to the chunk's phase and one 16-byte store.  The few chunks
// that straddle a header, a JSON literal or a run's end take a per-byte path.
//
// The receive side (unmarshal_val_kernel, below the marshal kernel) is the
// inverse: canonical messages decoded back into the device forms, everything
// else left to the host decoder.  unmarshal_echo_kernel is the same decode
// for a receiver that batches an epoch's ECHOs: it writes each shard and
// branch once, at the leaf position of its instance's shard set.
// unmarshal_ready_kernel decodes the third kind, READY, into a per-instance
// sender bitmap, and quorum_kernel turns that bitmap and verify's valid[] into
// the protocol's counts and decisions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace {

__device__ __forceinline__ uint32_t b64_len(uint32_t n) { return (n + 2) / 3 * 4; }
__device__ __forceinline__ uint32_t varint_len(uint32_t v) {
    uint32_t l = 1;
    while (v >= 0x80) {
        v >>= 7;
        ++l;
    }
    return l;
}

// JSON literals of the request (rbc/request.go field order)
__constant__ const char kLit[] =
    "{\"RootHash\":\""                  // 0, 13
    "\",\"Branch\":\""                  // 13, 12
    "\",\"Block\":[\""                  // 25, 12
    "\"]}"                              // 37, 3
    "\",\"Branch\":null,\"Block\":[\""; // 40, 26

// Message layout for one (instance, row): piece start offsets.
struct Layout {
    uint32_t total;            // message bytes
    uint32_t hdr;              // 0x1a varint(R) 0x0a varint(J)
    uint32_t R, J;
    uint32_t root_off;         // base64 of the root (44 chars)
    uint32_t br_lit_off;       // '","Branch":"' or the null variant
    uint32_t br_off, br_len;   // base64 of the branch (br_len source bytes)
    uint32_t blk_lit_off;      // '","Block":["' (absent for a null branch)
    uint32_t blk_off, S;       // base64 of the shard
    uint32_t end_lit_off;      // '"]}'
    uint32_t type_off;         // 0x10 type, when type != 0
};

__device__ __forceinline__ Layout layout(uint32_t S, uint32_t br_len, int type) {
    Layout L;
    L.S = S;
    L.br_len = br_len;
    const uint32_t Bk = b64_len(S), Bb = b64_len(br_len);
    L.J = br_len ? 84 + Bb + Bk : 86 + Bk;
    L.R = 1 + varint_len(L.J) + L.J + (type ? 2 : 0);
    L.hdr = 1 + varint_len(L.R) + 1 + varint_len(L.J);
    L.total = 1 + varint_len(L.R) + L.R;
    L.root_off = L.hdr + 13;
    L.br_lit_off = L.root_off + 44;
    if (br_len) {
        L.br_off = L.br_lit_off + 12;
        L.blk_lit_off = L.br_off + Bb;
        L.blk_off = L.blk_lit_off + 12;
    } else {
        L.br_off = L.blk_lit_off = L.br_lit_off + 26;
        L.blk_off = L.br_lit_off + 26;
    }
    L.end_lit_off = L.blk_off + Bk;
    L.type_off = L.end_lit_off + 3;
    return L;
}

__device__ __forceinline__ uint32_t b64_char(uint32_t v) {
    return v < 26 ? 'A' + v : v < 52 ? 'a' + v - 26 : v < 62 ? '0' + v - 52 : v == 62 ? '+' : '/';
}

// character c of base64(src[0..len)) (standard alphabet, '=' padding)
__device__ __forceinline__ uint32_t b64_at(const uint8_t *src, uint32_t len, uint32_t c) {
    const uint32_t g = c >> 2, r = c & 3, b = 3 * g;
    const uint32_t n = len - b;  // source bytes in this group (>= 1)
    if (r >= 2 && n <= r - 1) return '=';
    const uint32_t b0 = src[b], b1 = n > 1 ? src[b + 1] : 0, b2 = n > 2 ? src[b + 2] : 0;
    const uint32_t w = b0 << 16 | b1 << 8 | b2;
    return b64_char((w >> (18 - 6 * r)) & 63);
}

__device__ __forceinline__ uint32_t varint_byte(uint32_t v, uint32_t i) {
    const uint32_t b = (v >> (7 * i)) & 0x7f;
    return (v >> (7 * (i + 1))) ? (b | 0x80) : b;
}

// byte p of the message (the slow, per-byte path)
__device__ uint32_t msg_byte(const Layout &L, uint32_t p, int type, const uint8_t *root, const uint8_t *br,
                             const uint8_t *blk) {
    if (p >= L.total) return 0;
    if (p < L.hdr) {
        const uint32_t vr = varint_len(L.R);
        if (p == 0) return 0x1a;
        if (p < 1 + vr) return varint_byte(L.R, p - 1);
        if (p == 1 + vr) return 0x0a;
        return varint_byte(L.J, p - 2 - vr);
    }
    if (p < L.root_off) return (uint8_t)kLit[p - L.hdr];
    if (p < L.br_lit_off) return b64_at(root, 32, p - L.root_off);
    if (!L.br_len) {
        if (p < L.blk_off) return (uint8_t)kLit[40 + p - L.br_lit_off];
    } else {
        if (p < L.br_off) return (uint8_t)kLit[13 + p - L.br_lit_off];
        if (p < L.blk_lit_off) return b64_at(br, L.br_len, p - L.br_off);
        if (p < L.blk_off) return (uint8_t)kLit[25 + p - L.blk_lit_off];
    }
    if (p < L.end_lit_off) return b64_at(blk, L.S, p - L.blk_off);
    if (p < L.type_off) return (uint8_t)kLit[37 + p - L.end_lit_off];
    return p == L.type_off ? 0x10u : (uint32_t)type;
}

// 4 sextets (already in output order, one per byte) -> 4 base64 ASCII bytes
__device__ __forceinline__ uint32_t b64_ascii4(uint32_t v) {
    const uint32_t t26 = (v + 0x66666666u) & 0x80808080u;  // byte >= 26
    const uint32_t t52 = (v + 0x4c4c4c4cu) & 0x80808080u;  // >= 52
    const uint32_t t62 = (v + 0x42424242u) & 0x80808080u;  // >= 62
    const uint32_t t63 = (v + 0x41414141u) & 0x80808080u;  // == 63
    // 'A' + v, +6 from 26 ('a'), -75 from 52 ('0'), -15 at 62 ('+'), +3 at 63 ('/');
    // additions first, so no byte borrows from its neighbour
    const uint32_t pos = v + 0x41414141u + (t26 >> 5) + (t26 >> 6) + (t63 >> 6) + (t63 >> 7);
    const uint32_t neg = (t52 >> 1) + (t52 >> 4) + (t52 >> 6) + (t52 >> 7) + (t62 >> 3) - (t62 >> 7);
    return pos - neg;
}

// 24-bit big-endian group w -> its 4 sextets, first in the lowest byte
__device__ __forceinline__ uint32_t sextets(uint32_t w) {
    return ((w >> 18) & 0x3fu) | ((w >> 4) & 0x3f00u) | ((w << 10) & 0x3f0000u) | ((w << 24) & 0x3f000000u);
}

// Fast path: the 16 characters of base64(src) starting at character c0, all
// from full groups and with 20 readable source bytes from 3*(c0/4) on.
__device__ __forceinline__ uint4 b64_chunk16(const uint8_t *src, uint32_t c0) {
    const uint32_t g0 = c0 >> 2, e = c0 & 3, sb = 3 * g0, a = sb & 3;
    const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src) + (sb >> 2);
    const uint32_t d0 = s32[0], d1 = s32[1], d2 = s32[2], d3 = s32[3], d4 = s32[4];
    // E = source bytes sb .. sb+15
    const uint32_t e0 = __builtin_amdgcn_alignbyte(d1, d0, a), e1 = __builtin_amdgcn_alignbyte(d2, d1, a);
    const uint32_t e2 = __builtin_amdgcn_alignbyte(d3, d2, a), e3 = __builtin_amdgcn_alignbyte(d4, d3, a);
    // five groups as 24-bit big-endian words (byte-permute selectors: {hi:lo})
    const uint32_t w0 = __builtin_amdgcn_perm(e1, e0, 0x0c000102u);
    const uint32_t w1 = __builtin_amdgcn_perm(e1, e0, 0x0c030405u);
    const uint32_t w2 = __builtin_amdgcn_perm(e2, e1, 0x0c020304u);
    const uint32_t w3 = __builtin_amdgcn_perm(e3, e2, 0x0c010203u);
    const uint32_t w4 = __builtin_amdgcn_perm(e3, e3, 0x0c000102u);
    const uint32_t g[5] = {b64_ascii4(sextets(w0)), b64_ascii4(sextets(w1)), b64_ascii4(sextets(w2)),
                           b64_ascii4(sextets(w3)), b64_ascii4(sextets(w4))};
    // characters e .. e+15 of the 20
    return make_uint4(__builtin_amdgcn_alignbyte(g[1], g[0], e), __builtin_amdgcn_alignbyte(g[2], g[1], e),
                      __builtin_amdgcn_alignbyte(g[3], g[2], e), __builtin_amdgcn_alignbyte(g[4], g[3], e));
}

// is [p, p+16) a fast-path chunk of the base64 run of `len` bytes at `off`?
__device__ __forceinline__ bool fast_run(uint32_t p, uint32_t off, uint32_t len) {
    if (p < off) return false;
    const uint32_t c0 = p - off;
    const uint32_t full_chars = len / 3 * 4;
    if (c0 + 16 > full_chars) return false;
    const uint32_t w0 = (3 * (c0 >> 2)) >> 2;  // first source dword
    return 4 * (w0 + 5) <= len;                 // five dwords inside the run
}

// one wave per message; 4 waves (messages) per block
__global__ __launch_bounds__(256) void marshal_val_kernel(WireArgs a) {
    const uint32_t msg = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (msg >= (uint32_t)a.count * (uint32_t)a.n) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t inst = msg / a.n, j = msg - inst * a.n;
    const uint32_t S = a.lens ? a.lens[inst] : a.uniform_len;
    const bool empty0 = a.depth > 0 && (int)(j ^ 1u) >= a.n;
    const uint32_t br_len = 32u * (a.depth - (empty0 ? 1 : 0));
    const Layout L = layout(S, br_len, a.type);
    const uint8_t *root = a.roots + (size_t)inst * 32;
    const uint8_t *br = a.branches + ((size_t)inst * a.n + j) * a.depth * 32u + (empty0 ? 32u : 0u);
    const uint8_t *blk = a.shards + (size_t)inst * a.inst_pitch + (size_t)j * a.row_pitch;
    uint8_t *out = a.out + (size_t)msg * a.out_pitch;
    const uint32_t nchunks = (L.total + 15) >> 4;
    for (uint32_t q = lane; q < nchunks; q += 64) {
        const uint32_t p = q << 4;
        uint4 v;
        if (fast_run(p, L.blk_off, S)) {
            v = b64_chunk16(blk, p - L.blk_off);
        } else if (br_len && fast_run(p, L.br_off, br_len)) {
            v = b64_chunk16(br, p - L.br_off);
        } else {
            uint32_t d[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                uint32_t x = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) x |= msg_byte(L, p + 4 * w + b, a.type, root, br, blk) << (8 * b);
                d[w] = x;
            }
            v = make_uint4(d[0], d[1], d[2], d[3]);
        }
        *reinterpret_cast<uint4 *>(out + p) = v;
    }
    if (lane == 0 && a.out_lens) a.out_lens[msg] = L.total;
}

// ---------------------------------------------------------------------------
// The receive side: unmarshal_val_kernel, the inverse of marshal_val_kernel.
//
// A message is decoded only when it is canonical, i.e. byte-for-byte what the
// kernel above writes for some (root, branch, shard, type).  Its shape then
// follows from its length and the sender's leaf alone: the branch length from
// (idx, n, depth), the block's base64 length from the total, S from that and
// the block's trailing '=' count.  So the wave derives a Layout from lens[i],
// never from a byte of the message, and then checks every byte against it:
// header and literals against msg_byte(), every base64 character against the
// alphabet, '=' only where b64_len() pads.  Anything else is WIRE_FALLBACK,
// the host decoder's business.  Like Go's non-strict decoder (and
// b64_decode_range, rbc_node.cpp) the non-zero trailing bits of a last quantum
// are ignored.
//
// Output-centric like the send side: a lane-step produces one aligned 16-byte
// chunk of decoded bytes with one store.  A chunk wholly inside full groups
// reads its 24 characters as 7 dwords and one funnel shift each, maps ASCII to
// sextets with SWAR range arithmetic (which yields the invalid-character mask),
// packs each group with shift-or and a byte permute, and funnel-shifts the 18
// bytes to the chunk's phase.  The chunks at a run's end go byte by byte.
// ---------------------------------------------------------------------------

// The Layout of a canonical message of `total` bytes with a br_len-byte
// branch, if there is one (L.S is then the unpadded 3 * groups), from
// layout() alone: total = overhead + 4 * groups, where the overhead grows by
// at most 8 (two varints) over that of a one-group message.
__device__ bool rx_layout(uint32_t total, uint32_t br_len, Layout &L, int &type) {
    if (total > 0x7fffffffu) return false;
    for (int t = 0; t < 2; ++t) {
        const uint32_t t1 = layout(3, br_len, t).total;
        if (total < t1) continue;
        const uint32_t G = 1 + ((total - t1) >> 2);
        for (uint32_t d = 0; d < 4 && d < G; ++d) {
            const Layout c = layout(3 * (G - d), br_len, t);
            if (c.total == total) {
                L = c;
                type = t;
                return true;
            }
        }
    }
    return false;
}

// alphabet value of one character, -1 outside the standard alphabet
__device__ __forceinline__ int b64_val(uint32_t c) {
    return c - 'A' < 26u ? (int)(c - 'A')
           : c - 'a' < 26u ? (int)(c - 'a' + 26)
           : c - '0' < 10u ? (int)(c - '0' + 52)
           : c == '+' ? 62
           : c == '/' ? 63
                      : -1;
}

// 4 base64 characters -> their sextets, byte for byte; bad gets 0x80 in every
// byte that is outside the alphabet
__device__ __forceinline__ uint32_t b64_sextets4(uint32_t x, uint32_t &bad) {
    const uint32_t c = x & 0x7f7f7f7fu;  // 7-bit bytes: the range adds below never carry across
#define RBC_GE(k) ((c + (0x80u - (uint32_t)(k)) * 0x01010101u) & 0x80808080u)
    const uint32_t up = RBC_GE('A') & ~RBC_GE('Z' + 1), lo = RBC_GE('a') & ~RBC_GE('z' + 1);
    const uint32_t dg = RBC_GE('0') & ~RBC_GE('9' + 1), pl = RBC_GE('+') & ~RBC_GE('+' + 1);
    const uint32_t sl = RBC_GE('/') & ~RBC_GE('/' + 1);
#undef RBC_GE
    bad |= (x | ~(up | lo | dg | pl | sl)) & 0x80808080u;
    // value = c + offset (mod 64): 'A' -> 0, 'a' -> 26, '0' -> 52, '+' -> 62, '/' -> 63
    const uint32_t off = (up >> 7) * 63u + (lo >> 7) * 57u + (dg >> 7) * 4u + (pl >> 7) * 19u + (sl >> 7) * 16u;
    return (c + off) & 0x3f3f3f3fu;
}

// 4 sextets (first in the lowest byte) -> the group's 3 bytes, first in the lowest byte
__device__ __forceinline__ uint32_t b64_bytes3(uint32_t v) {
    const uint32_t w = ((v & 0x3fu) << 18) | ((v & 0x3f00u) << 4) | ((v >> 10) & 0xfc0u) | (v >> 24);
    return __builtin_amdgcn_perm(0u, w, 0x0c000102u);
}

// Fast path: decoded bytes [o0, o0 + 16) of the base64 run at message offset
// off, from the 6 full groups (24 characters) that hold them.  Reads the 7
// dwords from the one that holds the first character on.
__device__ __forceinline__ uint4 unb64_chunk16(const uint8_t *m, uint32_t off, uint32_t o0, uint32_t &bad) {
    const uint32_t g0 = o0 / 3, e = o0 - 3 * g0, P = off + 4 * g0, al = P & 3;
    const uint32_t *s32 = reinterpret_cast<const uint32_t *>(m) + (P >> 2);
    const uint32_t d0 = s32[0], d1 = s32[1], d2 = s32[2], d3 = s32[3], d4 = s32[4], d5 = s32[5], d6 = s32[6];
    const uint32_t t0 = b64_bytes3(b64_sextets4(__builtin_amdgcn_alignbyte(d1, d0, al), bad));
    const uint32_t t1 = b64_bytes3(b64_sextets4(__builtin_amdgcn_alignbyte(d2, d1, al), bad));
    const uint32_t t2 = b64_bytes3(b64_sextets4(__builtin_amdgcn_alignbyte(d3, d2, al), bad));
    const uint32_t t3 = b64_bytes3(b64_sextets4(__builtin_amdgcn_alignbyte(d4, d3, al), bad));
    const uint32_t t4 = b64_bytes3(b64_sextets4(__builtin_amdgcn_alignbyte(d5, d4, al), bad));
    const uint32_t t5 = b64_bytes3(b64_sextets4(__builtin_amdgcn_alignbyte(d6, d5, al), bad));
    // the 18 bytes as dwords, then bytes e .. e+15 of them
    const uint32_t D0 = t0 | t1 << 24, D1 = t1 >> 8 | t2 << 16, D2 = t2 >> 16 | t3 << 8, D3 = t4 | t5 << 24;
    const uint32_t D4 = t5 >> 8;
    return make_uint4(__builtin_amdgcn_alignbyte(D1, D0, e), __builtin_amdgcn_alignbyte(D2, D1, e),
                      __builtin_amdgcn_alignbyte(D3, D2, e), __builtin_amdgcn_alignbyte(D4, D3, e));
}

// Slow path: decoded bytes [o0, o0 + 16) of the run of len bytes, zeros from
// len on; checks all four characters of every group it takes a byte from
// (alphabet, and '=' exactly on the padding positions of the last group).
__device__ uint4 unb64_chunk_slow(const uint8_t *m, uint32_t off, uint32_t len, uint32_t o0, uint32_t &bad) {
    const uint32_t ng = (len + 2) / 3, pad = 3 * ng - len;
    uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        const uint32_t o = o0 + b;
        if (o < len) {
            const uint32_t g = o / 3, r = o - 3 * g;
            const uint32_t np = (g == ng - 1) ? pad : 0u;
            const uint8_t *c = m + off + 4 * g;
            uint32_t w = 0;
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t ch = c[q];
                int v = 0;
                if (q + np >= 4) {
                    if (ch != '=') bad |= 1u;
                } else if ((v = b64_val(ch)) < 0) {
                    bad |= 1u;
                    v = 0;
                }
                w = w << 6 | (uint32_t)v;
            }
            d[b >> 2] |= ((w >> (16 - 8 * r)) & 0xffu) << (8 * (b & 3));
        }
    }
    return make_uint4(d[0], d[1], d[2], d[3]);
}

// branch slot r of a receiver: max(depth, 1) entries
__device__ __forceinline__ uint8_t *branch_slot(uint8_t *branches, size_t r, int depth) {
    return branches + r * (depth > 1 ? depth : 1) * 32u;
}

// the bits in which 16 decoded bytes of a root differ from the wanted ones
__device__ __forceinline__ uint32_t root_diff(const uint4 &v, const uint8_t *want) {
    const uint4 w = *reinterpret_cast<const uint4 *>(want);
    return (v.x ^ w.x) | (v.y ^ w.y) | (v.z ^ w.z) | (v.w ^ w.w);
}

// S from rx_layout()'s L.S and the block's trailing '=': inside [0, total), the first bytes read
__device__ __forceinline__ uint32_t rx_shard_len(const uint8_t *m, const Layout &L) {
    const uint32_t pad = m[L.end_lit_off - 1] == '=' ? (m[L.end_lit_off - 2] == '=' ? 2u : 1u) : 0u;
    return L.S - pad;
}

// Header, JSON literals and type field against msg_byte(): at most
// 12 + 13 + 26 + 3 + 2 bytes, one per lane; 1 in a lane whose byte differs.
__device__ __forceinline__ uint32_t literals_bad(const uint8_t *m, const Layout &L, uint32_t br_len, int type,
                                                 uint32_t lane) {
    const uint32_t head = L.hdr + 13, mid = br_len ? 24u : 26u;
    const uint32_t nn = head + mid + 3 + (type ? 2u : 0u);
    uint32_t bad = 0;
    if (lane < nn) {
        uint32_t p;
        if (lane < head) {
            p = lane;
        } else {
            const uint32_t k = lane - head;
            if (k >= mid) p = L.end_lit_off + (k - mid);  // '"]}' and the type field behind it
            else if (br_len && k >= 12) p = L.blk_lit_off + (k - 12);
            else p = L.br_lit_off + k;
        }
        if (m[p] != msg_byte(L, p, type, nullptr, nullptr, nullptr)) bad = 1;
    }
    return bad;
}

// decoded bytes [o0, o0 + 16) of the run of len bytes: zeros from len on, else the fast or the slow path
__device__ __forceinline__ uint4 unb64_chunk(const uint8_t *m, uint32_t off, uint32_t len, uint32_t o0, uint32_t &bad) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (o0 < len) {
        if (4 * (o0 / 3) + 24 <= len / 3 * 4) v = unb64_chunk16(m, off, o0, bad);
        else v = unb64_chunk_slow(m, off, len, o0, bad);
    }
    return v;
}

// one wave per message; 4 waves (messages) per block
__global__ __launch_bounds__(256) void unmarshal_val_kernel(WireRxArgs a) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= (uint32_t)a.count) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t total = a.lens[i], j = a.idx[i];
    const uint8_t *m = a.msgs + a.offs[i];
    const bool empty0 = a.depth > 0 && (int)(j ^ 1u) >= a.n;
    const uint32_t br_len = 32u * (a.depth - (empty0 ? 1 : 0));
    // the shape, from the length and the leaf alone (wave-uniform)
    Layout L;
    int type = 0;
    bool shaped = j < (uint32_t)a.n && rx_layout(total, br_len, L, type);
    uint32_t S = 0;
    if (shaped) {
        S = rx_shard_len(m, L);
        shaped = S <= a.row_pitch;
    }
    if (!shaped) {
        if (lane == 0) {
            a.status[i] = WIRE_FALLBACK;
            a.types[i] = 0;
            a.shard_lens[i] = 0;
        }
        return;
    }
    L.S = S;
    uint32_t bad = literals_bad(m, L, br_len, type, lane);
    // the three base64 runs, one 16-byte chunk of decoded bytes per lane-step
    const uint32_t nblk = ((S + 63u) & ~63u) >> 4, nbr = br_len >> 4, nq = nblk + nbr + 2;
    uint8_t *slot = branch_slot(a.branches, i, a.depth);
    for (uint32_t q = lane; q < nq; q += 64) {
        uint32_t off, len, o0;
        uint8_t *dst;
        if (q < nblk) {
            off = L.blk_off, len = S, o0 = q << 4;
            dst = a.rows + (size_t)i * a.row_pitch;
        } else if (q < nblk + nbr) {
            off = L.br_off, len = br_len, o0 = (q - nblk) << 4;
            dst = slot + (empty0 ? 32u : 0u);
        } else {
            off = L.root_off, len = 32, o0 = (q - nblk - nbr) << 4;
            dst = a.roots + (size_t)i * 32;
        }
        const uint4 v = unb64_chunk(m, off, len, o0, bad);
        *reinterpret_cast<uint4 *>(dst + o0) = v;
    }
    // the zero slot of an empty level-0 sibling (or of a depth-0 tree)
    if ((empty0 || a.depth == 0) && lane < 2) reinterpret_cast<uint4 *>(slot)[lane] = make_uint4(0, 0, 0, 0);
    const bool fail = __any(bad != 0);
    if (lane == 0) {
        a.status[i] = fail ? WIRE_FALLBACK : WIRE_OK;
        a.types[i] = (uint8_t)type;
        a.shard_lens[i] = fail ? 0u : S;
    }
}

// unmarshal_echo_kernel: unmarshal_val_kernel for a receiver that already
// knows which instance a message belongs to and which root that instance
// collects ECHOs for.  The shard and the branch go straight to slot
// r = inst*n + idx of the rbc_rx_batch layout (what sha_rows / the decode
// read), so a shard is written once, and only once its message is accepted;
// the message's root is only compared, in registers, with roots[inst].  Same shape derivation, same byte checks, same
// chunk decode; the status order is kernels.h's (WireEchoArgs).
// one wave per message; 4 waves (messages) per block
__global__ __launch_bounds__(256) void unmarshal_echo_kernel(WireEchoArgs a) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= (uint32_t)a.msgs) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t total = a.lens[i], j = a.idx[i], in = a.inst[i];
    const uint8_t *m = a.ring + a.offs[i];
    const bool empty0 = a.depth > 0 && (int)(j ^ 1u) >= a.n;
    const uint32_t br_len = 32u * (a.depth - (empty0 ? 1 : 0));
    // the shape, from the length and the leaf alone (wave-uniform)
    Layout L;
    int type = 0;
    bool shaped = j < (uint32_t)a.n && in < (uint32_t)a.count && rx_layout(total, br_len, L, type);
    uint32_t S = 0;
    if (shaped) {
        S = rx_shard_len(m, L);
        shaped = S <= a.shard_pitch;
    }
    if (!shaped) {
        if (lane == 0) {
            a.msg_status[i] = WIRE_FALLBACK;
            if (a.types) a.types[i] = 0;
        }
        return;
    }
    // a shard of another length than its instance's: the slot stays as it is
    if (S != (a.shard_lens ? a.shard_lens[in] : a.uniform_len)) {
        if (lane == 0) {
            a.msg_status[i] = WIRE_OTHER_LEN;
            if (a.types) a.types[i] = (uint8_t)type;
        }
        return;
    }
    L.S = S;
    uint32_t bad = literals_bad(m, L, br_len, type, lane), other = 0;
    // the three base64 runs, one 16-byte chunk of decoded bytes per lane-step;
    // the two chunks of the root are compared, not stored
    const uint32_t nblk = ((S + 63u) & ~63u) >> 4, nbr = br_len >> 4, nq = nblk + nbr + 2;
    const size_t r = (size_t)in * a.n + j;
    uint8_t *row = a.shards + r * a.shard_pitch;
    uint8_t *slot = branch_slot(a.branches, r, a.depth);
    const uint8_t *want_root = a.roots + (size_t)in * 32;
    // chunk q: its run, its place in the run and where it goes (NULL: the root)
    auto chunk = [&](uint32_t q, uint32_t &off, uint32_t &len, uint32_t &o0) -> uint8_t * {
        if (q < nblk) {
            off = L.blk_off, len = S, o0 = q << 4;
            return row;
        }
        if (q < nblk + nbr) {
            off = L.br_off, len = br_len, o0 = (q - nblk) << 4;
            return slot + (empty0 ? 32u : 0u);
        }
        off = L.root_off, len = 32, o0 = (q - nblk - nbr) << 4;
        return nullptr;
    };
    // A rejected message leaves its slot as it was, so every character is
    // checked and the root compared before the first store.  The lane's first
    // chunk stays in registers (all of a message of up to 64 chunks, ~1 KB);
    // the chunks behind it are decoded a second time for the store.
    uint4 first = make_uint4(0, 0, 0, 0);
    for (uint32_t q = lane; q < nq; q += 64) {
        uint32_t off, len, o0;
        const uint8_t *dst = chunk(q, off, len, o0);
        const uint4 v = unb64_chunk(m, off, len, o0, bad);
        if (q == lane) first = v;
        if (!dst) other |= root_diff(v, want_root + o0);
    }
    const bool fail = __any(bad != 0), wrong = __any(other != 0);
    if (fail || wrong) {
        if (lane == 0) {
            a.msg_status[i] = fail ? WIRE_FALLBACK : WIRE_OTHER_ROOT;
            if (a.types) a.types[i] = (uint8_t)type;
        }
        return;
    }
    for (uint32_t q = lane; q < nq; q += 64) {
        uint32_t off, len, o0, again = 0;
        uint8_t *dst = chunk(q, off, len, o0);
        if (dst) *reinterpret_cast<uint4 *>(dst + o0) = q == lane ? first : unb64_chunk(m, off, len, o0, again);
    }
    // the zero slot of an empty level-0 sibling (or of a depth-0 tree)
    if ((empty0 || a.depth == 0) && lane < 2) reinterpret_cast<uint4 *>(slot)[lane] = make_uint4(0, 0, 0, 0);
    if (lane == 0) {
        a.msg_status[i] = WIRE_OK;
        if (a.types) a.types[i] = (uint8_t)type;
        a.present[r] = 1;
    }
}

// ---------------------------------------------------------------------------
// READY (include/rbc_protocol.h, RBC_HAS_WIRE_READY).  The third message kind
// has one canonical form of one length under both payload codecs,
//   0x1a R 0x0a J {"RootHash":"<44 characters>"} 0x10 0x02
// so there is no shape to derive: a message of another length is
// WIRE_FALLBACK before a byte of it is read, and every offset below is a
// constant.  The 44 characters are the base64 of 32 bytes: ten full groups and
// one padded by a single '=', which unb64_chunk_slow demands at the last
// character and refuses at the one before it -- the 31- and 33-byte roots,
// which encode to 44 characters too, fall back there.
//
// A message is 65 bytes, five 16-byte chunks, and has four pieces of work of
// at most 16 bytes each: the two halves of the root (the first wholly inside
// full groups: unb64_chunk16; the second holds the padded group:
// unb64_chunk_slow), the 17 literal bytes in front of the root and the 4
// behind it.  One lane takes each, so a message is a group of 4 lanes, a wave
// holds 16 messages and a block 64; a group never straddles a wave, and its
// verdict is one nibble of the wave's ballot.  No LDS, no cross-lane data.
// ---------------------------------------------------------------------------
constexpr uint32_t kReadyJ = 13 + 44 + 2;          // '{"RootHash":"', the root's base64, '"}'
constexpr uint32_t kReadyR = 1 + 1 + kReadyJ + 2;  // 0x0a varint(J), the payload, 0x10 type
constexpr uint32_t kReadyTotal = 1 + 1 + kReadyR;  // 0x1a varint(R), the rest
constexpr uint32_t kReadyRoot = 4 + 13;            // where the root's base64 begins
constexpr uint32_t kReadyTail = kReadyRoot + 44;   // '"}' and the type field
static_assert(kReadyJ < 128 && kReadyR < 128, "both varints are one byte");
static_assert(kReadyTail + 4 == kReadyTotal, "the READY layout");

// byte p of every canonical READY, for p outside the root's base64
__device__ __forceinline__ uint32_t ready_byte(uint32_t p) {
    if (p < 4) return p == 0 ? 0x1au : p == 1 ? kReadyR : p == 2 ? 0x0au : kReadyJ;
    if (p < kReadyRoot) return (uint8_t)kLit[p - 4];
    const uint32_t t = p - kReadyTail;
    return t == 0 ? '"' : t == 1 ? '}' : t == 2 ? 0x10u : 0x02u;
}

// four lanes per message; 16 messages per wave, 64 per block
__global__ __launch_bounds__(256) void unmarshal_ready_kernel(WireReadyArgs a) {
    const uint32_t m = blockIdx.x * 64 + (threadIdx.x >> 2);
    const uint32_t lane = threadIdx.x & 63, part = lane & 3;
    const bool live = m < (uint32_t)a.msgs;
    // length, instance and leaf: all that is decided before a byte of the message is read
    uint32_t in = 0, j = 0;
    bool shaped = false;
    if (live) {
        in = a.inst[m];
        j = a.idx[m];
        shaped = a.lens[m] == kReadyTotal && in < (uint32_t)a.count && j < (uint32_t)a.n;
    }
    uint32_t bad = 0, other = 0;
    if (shaped) {
        const uint8_t *msg = a.ring + a.offs[m];
        if (part < 2) {
            // half a root, compared with the instance's and not stored
            const uint32_t o0 = part << 4;
            uint4 v;
            if (4 * (o0 / 3) + 24 <= 32 / 3 * 4) v = unb64_chunk16(msg, kReadyRoot, o0, bad);
            else v = unb64_chunk_slow(msg, kReadyRoot, 32, o0, bad);
            other = root_diff(v, a.roots + (size_t)in * 32 + o0);
        } else {
            // the header and the JSON literal in front of the root, or '"}' and the type field behind it
            const uint32_t p0 = part == 2 ? 0u : kReadyTail, p1 = part == 2 ? kReadyRoot : kReadyTotal;
            for (uint32_t p = p0; p < p1; ++p)
                if (msg[p] != ready_byte(p)) bad = 1;
        }
    }
    // every lane of the wave is here: the group's verdict is its nibble of the ballots
    const uint32_t sh = lane & ~3u;
    const uint32_t fail = (uint32_t)(__ballot(bad != 0) >> sh) & 0xfu;
    const uint32_t wrong = (uint32_t)(__ballot(other != 0) >> sh) & 0xfu;
    if (live && part == 0) {
        const int st = (!shaped || fail) ? WIRE_FALLBACK : wrong ? WIRE_OTHER_ROOT : WIRE_OK;
        a.msg_status[m] = st;
        if (st == WIRE_OK) a.ready[(size_t)in * a.n + j] = 1;
    }
}

// quorum_kernel: the thresholds of rbc_node's advance() over counts
// (kernels.h, QuorumArgs).  One wave per instance; 4 waves (instances) per
// block.  n reaches 256, so the two counts take up to four wave-wide steps of
// one ballot and one popcount each; lane 0 then applies the rules.  Only
// ready[i][self] is ever written, by the wave that counted it.
__global__ __launch_bounds__(256) void quorum_kernel(QuorumArgs a) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= (uint32_t)a.count) return;  // wave-uniform
    const uint32_t lane = threadIdx.x & 63, n = (uint32_t)a.n;
    const uint8_t *valid = a.valid ? a.valid + (size_t)i * n : nullptr;
    uint8_t *ready = a.ready + (size_t)i * n;
    uint32_t E = 0, R = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += 64) {  // a wave-uniform trip count: every lane reaches the ballots
        const uint32_t t = t0 + lane;
        const bool inside = t < n;
        E += (uint32_t)__popcll(__ballot(inside && valid && valid[t] != 0));
        R += (uint32_t)__popcll(__ballot(inside && ready[t] != 0));
    }
    if (lane) return;
    const int32_t st = a.status ? a.status[i] : 1;  // no status: nothing is known about the interpolation
    const uint32_t f = (uint32_t)a.f;
    // n - f and n - 2f as signed numbers: a geometry with 2f > n has no quorum, not a wrapped one
    const bool echo_q = (int64_t)E >= (int64_t)n - (int64_t)f;
    const bool echo_k = (int64_t)E >= (int64_t)n - 2 * (int64_t)f;
    const bool amplify = R >= f + 1;
    const bool have = st == 0 && (echo_q || (R >= 2 * f + 1 && echo_k));
    const bool send_ready = amplify || have;
    if (send_ready && a.self >= 0 && !ready[a.self]) {  // the node's own READY counts
        ready[a.self] = 1;
        ++R;
    }
    const bool deliver = st == 0 && R >= 2 * f + 1 && echo_k;
    a.echo_counts[i] = E;
    a.ready_counts[i] = R;
    a.flags[i] = (uint8_t)((echo_q ? QUORUM_ECHO : 0) | (amplify ? QUORUM_AMPLIFY : 0) |
                           (send_ready ? QUORUM_SEND_READY : 0) | (deliver ? QUORUM_DELIVER : 0));
}

// ---------------------------------------------------------------------------
// The binary payload codec (include/rbc_protocol.h, RBC_HAS_WIRE_BINARY): the
// same pb.Message wrapper around
//   0xB1 0x01 L 0x00 | S as u32 LE | root[32] | branch[32*L] | shard[S]
// so root, branch and shard are raw bytes and the three kernels below are
// phase-shifted copies: the runs start 8 + 32*k bytes behind the wrapper's
// header, hence all at one phase of the 16-byte chunks, and that phase is
// wave-uniform.  Same launch shape and the same output contracts as the JSON
// kernels above; no LDS.
// ---------------------------------------------------------------------------

// Shape of the binary message of an S-byte shard with L branch entries.
struct BinLayout {
    uint32_t total, hdr;  // message bytes; 0x1a varint(R) 0x0a varint(J)
    uint32_t R, J, S, L;
    uint32_t root_off, br_off, blk_off, type_off;  // type_off: the end of the shard
};

__device__ __forceinline__ BinLayout bin_layout(uint32_t S, uint32_t L, int type) {
    BinLayout c;
    c.S = S;
    c.L = L;
    c.J = 40 + 32 * L + S;
    c.R = 1 + varint_len(c.J) + c.J + (type ? 2 : 0);
    c.hdr = 1 + varint_len(c.R) + 1 + varint_len(c.J);
    c.total = 1 + varint_len(c.R) + c.R;
    c.root_off = c.hdr + 8;
    c.br_off = c.root_off + 32;
    c.blk_off = c.br_off + 32 * L;
    c.type_off = c.blk_off + S;
    return c;
}

// byte p < hdr + 8 of the message: the wrapper's header and the payload's
__device__ __forceinline__ uint32_t bin_head_byte(const BinLayout &c, uint32_t p) {
    const uint32_t vr = varint_len(c.R);
    if (p == 0) return 0x1a;
    if (p < 1 + vr) return varint_byte(c.R, p - 1);
    if (p == 1 + vr) return 0x0a;
    if (p < c.hdr) return varint_byte(c.J, p - 2 - vr);
    const uint32_t k = p - c.hdr;
    return k == 0 ? 0xB1u : k == 1 ? 0x01u : k == 2 ? c.L : k == 3 ? 0u : (c.S >> (8 * (k - 4))) & 0xffu;
}

// byte p of the message (the slow, per-byte path of the marshal kernel)
__device__ uint32_t bin_msg_byte(const BinLayout &c, uint32_t p, const uint8_t *root, const uint8_t *br,
                                 const uint8_t *blk) {
    if (p >= c.total) return 0;
    if (p < c.root_off) return bin_head_byte(c, p);
    if (p < c.br_off) return root[p - c.root_off];
    if (p < c.blk_off) return br[p - c.br_off];
    if (p < c.type_off) return blk[p - c.blk_off];
    return p == c.type_off ? 0x10u : 0x01u;  // only ECHO has bytes here
}

// bytes [ph, ph + 16) of the 32 bytes lo:hi (ph < 16, wave-uniform)
__device__ __forceinline__ uint4 shift16(const uint4 lo, const uint4 hi, uint32_t ph) {
    const uint32_t c[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const uint32_t dw = ph >> 2, a = ph & 3;
    uint32_t e[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) e[k] = dw == 0 ? c[k] : dw == 1 ? c[k + 1] : dw == 2 ? c[k + 2] : c[k + 3];
    return make_uint4(__builtin_amdgcn_alignbyte(e[1], e[0], a), __builtin_amdgcn_alignbyte(e[2], e[1], a),
                      __builtin_amdgcn_alignbyte(e[3], e[2], a), __builtin_amdgcn_alignbyte(e[4], e[3], a));
}

// the first `keep` (< 16) bytes of v, zeros behind them
__device__ __forceinline__ uint4 keep_bytes(uint4 v, uint32_t keep) {
    uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        const uint32_t k = keep > 4 * w ? keep - 4 * w : 0u;
        if (k < 4) d[w] &= (1u << (8 * k)) - 1u;
    }
    return make_uint4(d[0], d[1], d[2], d[3]);
}

// 16 bytes from src, which may sit at any byte: the 4 or 5 aligned dwords that
// hold them (the last one holds src[15], so at most 3 bytes behind it are read)
__device__ __forceinline__ uint4 load16_any(const uint8_t *src) {
    const uintptr_t u = reinterpret_cast<uintptr_t>(src);
    const uint32_t a = (uint32_t)(u & 3);
    const uint32_t *s32 = reinterpret_cast<const uint32_t *>(u - a);
    const uint32_t d0 = s32[0], d1 = s32[1], d2 = s32[2], d3 = s32[3], d4 = a ? s32[4] : 0u;
    return make_uint4(__builtin_amdgcn_alignbyte(d1, d0, a), __builtin_amdgcn_alignbyte(d2, d1, a),
                      __builtin_amdgcn_alignbyte(d3, d2, a), __builtin_amdgcn_alignbyte(d4, d3, a));
}

// one wave per message; 4 waves (messages) per block
__global__ __launch_bounds__(256) void marshal_val_bin_kernel(WireArgs a) {
    const uint32_t msg = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (msg >= (uint32_t)a.count * (uint32_t)a.n) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t inst = msg / a.n, j = msg - inst * a.n;
    const uint32_t S = a.lens ? a.lens[inst] : a.uniform_len;
    const bool empty0 = a.depth > 0 && (int)(j ^ 1u) >= a.n;
    const BinLayout c = bin_layout(S, a.depth - (empty0 ? 1 : 0), a.type);
    const uint8_t *root = a.roots + (size_t)inst * 32;
    const uint8_t *br = a.branches + ((size_t)inst * a.n + j) * a.depth * 32u + (empty0 ? 32u : 0u);
    const uint8_t *blk = a.shards + (size_t)inst * a.inst_pitch + (size_t)j * a.row_pitch;
    uint8_t *out = a.out + (size_t)msg * a.out_pitch;
    const uint32_t nchunks = (c.total + 15) >> 4;
    for (uint32_t q = lane; q < nchunks; q += 64) {
        const uint32_t p = q << 4;
        uint4 v;
        // a chunk wholly inside one run is one shifted copy; the few that hold
        // the header, a run's border or the message's end go byte by byte
        if (p >= c.blk_off && p + 16 <= c.type_off) {
            v = load16_any(blk + (p - c.blk_off));
        } else if (p >= c.br_off && p + 16 <= c.blk_off) {
            v = load16_any(br + (p - c.br_off));
        } else if (p >= c.root_off && p + 16 <= c.br_off) {
            v = load16_any(root + (p - c.root_off));
        } else {
            uint32_t d[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                uint32_t x = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) x |= bin_msg_byte(c, p + 4 * w + b, root, br, blk) << (8 * b);
                d[w] = x;
            }
            v = make_uint4(d[0], d[1], d[2], d[3]);
        }
        *reinterpret_cast<uint4 *>(out + p) = v;
    }
    if (lane == 0 && a.out_lens) a.out_lens[msg] = c.total;
}

// The receive side.  Every offset comes from lens[i] and idx[i], never from a
// byte of the message: idx gives L, and for each type the total fixes S,
//   total = 2 + varint_len(R) + varint_len(J) + 40 + 32*L + S + (type ? 2 : 0),
// which grows strictly with S, so a type has at most one shape (and none where
// a varint grows past the total, or below the one-byte shard).  Most totals
// have one shape per type, (S, VAL) and (S - 2, ECHO).
__device__ bool bin_rx_shape(uint32_t total, uint32_t L, int type, uint32_t max_S, BinLayout &c) {
    if (total > 0x7fffffffu) return false;
    for (uint32_t vj = 1; vj <= 5; ++vj)
        for (uint32_t vr = vj; vr <= vj + 1; ++vr) {
            const uint32_t over = 2 + vr + vj + 40 + 32 * L + (type ? 2u : 0u);
            if (total <= over) continue;  // S >= 1
            c = bin_layout(total - over, L, type);
            if (c.total == total) return c.S <= max_S;
        }
    return false;
}

// Does the message carry candidate c's first hdr + 8 bytes (two varints, magic,
// version, L, reserved byte, S) and, for ECHO, the type field behind the shard?
// At most 20 + 2 bytes, one per lane; all inside [0, total).
__device__ __forceinline__ bool bin_matches(const uint8_t *m, const BinLayout &c, int type, uint32_t lane) {
    bool bad = false;
    if (lane < c.hdr + 8) bad = m[lane] != bin_head_byte(c, lane);
    else if (type && lane >= 32 && lane < 34) bad = m[c.type_off + lane - 32] != (lane == 32 ? 0x10u : 0x01u);
    return !__any(bad);
}

// Output chunk [o0, o0 + 16) of the run of len bytes at message offset off, as
// one or two aligned 16-byte loads inside [0, rt) and a shift by the run's
// phase; zeros from len on.
__device__ __forceinline__ uint4 bin_chunk16(const uint8_t *m, uint32_t rt, uint32_t off, uint32_t len,
                                             uint32_t o0) {
    if (o0 >= len) return make_uint4(0, 0, 0, 0);
    const uint32_t P = off + o0, A = P & ~15u, ph = P & 15u;
    const uint4 lo = *reinterpret_cast<const uint4 *>(m + A);
    uint4 hi = make_uint4(0, 0, 0, 0);
    if (ph && A + 16 < rt) hi = *reinterpret_cast<const uint4 *>(m + A + 16);
    const uint4 v = shift16(lo, hi, ph);
    return len - o0 < 16 ? keep_bytes(v, len - o0) : v;
}

// one wave per message; 4 waves (messages) per block
__global__ __launch_bounds__(256) void unmarshal_val_bin_kernel(WireRxArgs a) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= (uint32_t)a.count) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t total = a.lens[i], j = a.idx[i];
    const uint8_t *m = a.msgs + a.offs[i];
    const bool empty0 = a.depth > 0 && (int)(j ^ 1u) >= a.n;
    const uint32_t L = a.depth - (empty0 ? 1 : 0);
    // at most one candidate shape per type, then the one whose header the message carries
    BinLayout c, c1;
    int type = 0;
    bool shaped = false;
    if (j < (uint32_t)a.n) {
        shaped = bin_rx_shape(total, L, 0, a.row_pitch, c) && bin_matches(m, c, 0, lane);
        if (!shaped && bin_rx_shape(total, L, 1, a.row_pitch, c1) && bin_matches(m, c1, 1, lane)) {
            shaped = true;
            c = c1;
            type = 1;
        }
    }
    if (!shaped) {
        if (lane == 0) {
            a.status[i] = WIRE_FALLBACK;
            a.types[i] = 0;
            a.shard_lens[i] = 0;
        }
        return;
    }
    // root, branch and shard are any bytes: the message is canonical
    const uint32_t S = c.S, rt = (total + 15u) & ~15u;
    const uint32_t nblk = ((S + 63u) & ~63u) >> 4, nbr = 2 * L, nq = nblk + nbr + 2;
    uint8_t *slot = branch_slot(a.branches, i, a.depth);
    for (uint32_t q = lane; q < nq; q += 64) {
        uint32_t off, len, o0;
        uint8_t *dst;
        if (q < nblk) {
            off = c.blk_off, len = S, o0 = q << 4;
            dst = a.rows + (size_t)i * a.row_pitch;
        } else if (q < nblk + nbr) {
            off = c.br_off, len = 32 * L, o0 = (q - nblk) << 4;
            dst = slot + (empty0 ? 32u : 0u);
        } else {
            off = c.root_off, len = 32, o0 = (q - nblk - nbr) << 4;
            dst = a.roots + (size_t)i * 32;
        }
        *reinterpret_cast<uint4 *>(dst + o0) = bin_chunk16(m, rt, off, len, o0);
    }
    // the zero slot of an empty level-0 sibling (or of a depth-0 tree)
    if ((empty0 || a.depth == 0) && lane < 2) reinterpret_cast<uint4 *>(slot)[lane] = make_uint4(0, 0, 0, 0);
    if (lane == 0) {
        a.status[i] = WIRE_OK;
        a.types[i] = (uint8_t)type;
        a.shard_lens[i] = S;
    }
}

// unmarshal_val_bin_kernel for the receiver's batch layout (the contract of
// unmarshal_echo_kernel).  The instance's shard length is known, so the
// candidate is fixed before any byte of the message is read: the shape of that
// length, of whichever type has one.
// one wave per message; 4 waves (messages) per block
__global__ __launch_bounds__(256) void unmarshal_echo_bin_kernel(WireEchoArgs a) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= (uint32_t)a.msgs) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t total = a.lens[i], j = a.idx[i], in = a.inst[i];
    const uint8_t *m = a.ring + a.offs[i];
    const bool empty0 = a.depth > 0 && (int)(j ^ 1u) >= a.n;
    const uint32_t L = a.depth - (empty0 ? 1 : 0);
    BinLayout t;
    bool s0 = false, s1 = false;
    uint32_t S0 = 0, S1 = 0;
    if (j < (uint32_t)a.n && in < (uint32_t)a.count) {
        if ((s0 = bin_rx_shape(total, L, 0, a.shard_pitch, t))) S0 = t.S;
        if ((s1 = bin_rx_shape(total, L, 1, a.shard_pitch, t))) S1 = t.S;
    }
    if (!s0 && !s1) {
        if (lane == 0) {
            a.msg_status[i] = WIRE_FALLBACK;
            if (a.types) a.types[i] = 0;
        }
        return;
    }
    // a shard of another length than its instance's: the slot stays as it is
    const uint32_t S = a.shard_lens ? a.shard_lens[in] : a.uniform_len;
    const int type = (s0 && S0 == S) ? 0 : 1;
    if (type && !(s1 && S1 == S)) {
        if (lane == 0) {
            a.msg_status[i] = WIRE_OTHER_LEN;
            if (a.types) a.types[i] = (uint8_t)(s0 ? 0 : 1);
        }
        return;
    }
    const BinLayout c = bin_layout(S, L, type);
    if (!bin_matches(m, c, type, lane)) {
        if (lane == 0) {
            a.msg_status[i] = WIRE_FALLBACK;
            if (a.types) a.types[i] = (uint8_t)type;
        }
        return;
    }
    // the two chunks of the root are compared, not stored, and before any
    // store: a message for another root leaves its slot as it was
    const uint32_t rt = (total + 15u) & ~15u;
    const uint32_t nblk = ((S + 63u) & ~63u) >> 4, nbr = 2 * L, nq = nblk + nbr;
    const size_t r = (size_t)in * a.n + j;
    uint8_t *row = a.shards + r * a.shard_pitch;
    uint8_t *slot = branch_slot(a.branches, r, a.depth);
    const uint8_t *want_root = a.roots + (size_t)in * 32;
    uint32_t other = 0;
    if (lane < 2) other = root_diff(bin_chunk16(m, rt, c.root_off, 32, lane << 4), want_root + (lane << 4));
    if (__any(other != 0)) {
        if (lane == 0) {
            a.msg_status[i] = WIRE_OTHER_ROOT;
            if (a.types) a.types[i] = (uint8_t)type;
        }
        return;
    }
    // shard and branch to slot r
    for (uint32_t q = lane; q < nq; q += 64) {
        if (q < nblk) {
            *reinterpret_cast<uint4 *>(row + (q << 4)) = bin_chunk16(m, rt, c.blk_off, S, q << 4);
        } else {
            const uint32_t o0 = (q - nblk) << 4;
            *reinterpret_cast<uint4 *>(slot + (empty0 ? 32u : 0u) + o0) = bin_chunk16(m, rt, c.br_off, 32 * L, o0);
        }
    }
    // the zero slot of an empty level-0 sibling (or of a depth-0 tree)
    if ((empty0 || a.depth == 0) && lane < 2) reinterpret_cast<uint4 *>(slot)[lane] = make_uint4(0, 0, 0, 0);
    if (lane == 0) {
        a.msg_status[i] = WIRE_OK;
        if (a.types) a.types[i] = (uint8_t)type;
        a.present[r] = 1;
    }
}

}  // namespace

// The launchers choose the kernel by the payload codec (0 JSON, 1 binary).
hipError_t rbc_launch_unmarshal_echo(const WireEchoArgs &a, hipStream_t st) {
    if (a.codec != 0 && a.codec != 1) return hipErrorInvalidValue;
    if (a.msgs <= 0) return hipSuccess;
    const dim3 grid(((unsigned)a.msgs + 3) / 4), block(256);
    if (a.codec) hipLaunchKernelGGL(unmarshal_echo_bin_kernel, grid, block, 0, st, a);
    else hipLaunchKernelGGL(unmarshal_echo_kernel, grid, block, 0, st, a);
    return hipGetLastError();
}

// READY has one form under both codecs.  msg_len is what the host encoder
// emits for a 32-byte root: a kernel built for another layout refuses to run.
hipError_t rbc_launch_unmarshal_ready(const WireReadyArgs &a, hipStream_t st) {
    if (a.msg_len != kReadyTotal || a.n < 1 || a.n > 256) return hipErrorInvalidValue;
    if (a.msgs <= 0) return hipSuccess;
    const dim3 grid(((unsigned)a.msgs + 63) / 64), block(256);
    hipLaunchKernelGGL(unmarshal_ready_kernel, grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t rbc_launch_quorum(const QuorumArgs &a, hipStream_t st) {
    if (a.n < 1 || a.f < 0 || a.self < -1 || a.self >= a.n) return hipErrorInvalidValue;
    if (a.count <= 0) return hipSuccess;
    const dim3 grid(((unsigned)a.count + 3) / 4), block(256);
    hipLaunchKernelGGL(quorum_kernel, grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t rbc_launch_unmarshal_val(const WireRxArgs &a, hipStream_t st) {
    if (a.codec != 0 && a.codec != 1) return hipErrorInvalidValue;
    if (a.count <= 0) return hipSuccess;
    const dim3 grid(((unsigned)a.count + 3) / 4), block(256);
    if (a.codec) hipLaunchKernelGGL(unmarshal_val_bin_kernel, grid, block, 0, st, a);
    else hipLaunchKernelGGL(unmarshal_val_kernel, grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t rbc_launch_marshal_val(const WireArgs &a, hipStream_t st) {
    if (a.codec != 0 && a.codec != 1) return hipErrorInvalidValue;
    const uint64_t msgs = (uint64_t)a.count * a.n;
    if (!msgs) return hipSuccess;
    const dim3 grid((unsigned)((msgs + 3) / 4)), block(256);
    if (a.codec) hipLaunchKernelGGL(marshal_val_bin_kernel, grid, block, 0, st, a);
    else hipLaunchKernelGGL(marshal_val_kernel, grid, block, 0, st, a);
    return hipGetLastError();
}
