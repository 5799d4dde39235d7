// wire_rx_decode.cpp -- the host legs of tools/wire_rx_bench.py (A below, H at
// the end of the file).  Leg A: the host decode the
// parent path runs before rbc_validate_packed_keep.  One call decodes the
// messages [first, last) of a ring with rbc_pb_decode_rbc +
// rbc_json_decode_val straight into the packed validate arena; the bench
// calls it from 16 threads over disjoint slices.  Returns the number of
// messages the decoder rejected.
#include <stddef.h>
#include <stdint.h>

#include "../include/rbc_protocol.h"

extern "C" int wire_rx_decode_range(const uint8_t *ring, const uint64_t *offs, const uint32_t *lens, int first,
                                    int last, uint8_t *arena, const uint64_t *arena_offs, uint32_t slot_cap,
                                    uint8_t *branches, uint32_t bslot, uint8_t *roots, uint32_t *shard_lens,
                                    uint8_t *types) {
    int bad = 0;
    for (int i = first; i < last; ++i) {
        int type = 0;
        const uint8_t *payload = nullptr;
        size_t plen = 0, bl = 0, kl = 0;
        if (rbc_pb_decode_rbc(ring + offs[i], lens[i], &type, &payload, &plen) != RBC_OK ||
            rbc_json_decode_val(payload, plen, roots + (size_t)i * 32, branches + (size_t)i * bslot, bslot, &bl,
                                arena + arena_offs[i], slot_cap, &kl) != RBC_OK) {
            shard_lens[i] = 0;
            ++bad;
            continue;
        }
        shard_lens[i] = (uint32_t)kl;
        types[i] = (uint8_t)type;
    }
    return bad;
}

// Leg H of tools/wire_rx_bench.py: what a host does with READYs today.  One
// call takes the instances [first_inst, last_inst) of an epoch whose messages
// are ordered by instance (msg_first[i] .. msg_first[i + 1]): every READY
// through rbc_pb_decode_rbc + rbc_json_decode_ready, a per-sender dedupe into
// ready [instances][n], then the thresholds of include/rbc_protocol.h
// (rbc_dev_quorum) per instance.  verdict[m]: 0 counted, 1 rejected by the
// decoder, 2 another root.  The bench calls it from 16 threads over disjoint
// instance ranges.
extern "C" void wire_ready_host_range(const uint8_t *ring, const uint64_t *offs, const uint32_t *lens,
                                      const uint8_t *idx, const uint32_t *msg_first, int first_inst, int last_inst,
                                      const uint8_t *roots, int n, int f, int self, const uint8_t *valid,
                                      const int32_t *status, uint8_t *ready, uint8_t *verdict, uint32_t *echo_counts,
                                      uint32_t *ready_counts, uint8_t *flags) {
    for (int i = first_inst; i < last_inst; ++i) {
        uint8_t *rd = ready + (size_t)i * n;
        const uint8_t *want = roots + (size_t)i * 32;
        for (uint32_t m = msg_first[i]; m < msg_first[i + 1]; ++m) {
            int type = 0;
            const uint8_t *payload = nullptr;
            size_t plen = 0;
            uint8_t root[32];
            if (rbc_pb_decode_rbc(ring + offs[m], lens[m], &type, &payload, &plen) != RBC_OK ||
                type != RBC_MSG_READY || rbc_json_decode_ready(payload, plen, root) != RBC_OK) {
                verdict[m] = RBC_WIRE_FALLBACK;
                continue;
            }
            bool same = true;
            for (int b = 0; b < 32; ++b) same &= root[b] == want[b];
            verdict[m] = same ? RBC_WIRE_OK : RBC_WIRE_OTHER_ROOT;
            if (same) rd[idx[m]] = 1;
        }
        int E = 0, R = 0;
        for (int t = 0; t < n; ++t) {
            E += valid[(size_t)i * n + t] != 0;
            R += rd[t] != 0;
        }
        const bool ok = status[i] == RBC_OK;
        const bool have = ok && (E >= n - f || (R >= 2 * f + 1 && E >= n - 2 * f));
        const bool amplify = R >= f + 1, send_ready = amplify || have;
        if (send_ready && self >= 0 && !rd[self]) {
            rd[self] = 1;
            ++R;
        }
        const bool deliver = ok && R >= 2 * f + 1 && E >= n - 2 * f;
        echo_counts[i] = (uint32_t)E;
        ready_counts[i] = (uint32_t)R;
        flags[i] = (uint8_t)((E >= n - f ? RBC_QUORUM_ECHO : 0) | (amplify ? RBC_QUORUM_AMPLIFY : 0) |
                             (send_ready ? RBC_QUORUM_SEND_READY : 0) | (deliver ? RBC_QUORUM_DELIVER : 0));
    }
}
