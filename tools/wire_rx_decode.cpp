// wire_rx_decode.cpp -- leg A of tools/wire_rx_bench.py: the host decode the
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
