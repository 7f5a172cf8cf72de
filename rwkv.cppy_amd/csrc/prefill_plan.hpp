// prefill_plan.hpp -- the host planner of batched prefill (Engine::prefill_batch): plain C++, no
// device call, so it is tested on its own (rwkv_mi355x_selftest_prefill_plan; tests/prefill_plan_host.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace rwkvmi {

// Packs n_rows prompts of lengths[i] >= 1 tokens, in order, into chunks of at most cap tokens; every
// chunk but the last is full.  A row that crosses a chunk boundary is split: segment j is seg_len[j]
// tokens of row seg_row[j], from token seg_begin[j] of chunk seg_chunk[j] on; a row's segments follow
// each other, in consecutive chunks.  Returns the number of segments (at most n_rows + chunks - 1),
// -1 when there are more than max_segs of them (nothing past max_segs is written), -2 for no rows,
// cap == 0 or a zero length.
inline long long prefill_plan(const size_t * lengths, size_t n_rows, size_t cap, uint32_t * seg_row, uint32_t * seg_begin,
                              uint32_t * seg_len, uint32_t * seg_chunk, size_t max_segs) {
    if (!lengths || n_rows == 0 || cap == 0) return -2;
    for (size_t i = 0; i < n_rows; i++)
        if (lengths[i] == 0) return -2;
    size_t n = 0, pos = 0, chunk = 0;
    for (size_t i = 0; i < n_rows; i++) {
        size_t rem = lengths[i];
        while (rem) {
            const size_t take = rem < cap - pos ? rem : cap - pos;
            if (n >= max_segs) return -1;
            seg_row[n] = (uint32_t)i;
            seg_begin[n] = (uint32_t)pos;
            seg_len[n] = (uint32_t)take;
            seg_chunk[n] = (uint32_t)chunk;
            n++;
            rem -= take;
            pos += take;
            if (pos == cap) pos = 0, chunk++;
        }
    }
    return (long long)n;
}

}  // namespace rwkvmi
