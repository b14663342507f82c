// zk_ix_select.h — the host steps of the trace-id index (zk_ix.hip): the plan of a service's slices,
// the final sort of zk_ix_trace_ids and the name ids of zk_ix_span_names' bitmap.
//
// An entry of the select is 16 B: tkey = ts with the sign bit flipped, and the traceId. Its composite
// key is 128 bits, smallest first: hi = ~tkey (newest first), lo = the traceId (ascending). The digit,
// shift and bin steps are zk_td_select.h's, unchanged. Everything here is plain C++, so it compiles and
// runs without a device (tools/ix_select_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "zk_td_select.h"

namespace zk {

constexpr uint32_t kIxNameWords = 65536 / 32;  // zk_ix_span_names' bitmap: one bit per name id

struct IxEntry {
    uint64_t tkey;  // ts ^ sign
    uint64_t id;    // the traceId
};

// where one service's entries lie in one segment
struct IxSpan {
    uint32_t segment;
    uint64_t start, count;  // entries [start, start + count) of the segment's columns
};

// The non-empty slices of `service`, in segment order; offsets[g] points at segment g's
// num_services + 1 offsets. Returns the entries they hold.
inline uint64_t ix_plan(const uint64_t* const* offsets, uint32_t segments, uint32_t service, std::vector<IxSpan>* out) {
    uint64_t total = 0;
    out->clear();
    for (uint32_t g = 0; g < segments; ++g) {
        const uint64_t a = offsets[g][service], b = offsets[g][service + 1];
        if (b > a) {
            out->push_back(IxSpan{g, a, b - a});
            total += b - a;
        }
    }
    return total;
}

// The survivors (n of them, in any order) sorted by the composite key, followed in that order by
// `copies` entries equal to `same` (the equal-keys end of the select: every key of the survivors is
// smaller than `same` or equal to it); the first min(limit, n + copies) are written. Returns how many.
inline uint32_t ix_emit(IxEntry* e, size_t n, IxEntry same, uint64_t copies, uint32_t limit, uint64_t* trace_id, int64_t* ts) {
    std::sort(e, e + n, [](const IxEntry& a, const IxEntry& b) { return a.tkey != b.tkey ? a.tkey > b.tkey : a.id < b.id; });
    const uint32_t m = (uint32_t)std::min<uint64_t>((uint64_t)n + copies, limit);
    for (uint32_t i = 0; i < m; ++i) {
        const IxEntry& x = i < n ? e[i] : same;
        trace_id[i] = x.id;
        ts[i] = (int64_t)(x.tkey ^ kTdSign);
    }
    return m;
}

// The set bits of the bitmap except bit 0, ascending, into out (when it holds `cap`); returns their number.
inline uint32_t ix_names_of(const uint32_t* bitmap, uint16_t* out, uint32_t cap) {
    uint32_t n = 0;
    for (uint32_t w = 0; w < kIxNameWords; ++w)
        for (uint32_t word = bitmap[w] & (w ? ~0u : ~1u); word; word &= word - 1) {
            const uint32_t id = w * 32 + (uint32_t)__builtin_ctz(word);
            if (n < cap && out) out[n] = (uint16_t)id;
            ++n;
        }
    return n;
}

}  // namespace zk
