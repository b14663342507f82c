// zk_td_select.h — the order key and the host steps of zk_td_top's radix select (zk_td.hip).
//
// An entry of the select is a table slot's three words with the traceId itself in the first. Its
// composite key is 128 bits, smallest first: hi = the order key (duration or start with the sign bit
// flipped, complemented for the DESC orders), lo = the traceId (ascending in all four orders).
// Everything here is plain C++ (ZK_HD marks what the kernels share), so the host steps compile and
// run without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "zk_tracegen.h"  // ZK_HD
#include "zkduration.h"

namespace zk {

constexpr uint64_t kTdSign = 1ull << 63;
constexpr uint32_t kTdBins = 4096;   // 12 bits per round
constexpr uint32_t kTdDigitBits = 12;

struct TdEntry {
    uint64_t id;    // the traceId (in the table: the slot's key word)
    uint64_t skey;  // start ^ sign
    uint64_t ekey;  // end ^ sign
};

// duration = (uint64)end - (uint64)start; the two sign flips cancel in the difference
ZK_HD uint64_t td_duration(uint64_t skey, uint64_t ekey) { return ekey - skey; }

// the 64-bit order key: smallest first
ZK_HD uint64_t td_order_key(uint32_t order, uint64_t skey, uint64_t ekey) {
    const uint64_t v = order == ZK_TD_DURATION_ASC || order == ZK_TD_DURATION_DESC
                           ? td_duration(skey, ekey) ^ kTdSign
                           : skey;
    return order == ZK_TD_DURATION_DESC || order == ZK_TD_TIMESTAMP_DESC ? ~v : v;
}

// bits [shift, shift + 12) of the 128-bit key hi:lo; shift is 0..116
ZK_HD uint32_t td_digit(uint64_t hi, uint64_t lo, uint32_t shift) {
    uint64_t v;
    if (shift >= 64)
        v = hi >> (shift - 64);
    else if (shift == 0)
        v = lo;
    else
        v = (lo >> shift) | (hi << (64 - shift));
    return (uint32_t)v & (kTdBins - 1);
}

// The round's shift from the bits in which the keys differ (diff_hi:diff_lo, not both zero): the 12-bit
// digit whose top bit is the highest differing bit, so that the histogram always splits the keys.
inline uint32_t td_shift_of(uint64_t diff_hi, uint64_t diff_lo) {
    const uint32_t p = diff_hi ? 127u - (uint32_t)__builtin_clzll(diff_hi) : 63u - (uint32_t)__builtin_clzll(diff_lo);
    return p >= kTdDigitBits - 1 ? p - (kTdDigitBits - 1) : 0u;
}

// The bin in which the running count of hist crosses k (k >= 1, the counts sum to k or more): *below =
// the entries of the bins before it.
inline uint32_t td_pick_bin(const uint32_t* hist, uint64_t k, uint64_t* below) {
    uint64_t run = 0;
    for (uint32_t b = 0; b < kTdBins; ++b) {
        if (run + hist[b] >= k) {
            *below = run;
            return b;
        }
        run += hist[b];
    }
    *below = run;
    return kTdBins;
}

// The survivors (n of them, in any order) sorted by the composite key; the first min(k, n) are written
// to the caller's arrays. Returns how many.
inline uint32_t td_emit(TdEntry* e, size_t n, uint32_t order, uint32_t k, uint64_t* trace_id, int64_t* start,
                        int64_t* duration) {
    std::sort(e, e + n, [order](const TdEntry& a, const TdEntry& b) {
        const uint64_t ka = td_order_key(order, a.skey, a.ekey), kb = td_order_key(order, b.skey, b.ekey);
        return ka != kb ? ka < kb : a.id < b.id;
    });
    const uint32_t m = (uint32_t)std::min<size_t>(n, k);
    for (uint32_t i = 0; i < m; ++i) {
        trace_id[i] = e[i].id;
        start[i] = (int64_t)(e[i].skey ^ kTdSign);
        duration[i] = (int64_t)td_duration(e[i].skey, e[i].ekey);
    }
    return m;
}

}  // namespace zk
