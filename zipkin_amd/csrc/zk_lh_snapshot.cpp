// zk_lh_snapshot.cpp — the host side of link-histogram snapshots (include/zksketch.h,
// zk_lh_snapshot_*): validate, sum, remap and query the canonical sparse form of a per-link duration
// histogram. No device and no HIP header: a query host without a GPU answers from stored snapshots,
// and the file builds with a plain C++ compiler (tools/sanitize fuzzes it under ASan + UBSan).
//
// Every function validates its input blobs completely before it uses them, so the code after the
// validation indexes without further checks; the validation itself reads nothing past `bytes`.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "zk_guard.h"
#include "zk_lh_snapshot.h"
#include "zksketch.h"

namespace zk {

bool lh_snap_view(const void* blob, uint64_t bytes, LhSnapView* v) {
    if (!blob || bytes < sizeof(LhSnapHeader)) return false;
    const uint8_t* p = (const uint8_t*)blob;
    LhSnapHeader& h = v->h;
    memcpy(&h, p, sizeof h);
    if (h.magic != kLhSnapMagic || h.version != ZK_LH_SNAPSHOT_VERSION) return false;
    if (h.m < 2 || h.m > 7 || h.bins != lh_snap_bins(h.m)) return false;
    if (h.pad[0] || h.pad[1]) return false;
    const uint64_t body = bytes - sizeof h;
    if (h.rows > body / 16 || h.entries > body / 8 || h.rows * 16 + h.entries * 8 != body) return false;
    if (h.rows > h.entries || (h.rows == 0) != (h.entries == 0)) return false;  // a row has an entry, an entry a row
    v->rows = p + sizeof h;
    v->entries = v->rows + h.rows * 16;
    uint64_t links = 0;
    LhSnapRow prev{};
    for (uint64_t r = 0; r < h.rows; ++r) {
        const LhSnapRow row = v->row(r);
        if (r == 0) {
            if (row.first != 0) return false;
        } else {
            if (row.parent < prev.parent || (row.parent == prev.parent && row.child <= prev.child)) return false;
            if (row.first <= prev.first) return false;
        }
        if (row.first >= h.entries) return false;
        prev = row;
    }
    for (uint64_t r = 0; r < h.rows; ++r) {
        const uint64_t e0 = v->row(r).first, e1 = v->row_end(r);
        uint32_t last = 0;
        for (uint64_t i = e0; i < e1; ++i) {
            const uint64_t e = v->entry(i);
            const uint32_t bin = (uint32_t)(e >> 32), count = (uint32_t)e;
            if (bin >= h.bins || count == 0 || (i > e0 && bin <= last)) return false;
            last = bin;
            links += count;
        }
    }
    return links == h.links;
}

namespace {

// a snapshot under construction: rows in canonical order with their entries appended in order
struct Builder {
    uint32_t m = 4;
    uint64_t dropped = 0, links = 0;
    std::vector<LhSnapRow> rows;
    std::vector<uint64_t> entries;

    void begin_row(uint32_t parent, uint32_t child) { rows.push_back(LhSnapRow{parent, child, (uint64_t)entries.size()}); }
    void add(uint32_t bin, uint64_t count) {
        entries.push_back(((uint64_t)bin << 32) | count);
        links += count;
    }
    // two-phase output (zk_lh_snapshot): the size, then the bytes when they fit
    zk_status emit(void* out, uint64_t cap, uint64_t* bytes_out) const {
        const uint64_t size = sizeof(LhSnapHeader) + rows.size() * 16ull + entries.size() * 8ull;
        *bytes_out = size;
        if (!out) return ZK_OK;
        if (cap < size) return ZK_ERR_CAPACITY;
        LhSnapHeader h{};
        h.magic = kLhSnapMagic;
        h.version = ZK_LH_SNAPSHOT_VERSION;
        h.m = m;
        h.bins = lh_snap_bins(m);
        h.rows = rows.size();
        h.entries = entries.size();
        h.links = links;
        h.dropped = dropped;
        uint8_t* p = (uint8_t*)out;
        memcpy(p, &h, sizeof h);
        if (!rows.empty()) memcpy(p + sizeof h, rows.data(), rows.size() * 16);
        if (!entries.empty()) memcpy(p + sizeof h + rows.size() * 16, entries.data(), entries.size() * 8);
        return ZK_OK;
    }
};

bool row_less(const LhSnapRow& a, const LhSnapRow& b) {
    return a.parent < b.parent || (a.parent == b.parent && a.child < b.child);
}

void copy_row(const LhSnapView& v, uint64_t r, Builder* out) {
    const LhSnapRow row = v.row(r);
    out->begin_row(row.parent, row.child);
    for (uint64_t i = row.first, e1 = v.row_end(r); i < e1; ++i) {
        const uint64_t e = v.entry(i);
        out->add((uint32_t)(e >> 32), (uint32_t)e);
    }
}

// [lo, hi] of a bin (zk_lh.hip lh_bin_bounds, oracle/realtime.py bin_bounds)
void bin_bounds(uint32_t b, uint32_t m, int64_t* lo, int64_t* hi) {
    if (b < (1u << m)) {
        *lo = *hi = (int64_t)b;
        return;
    }
    const uint32_t g = b >> m, mant = b & ((1u << m) - 1u);
    const uint32_t e = g + m - 1u;
    *lo = (int64_t)(((1ull << m) | mant) << (e - m));
    *hi = *lo + (int64_t)(1ull << (e - m)) - 1;
}

}  // namespace
}  // namespace zk

using namespace zk;

extern "C" {

zk_status zk_lh_snapshot_validate(const void* blob, uint64_t bytes) {
    ZK_GUARD_BEGIN
    LhSnapView v;
    return lh_snap_view(blob, bytes, &v) ? ZK_OK : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

zk_status zk_lh_snapshot_plus(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes, void* out,
                              uint64_t cap, uint64_t* bytes_out) {
    ZK_GUARD_BEGIN
    if (!bytes_out) return ZK_ERR_INVALID_ARG;
    LhSnapView va, vb;
    if (!lh_snap_view(a, a_bytes, &va) || !lh_snap_view(b, b_bytes, &vb)) return ZK_ERR_INVALID_ARG;
    if (va.h.m != vb.h.m) return ZK_ERR_INVALID_ARG;
    Builder res;
    res.m = va.h.m;
    res.dropped = va.h.dropped + vb.h.dropped;
    res.rows.reserve((size_t)std::max(va.h.rows, vb.h.rows));
    res.entries.reserve((size_t)std::max(va.h.entries, vb.h.entries));
    uint64_t ra = 0, rb = 0;
    while (ra < va.h.rows || rb < vb.h.rows) {
        if (rb == vb.h.rows || (ra < va.h.rows && row_less(va.row(ra), vb.row(rb)))) {
            copy_row(va, ra++, &res);
            continue;
        }
        if (ra == va.h.rows || row_less(vb.row(rb), va.row(ra))) {
            copy_row(vb, rb++, &res);
            continue;
        }
        // the same (parent, child) in both: the entries merged by bin
        const LhSnapRow row = va.row(ra);
        res.begin_row(row.parent, row.child);
        uint64_t ia = row.first, ib = vb.row(rb).first;
        const uint64_t ea = va.row_end(ra), eb = vb.row_end(rb);
        while (ia < ea || ib < eb) {
            const uint64_t xa = ia < ea ? va.entry(ia) : ~0ull, xb = ib < eb ? vb.entry(ib) : ~0ull;
            const uint32_t ba = (uint32_t)(xa >> 32), bb = (uint32_t)(xb >> 32);  // (0xFFFFFFFF: exhausted, above every bin)
            if (ba < bb) {
                res.add(ba, (uint32_t)xa);
                ++ia;
            } else if (bb < ba) {
                res.add(bb, (uint32_t)xb);
                ++ib;
            } else {
                const uint64_t sum = (uint64_t)(uint32_t)xa + (uint32_t)xb;
                if (sum > kLhCounterMax) return ZK_ERR_CAPACITY;  // a u32 counter of the table would wrap
                res.add(ba, sum);
                ++ia;
                ++ib;
            }
        }
        ++ra;
        ++rb;
    }
    return res.emit(out, cap, bytes_out);
    ZK_GUARD_END
}

zk_status zk_lh_snapshot_remap(const void* in, uint64_t bytes, const uint32_t* map, uint32_t n_map, void* out,
                               uint64_t cap, uint64_t* bytes_out) {
    ZK_GUARD_BEGIN
    if (!bytes_out || (n_map && !map)) return ZK_ERR_INVALID_ARG;
    LhSnapView v;
    if (!lh_snap_view(in, bytes, &v)) return ZK_ERR_INVALID_ARG;
    std::vector<LhSnapRow> moved((size_t)v.h.rows);  // the new ids; first = the row's index in the input
    for (uint64_t r = 0; r < v.h.rows; ++r) {
        const LhSnapRow row = v.row(r);
        if (row.parent >= n_map || row.child >= n_map) return ZK_ERR_SERVICE_RANGE;
        moved[(size_t)r] = LhSnapRow{map[row.parent], map[row.child], r};
    }
    std::sort(moved.begin(), moved.end(), row_less);
    for (size_t r = 1; r < moved.size(); ++r)
        if (!row_less(moved[r - 1], moved[r])) return ZK_ERR_INVALID_ARG;  // two rows on one (parent, child)
    Builder res;
    res.m = v.h.m;
    res.dropped = v.h.dropped;
    res.rows.reserve(moved.size());
    res.entries.reserve((size_t)v.h.entries);
    for (const LhSnapRow& mv : moved) {
        res.begin_row(mv.parent, mv.child);
        for (uint64_t i = v.row(mv.first).first, e1 = v.row_end(mv.first); i < e1; ++i) {
            const uint64_t e = v.entry(i);
            res.add((uint32_t)(e >> 32), (uint32_t)e);
        }
    }
    return res.emit(out, cap, bytes_out);
    ZK_GUARD_END
}

zk_status zk_lh_snapshot_quantiles(const void* blob, uint64_t bytes, const double* q, uint32_t nq, int64_t* lo,
                                   int64_t* hi, uint64_t* count) {
    ZK_GUARD_BEGIN
    LhSnapView v;
    if (!lh_snap_view(blob, bytes, &v)) return ZK_ERR_INVALID_ARG;
    if (nq && (!q || !lo || !hi)) return ZK_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < nq; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return ZK_ERR_INVALID_ARG;
    for (uint64_t r = 0; r < v.h.rows; ++r) {
        const uint64_t e0 = v.row(r).first, e1 = v.row_end(r);
        uint64_t N = 0;
        for (uint64_t i = e0; i < e1; ++i) N += (uint32_t)v.entry(i);
        if (count) count[r] = N;
        for (uint32_t k = 0; k < nq; ++k) {
            uint64_t rank = (uint64_t)ceil(q[k] * (double)N);  // nearest rank, 1-based (zk_lh_quantiles)
            if (rank < 1) rank = 1;
            if (rank > N) rank = N;
            uint64_t cum = 0;
            for (uint64_t i = e0; i < e1; ++i) {
                const uint64_t e = v.entry(i);
                cum += (uint32_t)e;
                if (cum >= rank) {
                    bin_bounds((uint32_t)(e >> 32), v.h.m, &lo[r * nq + k], &hi[r * nq + k]);
                    break;
                }
            }
        }
    }
    return ZK_OK;
    ZK_GUARD_END
}

}  // extern "C"
