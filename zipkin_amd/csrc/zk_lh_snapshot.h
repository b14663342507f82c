// zk_lh_snapshot.h — the byte layout of a link-histogram snapshot (include/zksketch.h), shared by the
// host functions (zk_lh_snapshot.cpp, no HIP) and the device compaction and merge (zk_lh.hip).
// Fields are read and written with memcpy: a blob has no alignment.
#pragma once
#include <stdint.h>
#include <string.h>

namespace zk {

struct LhSnapHeader {  // 64 bytes, little-endian
    uint32_t magic, version, m, bins;
    uint64_t rows, entries, links, dropped;
    uint64_t pad[2];
};
struct LhSnapRow {  // 16 bytes
    uint32_t parent, child;
    uint64_t first;
};
static_assert(sizeof(LhSnapHeader) == 64 && sizeof(LhSnapRow) == 16, "snapshot layout");

constexpr uint32_t kLhSnapMagic = 0x484C4B5Au;  // "ZKLH"
constexpr uint64_t kLhCounterMax = 0xFFFFFFFFull;

inline uint32_t lh_snap_bins(uint32_t m) { return (41u - m) << m; }

// a validated blob: where its parts are
struct LhSnapView {
    LhSnapHeader h;
    const uint8_t* rows;     // h.rows x 16 B
    const uint8_t* entries;  // h.entries x 8 B
    LhSnapRow row(uint64_t i) const {
        LhSnapRow r;
        memcpy(&r, rows + i * 16, 16);
        return r;
    }
    uint64_t entry(uint64_t i) const {
        uint64_t e;
        memcpy(&e, entries + i * 8, 8);
        return e;
    }
    uint64_t row_end(uint64_t i) const { return i + 1 < h.rows ? row(i + 1).first : h.entries; }
};

// the view of a blob that zk_lh_snapshot_validate accepts (false: malformed, *v unspecified)
bool lh_snap_view(const void* blob, uint64_t bytes, LhSnapView* v);

}  // namespace zk
