// zk_an.hip — the annotation store by trace id (include/zkannots.h): segments of 44-B annotation rows
// grouped by the span store's 12-bit hash of the trace id in HBM, and the lookup of asked traces' rows.
//
// A segment is one allocation of seven columns, trace_id, span_id, ts, value [8 B], ipv4, service_id,
// bits [4 B], each 256-B aligned, then off[4097] (u32): the entries of bucket b lie at [off[b], off[b + 1]).
// The host keeps the same offsets. The plan is zk_sp.hip's, kernel for kernel; this file shares none of its
// code, so the span store's kernels stay as they were.
//
//   k_an_count    the batch's rows per bucket: a per-workgroup LDS histogram of 4096 bins (16 KB), lanes of
//                 a wave that share a bin added once, flushed with atomics. 8 B per row.
//   (host)        the counts' exclusive scan = the segment's offsets; they also start the cursors.
//   k_an_scatter  a workgroup owns a stretch of the batch and walks it twice: an LDS histogram of its rows'
//                 buckets, ONE returning atomic per workgroup and bucket with rows to claim that many places
//                 behind the bucket's cursor, then every row again, its rank inside the workgroup from LDS
//                 (32 KB of LDS, so five workgroups share a CU). trace_id is read twice, 44 B per row read
//                 and 44 B written.
//   k_an_merge    one old segment's entries into the merged one: an entry's bucket from its trace id, its
//                 place = the bucket's base for this segment + the entry's index in the old slice.
//   k_an_find_count, k_an_find_write   zk_an_gather's passes: a workgroup per (asked id, segment, part of
//                 the slice) walks the trace_id slice of the id's bucket; the write pass appends a wave's
//                 matching rows behind the asked id's offset with one returning atomic per wave. Nothing of
//                 a trace is held in LDS: a trace may be of any length.
//   k_an_end_fold, k_an_end_pins, k_an_end_mark, k_an_expire_rewrite   zk_an_expire's passes: per range of
//                 buckets a scratch table {trace id, end} is folded from trace_id and ts (16 B per entry), the
//                 pinned ids get their verdicts, every entry gets one mark bit and the survivors are counted
//                 per (segment, bucket); then the survivors of the mixed segments are scattered, as
//                 k_an_scatter does, into one new segment.
//
// Every store is bounded: the scatter and the merge drop a place outside the bucket's slice of the segment
// they write (it cannot arise while the columns stay as they were between the count and the scatter, which
// the header asks of the caller), the lookups clamp a slice to its segment and drop a row at or past its
// asked id's count or the output's size, and the expiry's probes stay inside their table (at most `slots`
// steps), its mark words inside the segment's and its rewrite inside the new segment's slices.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "zk_guard.h"
#include "zk_hist.h"
#include "zk_launch.h"
#include "zk_sp_staged.h"
#include "zk_tracegen.h"
#include "zkannots.h"
#include "zkbinannots.h"
#include "zkingest.h"

namespace zk {
namespace {

constexpr int kAnWG = 256;
constexpr uint32_t kAnBins = ZK_AN_BUCKETS;
constexpr uint32_t kAnMaxGrid = 4096;
constexpr uint32_t kAnHistGrid = 1024;        // k_an_count: every workgroup flushes up to 4096 bins
constexpr uint32_t kAnScatterPerWG = 16384;   // k_an_scatter: rows per workgroup at least (4096 atomics each at most)
constexpr uint64_t kAnMaxEntries = 0xFFFFFFFFull;
constexpr int kAnCntItems = 4;                // k_an_count: rows per thread and step
constexpr uint32_t kAnCntTile = kAnWG * kAnCntItems;
constexpr uint32_t kAnPart = 4096;            // the lookups: a slice longer than this is split over workgroups
constexpr uint32_t kAnMaxParts = 64;
constexpr uint64_t kAnMaxFindGrid = 1ull << 20;
constexpr unsigned long long kAnSalt = ZK_SP_SALT;   // the span store's bucket function, on purpose
constexpr unsigned long long kAnEndSalt = ZK_SP_END_SALT;  // the expiry's scratch table: apart from the bucket salt
constexpr unsigned long long kAnSign = 1ull << 63;   // ts ^ sign: the unsigned order is the signed one
constexpr unsigned long long kAnNone = ~0ull;
constexpr uint64_t kAnExpireChunk = 1ull << 24;      // zk_an_config.expire_chunk's default
constexpr uint64_t kAnEndMinSlots = 1024;
constexpr uint32_t kAnEndGrid = 4096;                // the end-table passes: workgroups per segment at most
constexpr uint32_t kAnMaxItems = 4096;               // the rewrite's work items at most, plus one per segment

static_assert(kAnBins == 4096 && ZK_AN_BUCKETS == ZK_SP_BUCKETS, "the bucket is the span store's: the hash's 12 highest bits");
static_assert(ZK_AN_ROW_BYTES == 4 * 8 + 3 * 4, "a row's seven columns");
static_assert(sizeof(zk_an_cols) == 56 && sizeof(zk_an_config) == 48, "the ABI's layouts");
static_assert(kAnEndSalt != kAnSalt, "a range's ids share the bucket hash's high bits");
static_assert(kAnScatterPerWG % kAnWG == 0 && kAnWG % 64 == 0, "a wave's 64 entries share a mark word");

__host__ __device__ inline uint32_t an_bucket(unsigned long long id) { return (uint32_t)(zk_mix64(id ^ kAnSalt) >> 52); }

// a segment's columns and offsets as the kernels see them (const), or as the scatter and the merge write them
struct AnCols {
    unsigned long long* tid;
    unsigned long long* span;
    long long* ts;
    unsigned long long* val;
    uint32_t* ip;
    uint32_t* svc;
    uint32_t* bits;
    uint32_t* off;  // [kAnBins + 1] (a segment), or nullptr (a batch, the lookups' output)
    unsigned long long n;
};
static_assert(sizeof(AnCols) == 72, "the segment table's stride");

// the lookups' block: the asked ids, their counts, the write pass's cursors, the rows' bases, the segments
constexpr size_t kQIdsAt = 0;
constexpr size_t kQCountsAt = kQIdsAt + ZK_AN_MAX_IDS * 8;
constexpr size_t kQCursorAt = kQCountsAt + ZK_AN_MAX_IDS * 4;
constexpr size_t kQBaseAt = kQCursorAt + ZK_AN_MAX_IDS * 4;
constexpr size_t kQSegsAt = kQBaseAt + ZK_AN_MAX_IDS * 8;
constexpr size_t kQBytes = kQSegsAt + ZK_AN_MAX_SEGMENTS * sizeof(AnCols);
// the observe's block: the counts, then the cursors
constexpr size_t kObsCursorAt = kAnBins * 4;
constexpr size_t kObsBytes = 2 * kAnBins * 4;
// the expiry's block: the segments (80 B each), the survivors [segment][bucket], the new segment's
// cursors, the full-table counter, the pins (ids ascending, cuts, verdicts), the rewrite's work items
constexpr size_t kXSegsAt = 0;
constexpr size_t kXSurvAt = kXSegsAt + ZK_AN_MAX_SEGMENTS * 80;
constexpr size_t kXCursorAt = kXSurvAt + (size_t)ZK_AN_MAX_SEGMENTS * kAnBins * 4;
constexpr size_t kXFullAt = kXCursorAt + kAnBins * 4;
constexpr size_t kXPinIdsAt = kXFullAt + 256;
constexpr size_t kXPinCutsAt = kXPinIdsAt + ZK_AN_MAX_PINS * 8;
constexpr size_t kXVerdictAt = kXPinCutsAt + ZK_AN_MAX_PINS * 8;
constexpr size_t kXItemsAt = kXVerdictAt + ZK_AN_MAX_PINS * 4;
constexpr size_t kXBytes = kXItemsAt + (size_t)(kAnMaxItems + ZK_AN_MAX_SEGMENTS) * 8;
static_assert(kXSurvAt % 256 == 0 && kXPinIdsAt % 256 == 0 && kXItemsAt % 8 == 0, "the expiry block's alignment");

uint32_t an_grid(uint64_t items, uint32_t cap = kAnMaxGrid) {
    const uint64_t g = (items + kAnWG - 1) / kAnWG;
    return (uint32_t)(g < 1 ? 1 : g > cap ? cap : g);
}

// ---- observe -------------------------------------------------------------------------------------------
// counts[b] += the rows of bucket b. The loop's bounds are the same for all threads of a workgroup, so
// every lane reaches the ballots.
__global__ __launch_bounds__(kAnWG) void k_an_count(const unsigned long long* __restrict__ tid, unsigned long long n,
                                                    uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_hist[kAnBins];
    for (uint32_t b = threadIdx.x; b < kAnBins; b += kAnWG) s_hist[b] = 0u;
    __syncthreads();
    const unsigned long long stride = (unsigned long long)gridDim.x * kAnCntTile;
    for (unsigned long long base = (unsigned long long)blockIdx.x * kAnCntTile; base < n; base += stride) {
        unsigned long long t[kAnCntItems];  // (the tile's loads first, then the ballots)
#pragma unroll
        for (int j = 0; j < kAnCntItems; ++j) {
            const unsigned long long i = base + (unsigned long long)j * kAnWG + threadIdx.x;
            t[j] = i < n ? tid[i] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < kAnCntItems; ++j)
            hist_add(s_hist, base + (unsigned long long)j * kAnWG + threadIdx.x < n, an_bucket(t[j]));
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kAnBins; b += kAnWG) {
        const uint32_t c = s_hist[b];
        if (c) atomicAdd(&counts[b], c);
    }
}

// Workgroup w owns rows [w * chunk, (w + 1) * chunk) (chunk a multiple of the workgroup). cursor[b] starts
// at the segment's off[b]; a place at or past off[b + 1] is dropped.
__global__ __launch_bounds__(kAnWG) void k_an_scatter(AnCols in, unsigned long long chunk, uint32_t* __restrict__ cursor, AnCols out) {
    __shared__ uint32_t s_cnt[kAnBins];   // the stretch's rows per bucket, then the ranks given out
    __shared__ uint32_t s_base[kAnBins];  // where the workgroup's places of a bucket begin
    const unsigned long long lo = (unsigned long long)blockIdx.x * chunk;
    const unsigned long long hi = lo + chunk < in.n ? lo + chunk : in.n;
    for (uint32_t b = threadIdx.x; b < kAnBins; b += kAnWG) s_cnt[b] = 0u;
    __syncthreads();
    for (unsigned long long base = lo; base < hi; base += kAnCntTile) {
        unsigned long long t[kAnCntItems];
#pragma unroll
        for (int j = 0; j < kAnCntItems; ++j) {
            const unsigned long long i = base + (unsigned long long)j * kAnWG + threadIdx.x;
            t[j] = i < hi ? in.tid[i] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < kAnCntItems; ++j)
            hist_add(s_cnt, base + (unsigned long long)j * kAnWG + threadIdx.x < hi, an_bucket(t[j]));
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kAnBins; b += kAnWG) {
        const uint32_t c = s_cnt[b];
        s_base[b] = c ? atomicAdd(&cursor[b], c) : 0u;
        s_cnt[b] = 0u;
    }
    __syncthreads();
    for (unsigned long long base = lo; base < hi; base += kAnWG) {
        const unsigned long long i = base + threadIdx.x;
        const bool valid = i < hi;
        const unsigned long long t = valid ? in.tid[i] : 0ull;
        const uint32_t b = an_bucket(t);
        const uint32_t rank = hist_rank(s_cnt, valid, b);
        if (valid) {
            const unsigned long long at = (unsigned long long)s_base[b] + rank;
            if (at < (unsigned long long)out.off[b + 1] && at < out.n) {
                out.tid[at] = t;
                out.span[at] = in.span[i];
                out.ts[at] = in.ts[i];
                out.val[at] = in.val[i];
                out.ip[at] = in.ip[i];
                out.svc[at] = in.svc[i];
                out.bits[at] = in.bits[i];
            }
        }
    }
}

// dst_base[b]: where this old segment's slice of bucket b begins in the merged segment
__global__ __launch_bounds__(kAnWG) void k_an_merge(AnCols src, const uint32_t* __restrict__ dst_base, AnCols dst) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kAnWG;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kAnWG + threadIdx.x; i < src.n; i += stride) {
        const unsigned long long t = src.tid[i];
        const uint32_t b = an_bucket(t);
        const unsigned long long so = src.off[b];
        if (i < so || i >= (unsigned long long)src.off[b + 1]) continue;  // (not in its bucket's slice: never a scattered entry)
        const unsigned long long at = (unsigned long long)dst_base[b] + (i - so);
        if (at < (unsigned long long)dst.off[b + 1] && at < dst.n) {
            dst.tid[at] = t;
            dst.span[at] = src.span[i];
            dst.ts[at] = src.ts[i];
            dst.val[at] = src.val[i];
            dst.ip[at] = src.ip[i];
            dst.svc[at] = src.svc[i];
            dst.bits[at] = src.bits[i];
        }
    }
}

// ---- the lookups ---------------------------------------------------------------------------------------
// The grid: x the asked id, y the segment, z the part of the slice. [*a, *e) = this workgroup's stretch of
// the trace_id slice of the id's bucket, clamped to the segment; false when it is empty. The same for all
// threads of a workgroup.
__device__ inline bool an_stretch(const AnCols& sg, unsigned long long id, unsigned long long* a, unsigned long long* e) {
    const uint32_t b = an_bucket(id);
    unsigned long long lo = sg.off[b], hi = sg.off[b + 1];
    if (hi > sg.n) hi = sg.n;
    if (lo >= hi) return false;
    const unsigned long long parts = gridDim.z;
    const unsigned long long part = (((hi - lo) + parts - 1) / parts + kAnWG - 1) / kAnWG * kAnWG;
    *a = lo + (unsigned long long)blockIdx.z * part;
    if (*a >= hi) return false;
    *e = *a + part < hi ? *a + part : hi;
    return true;
}

// counts[q] += the entries of segment blockIdx.y whose trace id is ids[q]
__global__ __launch_bounds__(kAnWG) void k_an_find_count(const AnCols* __restrict__ segs, const unsigned long long* __restrict__ ids,
                                                         uint32_t* __restrict__ counts) {
    const AnCols sg = segs[blockIdx.y];
    const unsigned long long id = ids[blockIdx.x];
    unsigned long long a, e;
    if (!an_stretch(sg, id, &a, &e)) return;
    uint32_t c = 0;
    for (unsigned long long i = a + threadIdx.x; i < e; i += kAnWG) c += sg.tid[i] == id ? 1u : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if (lane_id() == 0 && c) atomicAdd(&counts[blockIdx.x], c);
}

// The matching rows behind base[q]: a wave draws its matches' places with one returning atomic on cursor[q]
// (from 0); a place at or past counts[q], or a row at or past out.n, is dropped. The loop's bounds are the
// same for all threads of a workgroup, so every lane reaches the ballot and the shuffle.
__global__ __launch_bounds__(kAnWG) void k_an_find_write(const AnCols* __restrict__ segs, const unsigned long long* __restrict__ ids,
                                                         const uint32_t* __restrict__ counts, uint32_t* __restrict__ cursor,
                                                         const unsigned long long* __restrict__ base, AnCols out) {
    const AnCols sg = segs[blockIdx.y];
    const uint32_t q = blockIdx.x;
    const unsigned long long id = ids[q];
    unsigned long long a, e;
    if (!an_stretch(sg, id, &a, &e)) return;
    const uint32_t limit = counts[q];
    const unsigned long long row0 = base[q];
    for (unsigned long long tile = a; tile < e; tile += kAnWG) {
        const unsigned long long i = tile + threadIdx.x;
        const bool hit = i < e && sg.tid[i] == id;
        const unsigned long long m = __ballot(hit);
        if (!m) continue;  // (wave-uniform)
        const int lead = __ffsll((long long)m) - 1;
        uint32_t first = 0;
        if ((int)lane_id() == lead) first = atomicAdd(&cursor[q], (uint32_t)__popcll(m));
        first = __shfl(first, lead);
        if (hit) {
            const unsigned long long r = (unsigned long long)first + rank_in(m);
            const unsigned long long at = row0 + r;
            if (r < limit && at < out.n) {
                out.tid[at] = id;
                out.span[at] = sg.span[i];
                out.ts[at] = sg.ts[i];
                out.val[at] = sg.val[i];
                out.ip[at] = sg.ip[i];
                out.svc[at] = sg.svc[i];
                out.bits[at] = sg.bits[i];
            }
        }
    }
}

// ---- expiry --------------------------------------------------------------------------------------------
// A segment as the expiry's passes see it: its columns and where its mark words begin.
struct AnXSeg {
    AnCols c;
    unsigned long long mark_at;
};
struct AnItem {
    uint32_t seg, chunk;
};
static_assert(sizeof(AnXSeg) == 80 && sizeof(AnItem) == 8, "the expiry plan's layouts");

__device__ inline unsigned long long an_end_home(unsigned long long id, unsigned long long slots) {
    return zk_mix64(id ^ kAnEndSalt) & (slots - 1ull);
}

// [*lo, *hi): the slice of buckets [b0, b1) (b0 < b1 <= kAnBins) in the segment, clamped to it
__device__ inline void an_range(const AnCols& sg, uint32_t b0, uint32_t b1, unsigned long long* lo, unsigned long long* hi) {
    unsigned long long a = sg.off[b0], e = sg.off[b1];
    if (e > sg.n) e = sg.n;
    if (a > e) a = e;
    *lo = a;
    *hi = e;
}

// The slot of `id` in the scratch table (slots a power of two; tab[2 * s] the key, tab[2 * s + 1] the end;
// trace id 0 has the slot behind the table, its key held as 1), or kAnNone when it is not there. A probe
// ends at an empty slot or after `slots` steps.
__device__ inline unsigned long long an_end_find(const unsigned long long* tab, unsigned long long slots, unsigned long long id) {
    if (id == 0ull) return tab[2 * slots] != 0ull ? slots : kAnNone;
    unsigned long long s = an_end_home(id, slots);
    for (unsigned long long tries = 0; tries < slots; ++tries) {
        const unsigned long long k = tab[2 * s];
        if (k == id) return s;
        if (k == 0ull) return kAnNone;
        s = (s + 1ull) & (slots - 1ull);
    }
    return kAnNone;
}

// end[trace] = max over the entries of the range's slices of ts ^ sign (every row is timed; the table is
// cleared to zeros, the key of INT64_MIN). grid.y = the segment. A wave owns rows of 64 consecutive entries
// and folds each RUN of equal trace ids in a row first (a segmented max over the lanes, log2 steps): only
// a run's first lane goes to the table. One span's annotations are adjacent in a batch and the scatter
// keeps a batch's neighbours neighbours inside a bucket's slice, so runs are the common case. The plain
// loads are hints: a key never changes once claimed and an end only rises, so a stale word costs an atomic,
// never an answer. A table that ran full (it cannot at load <= 1/2) is counted in *full. The rows' bounds
// are wave-uniform, so every lane reaches the shuffles.
__global__ __launch_bounds__(kAnWG) void k_an_end_fold(const AnXSeg* __restrict__ segs, uint32_t b0, uint32_t b1,
                                                       unsigned long long* tab, unsigned long long slots,
                                                       unsigned long long* __restrict__ full) {
    const AnCols sg = segs[blockIdx.y].c;
    unsigned long long lo, hi;
    an_range(sg, b0, b1, &lo, &hi);
    const unsigned long long stride = (unsigned long long)gridDim.x * kAnWG;
    const uint32_t lane = lane_id();
    for (unsigned long long base = lo + (unsigned long long)blockIdx.x * kAnWG + (threadIdx.x - lane); base < hi; base += stride) {
        const unsigned long long i = base + lane;
        const bool valid = i < hi;
        const unsigned long long id = valid ? sg.tid[i] : 0ull;
        unsigned long long val = valid ? (unsigned long long)sg.ts[i] ^ kAnSign : 0ull;
        // (an invalid lane has val 0, the floor: whichever run takes it in changes nothing)
        const unsigned long long prev = __shfl_up(id, 1);
        const bool head = valid && (lane == 0 || prev != id);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long oid = __shfl_down(id, off), oval = __shfl_down(val, off);
            if (lane + off < 64 && oid == id && oval > val) val = oval;
        }
        if (!head) continue;
        const unsigned long long want = id ? id : 1ull;
        unsigned long long s = id ? an_end_home(id, slots) : slots, tries = 0;
        for (; tries < slots; ++tries) {
            unsigned long long* p = tab + 2 * s;
            unsigned long long k = p[0];
            if (k == 0ull) {
                k = atomicCAS(p, 0ull, want);
                if (k == 0ull) k = want;
            }
            if (k == want) {
                if (p[1] < val) atomicMax(p + 1, val);
                break;
            }
            s = (s + 1ull) & (slots - 1ull);
        }
        if (tries == slots) atomicAdd(full, 1ull);
    }
}

// One thread per pin (ids ascending): a pinned id of this range that is in the table gets its verdict,
// 1 = goes, 2 = stays (0: never met), and its end becomes all ones, which sends the mark pass to the
// verdicts. A pin's id lies in one bucket, so in one range: a verdict is written once.
__global__ __launch_bounds__(kAnWG) void k_an_end_pins(const unsigned long long* __restrict__ ids,
                                                       const unsigned long long* __restrict__ cuts, uint32_t n, uint32_t b0,
                                                       uint32_t b1, unsigned long long* tab, unsigned long long slots,
                                                       uint32_t* __restrict__ verdict) {
    const uint32_t p = blockIdx.x * kAnWG + threadIdx.x;
    if (p >= n) return;
    const unsigned long long id = ids[p];
    const uint32_t b = an_bucket(id);
    if (b < b0 || b >= b1) return;
    const unsigned long long s = an_end_find(tab, slots, id);
    if (s == kAnNone) return;
    verdict[p] = tab[2 * s + 1] >= cuts[p] ? 2u : 1u;
    tab[2 * s + 1] = kAnNone;
}

// Entry i of the range's slice of segment blockIdx.y survives when its trace's end is >= cut, or by its
// pin's verdict. A wave owns the 64 entries of one mark word (the slice's edges inside a word are masked
// out, and words of different ranges are ORed: the ranges run one after another), writes its ballot with
// one atomic and adds its survivors to surv[segment][bucket], the lanes of one bucket at once. All bounds
// of the loop are wave-uniform, so every lane reaches the ballots.
__global__ __launch_bounds__(kAnWG) void k_an_end_mark(const AnXSeg* __restrict__ segs, uint32_t b0, uint32_t b1,
                                                       const unsigned long long* __restrict__ tab, unsigned long long slots,
                                                       unsigned long long cut, const unsigned long long* __restrict__ pin_ids,
                                                       const uint32_t* __restrict__ verdict, uint32_t n_pins,
                                                       unsigned long long* __restrict__ marks, uint32_t* __restrict__ surv) {
    const AnXSeg xs = segs[blockIdx.y];
    const AnCols sg = xs.c;
    unsigned long long lo, hi;
    an_range(sg, b0, b1, &lo, &hi);
    if (lo >= hi) return;
    const unsigned long long w_hi = (hi + 63ull) >> 6, wstride = (unsigned long long)gridDim.x * (kAnWG / 64);
    for (unsigned long long w = (lo >> 6) + (unsigned long long)blockIdx.x * (kAnWG / 64) + (threadIdx.x >> 6); w < w_hi; w += wstride) {
        const unsigned long long i = (w << 6) + lane_id();
        bool alive = false;
        uint32_t b = 0;
        if (i >= lo && i < hi) {
            const unsigned long long id = sg.tid[i];
            b = an_bucket(id);
            const unsigned long long s = b >= b0 && b < b1 ? an_end_find(tab, slots, id) : kAnNone;
            if (s != kAnNone) {
                const unsigned long long e = tab[2 * s + 1];
                alive = e >= cut;
                if (e == kAnNone && n_pins) {  // a pinned trace, or an end at INT64_MAX (which stays at any cut)
                    uint32_t a = 0, z = n_pins;
                    while (a < z) {
                        const uint32_t mid = (a + z) >> 1;
                        if (pin_ids[mid] < id) a = mid + 1; else z = mid;
                    }
                    if (a < n_pins && pin_ids[a] == id && verdict[a]) alive = verdict[a] == 2u;
                }
            }
        }
        const unsigned long long m = __ballot(alive);
        if (!m) continue;  // (wave-uniform)
        if ((int)lane_id() == __ffsll((long long)m) - 1) atomicOr(&marks[xs.mark_at + w], m);  // (i < hi <= n: a word of this segment)
        bool todo = alive;
        for (;;) {  // every turn settles at least one lane
            const unsigned long long mm = __ballot(todo);
            if (!mm) break;
            const int lead = __ffsll((long long)mm) - 1;
            const uint32_t lb = __shfl(b, lead);
            const unsigned long long same = __ballot(todo && b == lb);
            if ((int)lane_id() == lead) atomicAdd(&surv[(size_t)blockIdx.y * kAnBins + lb], (uint32_t)__popcll(same));  // (lb < kAnBins)
            if (b == lb) todo = false;
        }
    }
}

// k_an_scatter over a stretch of an old segment, for the marked entries only: the mark bits are read for
// every entry, trace_id (twice) and the other six columns for survivors. cursor[b] starts at the new
// segment's off[b]; a place at or past off[b + 1] is dropped.
__global__ __launch_bounds__(kAnWG) void k_an_expire_rewrite(const AnXSeg* __restrict__ segs, const AnItem* __restrict__ items,
                                                             unsigned long long chunk, const unsigned long long* __restrict__ marks,
                                                             uint32_t* __restrict__ cursor, AnCols out) {
    __shared__ uint32_t s_cnt[kAnBins];
    __shared__ uint32_t s_base[kAnBins];
    const AnItem it = items[blockIdx.x];
    const AnXSeg xs = segs[it.seg];
    const AnCols in = xs.c;
    const unsigned long long lo = (unsigned long long)it.chunk * chunk;  // (a multiple of the workgroup: a wave's 64 entries share a mark word)
    if (lo >= in.n) return;  // (the same for the whole workgroup)
    const unsigned long long hi = lo + chunk < in.n ? lo + chunk : in.n;
    for (uint32_t b = threadIdx.x; b < kAnBins; b += kAnWG) s_cnt[b] = 0u;
    __syncthreads();
    for (unsigned long long base = lo; base < hi; base += kAnWG) {
        const unsigned long long i = base + threadIdx.x;
        const bool keep = i < hi && ((marks[xs.mark_at + (i >> 6)] >> (i & 63ull)) & 1ull);
        const unsigned long long t = keep ? in.tid[i] : 0ull;
        hist_add(s_cnt, keep, an_bucket(t));
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kAnBins; b += kAnWG) {
        const uint32_t c = s_cnt[b];
        s_base[b] = c ? atomicAdd(&cursor[b], c) : 0u;
        s_cnt[b] = 0u;
    }
    __syncthreads();
    for (unsigned long long base = lo; base < hi; base += kAnWG) {
        const unsigned long long i = base + threadIdx.x;
        const bool keep = i < hi && ((marks[xs.mark_at + (i >> 6)] >> (i & 63ull)) & 1ull);
        const unsigned long long t = keep ? in.tid[i] : 0ull;
        const uint32_t b = an_bucket(t);
        const uint32_t rank = hist_rank(s_cnt, keep, b);
        if (keep) {
            const unsigned long long at = (unsigned long long)s_base[b] + rank;
            if (at < (unsigned long long)out.off[b + 1] && at < out.n) {
                out.tid[at] = t;
                out.span[at] = in.span[i];
                out.ts[at] = in.ts[i];
                out.val[at] = in.val[i];
                out.ip[at] = in.ip[i];
                out.svc[at] = in.svc[i];
                out.bits[at] = in.bits[i];
            }
        }
    }
}

size_t al256(size_t b) { return (b + 255) / 256 * 256; }

// seven columns of n entries in one block, each 256-B aligned; with_off: off[4097] behind them
struct Block {
    static size_t col8(uint64_t n) { return al256((size_t)n * 8); }
    static size_t col4(uint64_t n) { return al256((size_t)n * 4); }
    static size_t cols_bytes(uint64_t n) { return 4 * col8(n) + 3 * col4(n); }
    static AnCols view(void* block, uint64_t n, bool with_off) {
        uint8_t* p = (uint8_t*)block;
        const size_t a8 = col8(n), a4 = col4(n);
        return AnCols{(unsigned long long*)p, (unsigned long long*)(p + a8), (long long*)(p + 2 * a8),
                      (unsigned long long*)(p + 3 * a8), (uint32_t*)(p + 4 * a8), (uint32_t*)(p + 4 * a8 + a4),
                      (uint32_t*)(p + 4 * a8 + 2 * a4), with_off ? (uint32_t*)(p + 4 * a8 + 3 * a4) : nullptr,
                      (unsigned long long)n};
    }
};

struct Segment {
    void* block = nullptr;
    size_t bytes = 0;
    uint64_t n = 0;
    std::vector<uint32_t> off;  // kAnBins + 1

    static size_t bytes_for(uint64_t n) { return Block::cols_bytes(n) + al256((kAnBins + 1) * 4); }
    AnCols cols() const { return Block::view(block, n, true); }
};

}  // namespace
}  // namespace zk

using namespace zk;

struct zk_an {
    int device = 0;
    bool opened = false;     // the device is checked and the stream exists (the first observe with rows)
    hipStream_t stream = nullptr, own = nullptr;
    bool timing = false;
    std::vector<Segment> segs;
    uint64_t entries = 0;
    void* obs = nullptr;     // the observe's counts and cursors (kObsBytes)
    void* stage = nullptr;   // the seven columns of a host batch
    void* mplan = nullptr;   // a merge's bases, per old segment
    void* q = nullptr;       // the lookups' block (kQBytes)
    void* rows = nullptr;    // the write pass's rows, seven columns
    void* adj = nullptr;     // the adjusted summaries' block: the heads, then the work lists (kAdjBytes)
    void* adj_ents = nullptr;  // their entries at the span store's row bases: first, last [8 B], service [4 B]
    void* adjt = nullptr;      // the adjusted traces' block: the heads (56 B), then the work lists (kAdjtBytes)
    void* adjt_spans = nullptr;  // their spans (56 B) at the span store's row bases
    void* adjt_svc = nullptr;    // their (span, service) pairs at the same bases
    void* adjt_rows = nullptr;   // their rows, six columns (the trace id is the asked one): a trace at its row base + 2 x its span base
    size_t stage_bytes = 0, mplan_bytes = 0, rows_bytes = 0, adj_ents_bytes = 0;
    size_t adjt_spans_bytes = 0, adjt_svc_bytes = 0, adjt_rows_bytes = 0;
    std::vector<uint8_t> adj_traces_host, adj_heads_host, adj_ents_host;
    std::vector<uint8_t> adjt_heads_host, adjt_spans_host, adjt_svc_host, adjt_rows_host;
    std::vector<uint32_t> adj_counts_host, adj_list_host;
    std::vector<uint32_t> counts_host, cursor_host, off_host;  // (queued copies read the last two: they change only behind a synchronisation)
    std::vector<uint32_t> mplan_host, moff_host;
    std::vector<uint64_t> ids_host, base_host;
    std::vector<AnCols> segs_host;
    std::vector<uint8_t> rows_host;
    hipEvent_t oev[4] = {};  // around the passes of the last observe (zk_an_observe_ms)
    hipEvent_t qev[2] = {};  // around the last lookup (zk_an_query_ms)
    hipEvent_t xev[4] = {};  // around the passes of the last expiry (zk_an_expire_ms)
    bool otimed = false, qtimed = false, xtimed = false;
    uint64_t expire_chunk = 0;  // entries per range of buckets at most
    void* xplan = nullptr;      // the expiry's block (kXBytes)
    std::vector<AnXSeg> xsegs_host;
    std::vector<AnItem> xitems_host;
    std::vector<uint32_t> xsurv_host, xcursor_host, xoff_host;
    std::vector<unsigned long long> xpin_ids_host, xpin_cuts_host;
    std::string err;
};

namespace {

zk_status afail(zk_an* h, zk_status s, const std::string& m) {
    if (h) h->err = m;
    return s;
}

#define AN_HIP(h, call)                                                                            \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess) return afail(h, is_refusal(_e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP,       \
                                           std::string(#call) + ": " + launch_error_str(_e));      \
    } while (0)

// the first call that needs the device: it must be a gfx950; the private stream is made here
zk_status open_device(zk_an* h) {
    if (h->opened) return ZK_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || h->device >= ndev) {
        (void)hipGetLastError();
        return afail(h, ZK_ERR_NO_DEVICE, "no such HIP device");
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) return afail(h, ZK_ERR_NO_DEVICE, "no such HIP device");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return afail(h, ZK_ERR_NO_DEVICE, "the device is not a gfx950");
    AN_HIP(h, hipSetDevice(h->device));
    if (!h->stream) {
        AN_HIP(h, hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking));
        h->stream = h->own;
    }
    h->opened = true;
    return ZK_OK;
}

// a fresh block of `need` bytes; a refused allocation is ZK_ERR_CAPACITY
zk_status alloc(zk_an* h, void** p, size_t need, const char* what) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, need ? need : 8);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (e != hipErrorOutOfMemory) return afail(h, ZK_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        return afail(h, ZK_ERR_CAPACITY, std::string("no device memory for ") + what);
    }
    *p = q;
    return ZK_OK;
}

// at least `need` bytes behind *p: a larger block first, then the old one freed (its content is not kept);
// a refused allocation leaves *p as it was
zk_status grow(zk_an* h, void** p, size_t* have, size_t need, const char* what) {
    if (need <= *have && *p) return ZK_OK;
    void* q = nullptr;
    const zk_status st = alloc(h, &q, need, what);
    if (st != ZK_OK) return st;
    if (*p) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(*p);
    }
    *p = q;
    *have = need;
    return ZK_OK;
}

void free_segments(zk_an* h) {
    if (!h->segs.empty()) (void)hipStreamSynchronize(h->stream);
    for (Segment& g : h->segs)
        if (g.block) (void)hipFree(g.block);
    h->segs.clear();
}

// All segments into one: each bucket's slices concatenated in segment order. Anything refused leaves the
// store as it was. Synchronises.
zk_status merge_all(zk_an* h) {
    const uint32_t G = (uint32_t)h->segs.size();
    if (G < 2) return ZK_OK;
    Segment m;
    m.n = h->entries;
    m.off.assign(kAnBins + 1, 0);
    std::vector<uint64_t> wide(kAnBins + 1, 0);
    for (uint32_t b = 0; b < kAnBins; ++b) {
        uint64_t c = 0;
        for (const Segment& sg : h->segs) c += sg.off[b + 1] - sg.off[b];
        wide[b + 1] = wide[b] + c;
    }
    if (wide[kAnBins] != m.n || m.n > kAnMaxEntries) return afail(h, ZK_ERR_HIP, "the segments' offsets do not add up");
    for (uint32_t b = 0; b <= kAnBins; ++b) m.off[b] = (uint32_t)wide[b];
    // per old segment: the bases of its slices in the merged segment [kAnBins]
    h->mplan_host.assign((size_t)kAnBins * G, 0);
    std::vector<uint32_t> next(m.off.begin(), m.off.begin() + kAnBins);
    for (uint32_t g = 0; g < G; ++g) {
        const Segment& sg = h->segs[g];
        for (uint32_t b = 0; b < kAnBins; ++b) {
            h->mplan_host[(size_t)kAnBins * g + b] = next[b];
            next[b] += sg.off[b + 1] - sg.off[b];
        }
    }
    zk_status st = grow(h, &h->mplan, &h->mplan_bytes, (size_t)kAnBins * G * 4, "a merge's bases");
    if (st != ZK_OK) return st;
    m.bytes = Segment::bytes_for(m.n);
    if ((st = alloc(h, &m.block, m.bytes, "the merged segment (44 B per entry)")) != ZK_OK) return st;
    const AnCols dst = m.cols();
    h->moff_host = m.off;
    hipError_t e = hipMemcpyAsync(h->mplan, h->mplan_host.data(), (size_t)kAnBins * G * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dst.off, h->moff_host.data(), (kAnBins + 1) * 4, hipMemcpyHostToDevice, h->stream);
    for (uint32_t g = 0; g < G && e == hipSuccess; ++g) {
        const Segment& sg = h->segs[g];
        e = launch_checked("k_an_merge", k_an_merge, dim3(an_grid(sg.n)), dim3(kAnWG), 0, h->stream, sg.cols(),
                           (const uint32_t*)h->mplan + (size_t)kAnBins * g, dst);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(m.block);
        return afail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("merging the segments: ") + launch_error_str(e));
    }
    free_segments(h);
    h->segs.push_back(std::move(m));
    return ZK_OK;
}

// The lookups' count pass: the ids into the block (from the host or the device), counts[n] back. *parts =
// the grid's z of both passes. Synchronises; needs a store with segments.
zk_status find_count(zk_an* h, const uint64_t* ids, uint32_t n, uint32_t flags, uint32_t* counts, uint32_t* parts) {
    zk_status st;
    if (!h->q && (st = alloc(h, &h->q, kQBytes, "the lookups' block")) != ZK_OK) return st;
    uint8_t* qb = (uint8_t*)h->q;
    unsigned long long* d_ids = (unsigned long long*)(qb + kQIdsAt);
    uint32_t* d_counts = (uint32_t*)(qb + kQCountsAt);
    const uint32_t G = (uint32_t)h->segs.size();
    // the host needs the ids too: it sizes the grid by the longest asked slice
    h->ids_host.resize(n);
    if (flags & ZK_BATCH_DEVICE_PTRS) {
        AN_HIP(h, hipMemcpyAsync(d_ids, ids, (size_t)n * 8, hipMemcpyDeviceToDevice, h->stream));
        AN_HIP(h, hipMemcpyAsync(h->ids_host.data(), ids, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
        AN_HIP(h, hipStreamSynchronize(h->stream));
    } else {
        memcpy(h->ids_host.data(), ids, (size_t)n * 8);
        AN_HIP(h, hipMemcpyAsync(d_ids, h->ids_host.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    }
    uint64_t longest = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t b = an_bucket(h->ids_host[i]);
        for (const Segment& sg : h->segs) longest = std::max<uint64_t>(longest, sg.off[b + 1] - sg.off[b]);
    }
    uint64_t z = std::min<uint64_t>(kAnMaxParts, std::max<uint64_t>(1, (longest + kAnPart - 1) / kAnPart));
    z = std::max<uint64_t>(1, std::min<uint64_t>(z, kAnMaxFindGrid / ((uint64_t)n * G)));
    *parts = (uint32_t)z;
    h->segs_host.clear();
    for (const Segment& sg : h->segs) h->segs_host.push_back(sg.cols());
    AN_HIP(h, hipMemcpyAsync(qb + kQSegsAt, h->segs_host.data(), G * sizeof(AnCols), hipMemcpyHostToDevice, h->stream));
    AN_HIP(h, hipMemsetAsync(d_counts, 0, (size_t)n * 4, h->stream));
    for (hipEvent_t& e : h->qev)
        if (h->timing && !e) AN_HIP(h, hipEventCreate(&e));
    h->qtimed = false;
    if (h->timing) AN_HIP(h, hipEventRecord(h->qev[0], h->stream));
    AN_HIP(h, launch_checked("k_an_find_count", k_an_find_count, dim3(n, G, *parts), dim3(kAnWG), 0, h->stream,
                             (const AnCols*)(qb + kQSegsAt), (const unsigned long long*)d_ids, d_counts));
    AN_HIP(h, hipMemcpyAsync(counts, d_counts, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    AN_HIP(h, hipStreamSynchronize(h->stream));
    return ZK_OK;
}

// a range of buckets [b0, b1) and its entries over all segments
struct AnRange {
    uint32_t b0, b1;
    uint64_t entries;
};

// zk_an_expire behind its argument checks (a store with segments; the pins ascending by id, their cuts
// as keys, in the handle's vectors). Per range of buckets the end table's three passes, then the one
// synchronisation that sizes the rest, then the segments sorted into untouched (no entry goes: not read
// again), gone (every entry goes: freed) and mixed (their survivors rewritten into ONE new segment, which
// takes the place of the first of them). Nothing is freed and no bookkeeping changes before the new
// segment is complete; anything refused leaves the store as it was. The table and the marks are scratch
// of this call.
zk_status expire(zk_an* h, unsigned long long cut, uint64_t* removed_out, void** table, void** marks) {
    const uint32_t G = (uint32_t)h->segs.size(), P = (uint32_t)h->xpin_ids_host.size();
    // the ranges: consecutive buckets while their entries over all segments stay inside the chunk
    std::vector<AnRange> ranges;
    uint64_t most = 0;
    for (uint32_t b = 0; b < kAnBins; ++b) {
        uint64_t c = 0;
        for (const Segment& sg : h->segs) c += sg.off[b + 1] - sg.off[b];
        if (ranges.empty() || (ranges.back().entries && ranges.back().entries + c > h->expire_chunk))
            ranges.push_back(AnRange{b, b + 1, c});
        else {
            ranges.back().b1 = b + 1;
            ranges.back().entries += c;
        }
        most = std::max(most, ranges.back().entries);
    }
    const auto slots_for = [](uint64_t entries) {
        uint64_t s = kAnEndMinSlots;
        while (s < 2 * entries) s <<= 1;
        return s;
    };
    zk_status st;
    if (!h->xplan && (st = alloc(h, &h->xplan, kXBytes, "the expiry's block")) != ZK_OK) return st;
    if ((st = alloc(h, table, (size_t)(slots_for(most) + 1) * 16, "the expiry's end table (16 B per slot)")) != ZK_OK) return st;
    h->xsegs_host.clear();
    uint64_t words = 0;
    for (const Segment& sg : h->segs) {
        h->xsegs_host.push_back(AnXSeg{sg.cols(), (unsigned long long)words});
        words += (sg.n + 63) / 64;
    }
    if ((st = alloc(h, marks, (size_t)words * 8, "the expiry's marks (1 bit per entry)")) != ZK_OK) return st;
    uint8_t* xp = (uint8_t*)h->xplan;
    const AnXSeg* segs = (const AnXSeg*)(xp + kXSegsAt);
    uint32_t* surv = (uint32_t*)(xp + kXSurvAt);
    uint32_t* cursor = (uint32_t*)(xp + kXCursorAt);
    unsigned long long* full = (unsigned long long*)(xp + kXFullAt);
    const unsigned long long* pin_ids = (const unsigned long long*)(xp + kXPinIdsAt);
    const unsigned long long* pin_cuts = (const unsigned long long*)(xp + kXPinCutsAt);
    uint32_t* verdict = (uint32_t*)(xp + kXVerdictAt);
    const AnItem* items = (const AnItem*)(xp + kXItemsAt);
    unsigned long long* tab = (unsigned long long*)*table;
    unsigned long long* mk = (unsigned long long*)*marks;
    const bool timing = h->timing;
    for (hipEvent_t& e : h->xev)
        if (timing && !e) AN_HIP(h, hipEventCreate(&e));
    AN_HIP(h, hipMemcpyAsync(xp + kXSegsAt, h->xsegs_host.data(), G * sizeof(AnXSeg), hipMemcpyHostToDevice, h->stream));
    AN_HIP(h, hipMemsetAsync(surv, 0, (size_t)G * kAnBins * 4, h->stream));
    AN_HIP(h, hipMemsetAsync(full, 0, 8, h->stream));
    AN_HIP(h, hipMemsetAsync(mk, 0, (size_t)words * 8, h->stream));
    if (P) {
        AN_HIP(h, hipMemcpyAsync(xp + kXPinIdsAt, h->xpin_ids_host.data(), (size_t)P * 8, hipMemcpyHostToDevice, h->stream));
        AN_HIP(h, hipMemcpyAsync(xp + kXPinCutsAt, h->xpin_cuts_host.data(), (size_t)P * 8, hipMemcpyHostToDevice, h->stream));
        AN_HIP(h, hipMemsetAsync(verdict, 0, (size_t)P * 4, h->stream));
    }
    if (timing) AN_HIP(h, hipEventRecord(h->xev[0], h->stream));
    for (const AnRange& r : ranges) {
        if (!r.entries) continue;
        const uint64_t slots = slots_for(r.entries);
        uint64_t longest = 0;  // the range's longest slice in one segment sizes the grid's x
        for (const Segment& sg : h->segs) longest = std::max<uint64_t>(longest, sg.off[r.b1] - sg.off[r.b0]);
        const dim3 grid(an_grid(longest, kAnEndGrid), G);
        AN_HIP(h, hipMemsetAsync(tab, 0, (size_t)(slots + 1) * 16, h->stream));
        AN_HIP(h, launch_checked("k_an_end_fold", k_an_end_fold, grid, dim3(kAnWG), 0, h->stream, segs, r.b0, r.b1, tab,
                                 (unsigned long long)slots, full));
        if (P)
            AN_HIP(h, launch_checked("k_an_end_pins", k_an_end_pins, dim3(an_grid(P)), dim3(kAnWG), 0, h->stream, pin_ids, pin_cuts, P,
                                     r.b0, r.b1, tab, (unsigned long long)slots, verdict));
        AN_HIP(h, launch_checked("k_an_end_mark", k_an_end_mark, grid, dim3(kAnWG), 0, h->stream, segs, r.b0, r.b1,
                                 (const unsigned long long*)tab, (unsigned long long)slots, cut, pin_ids, (const uint32_t*)verdict, P, mk,
                                 surv));
    }
    if (timing) AN_HIP(h, hipEventRecord(h->xev[1], h->stream));
    h->xsurv_host.resize((size_t)G * kAnBins);
    unsigned long long ran_full = 0;
    AN_HIP(h, hipMemcpyAsync(h->xsurv_host.data(), surv, (size_t)G * kAnBins * 4, hipMemcpyDeviceToHost, h->stream));
    AN_HIP(h, hipMemcpyAsync(&ran_full, full, 8, hipMemcpyDeviceToHost, h->stream));
    AN_HIP(h, hipStreamSynchronize(h->stream));  // the sizing synchronisation
    if (ran_full) return afail(h, ZK_ERR_HIP, "the expiry's end table ran full (the sizing rule was broken)");
    std::vector<uint64_t> keep(G, 0);
    std::vector<uint32_t> mixed;
    uint64_t removed = 0;
    for (uint32_t g = 0; g < G; ++g) {
        const Segment& sg = h->segs[g];
        for (uint32_t b = 0; b < kAnBins; ++b) {
            const uint64_t c = h->xsurv_host[(size_t)g * kAnBins + b];
            if (c > (uint64_t)(sg.off[b + 1] - sg.off[b])) return afail(h, ZK_ERR_HIP, "the expiry counted more survivors than a slice holds");
            keep[g] += c;
        }
        removed += sg.n - keep[g];
        if (keep[g] != 0 && keep[g] != sg.n) mixed.push_back(g);
    }
    if (removed == 0) {  // nothing goes: nothing is rewritten, reallocated or freed
        if (timing) AN_HIP(h, hipEventRecord(h->xev[2], h->stream));
        if (timing) AN_HIP(h, hipEventRecord(h->xev[3], h->stream));
        h->xtimed = timing;
        return ZK_OK;
    }
    Segment m;
    uint64_t chunk = kAnScatterPerWG;
    if (!mixed.empty()) {
        m.off.assign(kAnBins + 1, 0);
        for (uint32_t b = 0; b < kAnBins; ++b) {
            uint64_t c = 0;
            for (uint32_t g : mixed) c += h->xsurv_host[(size_t)g * kAnBins + b];
            m.off[b + 1] = (uint32_t)(m.off[b] + c);  // (below the store's entries, which fit)
        }
        m.n = m.off[kAnBins];
        m.bytes = Segment::bytes_for(m.n);
        const auto items_at = [&](uint64_t c) {
            uint64_t w = 0;
            for (uint32_t g : mixed) w += (h->segs[g].n + c - 1) / c;
            return w;
        };
        while (items_at(chunk) > kAnMaxItems + mixed.size()) chunk *= 2;
        h->xitems_host.clear();
        for (uint32_t g : mixed)
            for (uint64_t c = 0; c * chunk < h->segs[g].n; ++c) h->xitems_host.push_back(AnItem{g, (uint32_t)c});
        if ((st = alloc(h, &m.block, m.bytes, "the survivors' segment (44 B per entry)")) != ZK_OK) return st;
        h->xcursor_host.assign(m.off.begin(), m.off.begin() + kAnBins);
        h->xoff_host = m.off;
    }
    hipError_t e = hipSuccess;
    if (!mixed.empty()) {
        const AnCols dst = m.cols();
        e = hipMemcpyAsync(xp + kXItemsAt, h->xitems_host.data(), h->xitems_host.size() * sizeof(AnItem), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cursor, h->xcursor_host.data(), kAnBins * 4, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dst.off, h->xoff_host.data(), (kAnBins + 1) * 4, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess && timing) e = hipEventRecord(h->xev[2], h->stream);
        if (e == hipSuccess)
            e = launch_checked("k_an_expire_rewrite", k_an_expire_rewrite, dim3((uint32_t)h->xitems_host.size()), dim3(kAnWG), 0,
                               h->stream, segs, items, (unsigned long long)chunk, (const unsigned long long*)mk, cursor, dst);
    } else if (timing) {
        e = hipEventRecord(h->xev[2], h->stream);
    }
    if (e == hipSuccess && timing) e = hipEventRecord(h->xev[3], h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        if (m.block) (void)hipFree(m.block);
        return afail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("rewriting the survivors: ") + launch_error_str(e));
    }
    // the new segment is complete: the gone and the mixed segments leave
    std::vector<Segment> left;
    for (uint32_t g = 0; g < G; ++g) {
        Segment& sg = h->segs[g];
        if (keep[g] == sg.n) {
            left.push_back(std::move(sg));
            continue;
        }
        (void)hipFree(sg.block);
        if (!mixed.empty() && g == mixed[0]) left.push_back(std::move(m));
    }
    h->segs = std::move(left);
    h->entries -= removed;
    h->xtimed = timing;
    *removed_out = removed;
    return ZK_OK;
}

}  // namespace

extern "C" {

zk_status zk_an_create(const zk_an_config* cfg, zk_an** out) {
    ZK_GUARD_BEGIN
    if (!cfg || !out) return ZK_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->device < 0) return ZK_ERR_INVALID_ARG;
    zk_an* h = new zk_an();
    h->device = cfg->device;
    h->timing = cfg->timing != 0;
    h->expire_chunk = cfg->expire_chunk ? cfg->expire_chunk : kAnExpireChunk;
    h->stream = (hipStream_t)cfg->stream;  // (NULL: a private stream, made with the device's first use)
    *out = h;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_an_destroy(zk_an* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (h->opened) {
        (void)hipSetDevice(h->device);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        free_segments(h);
        for (void* p : {h->obs, h->stage, h->mplan, h->q, h->rows, h->xplan, h->adj, h->adj_ents, h->adjt, h->adjt_spans,
                        h->adjt_svc, h->adjt_rows})
            if (p) (void)hipFree(p);
        for (hipEvent_t e : h->oev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : h->qev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : h->xev)
            if (e) (void)hipEventDestroy(e);
        if (h->own) (void)hipStreamDestroy(h->own);
    }
    delete h;
    return ZK_OK;
    ZK_GUARD_END
}

const char* zk_an_last_error(const zk_an* h) { return h ? h->err.c_str() : "null handle"; }

zk_status zk_an_observe(zk_an* h, const zk_an_cols* in, uint64_t n, uint32_t flags) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!in) return afail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (flags & ~ZK_BATCH_DEVICE_PTRS) return afail(h, ZK_ERR_INVALID_ARG, "unknown batch flag");
    if (n >= (1ull << 32)) return afail(h, ZK_ERR_UNSUPPORTED, "2^32 rows or more in one batch");
    if (n == 0) return ZK_OK;
    if (!in->trace_id || !in->span_id || !in->ts || !in->value || !in->ipv4 || !in->service_id || !in->bits)
        return afail(h, ZK_ERR_INVALID_ARG, "null column");
    if (h->entries + n > kAnMaxEntries) return afail(h, ZK_ERR_CAPACITY, "more than 2^32 - 1 entries in one store");
    zk_status st;
    if ((st = open_device(h)) != ZK_OK) return st;
    AN_HIP(h, hipSetDevice(h->device));
    if (!h->obs && (st = alloc(h, &h->obs, kObsBytes, "the observe's counters")) != ZK_OK) return st;
    AnCols src{(unsigned long long*)in->trace_id, (unsigned long long*)in->span_id, (long long*)in->ts,
               (unsigned long long*)in->value, (uint32_t*)in->ipv4, (uint32_t*)in->service_id, (uint32_t*)in->bits, nullptr,
               (unsigned long long)n};
    if (!(flags & ZK_BATCH_DEVICE_PTRS)) {
        // a host batch: the seven columns staged (each 256-B aligned)
        if ((st = grow(h, &h->stage, &h->stage_bytes, Block::cols_bytes(n), "staging a host batch (44 B per row)")) != ZK_OK)
            return st;
        const AnCols s = Block::view(h->stage, n, false);
        AN_HIP(h, hipMemcpyAsync(s.tid, in->trace_id, n * 8, hipMemcpyHostToDevice, h->stream));
        AN_HIP(h, hipMemcpyAsync(s.span, in->span_id, n * 8, hipMemcpyHostToDevice, h->stream));
        AN_HIP(h, hipMemcpyAsync(s.ts, in->ts, n * 8, hipMemcpyHostToDevice, h->stream));
        AN_HIP(h, hipMemcpyAsync(s.val, in->value, n * 8, hipMemcpyHostToDevice, h->stream));
        AN_HIP(h, hipMemcpyAsync(s.ip, in->ipv4, n * 4, hipMemcpyHostToDevice, h->stream));
        AN_HIP(h, hipMemcpyAsync(s.svc, in->service_id, n * 4, hipMemcpyHostToDevice, h->stream));
        AN_HIP(h, hipMemcpyAsync(s.bits, in->bits, n * 4, hipMemcpyHostToDevice, h->stream));
        src = s;
    }
    uint32_t* counts = (uint32_t*)h->obs;
    uint32_t* cursor = (uint32_t*)((uint8_t*)h->obs + kObsCursorAt);
    const bool timing = h->timing;
    for (hipEvent_t& e : h->oev)
        if (timing && !e) AN_HIP(h, hipEventCreate(&e));
    h->otimed = false;
    AN_HIP(h, hipMemsetAsync(counts, 0, kAnBins * 4, h->stream));
    if (timing) AN_HIP(h, hipEventRecord(h->oev[0], h->stream));
    AN_HIP(h, launch_checked("k_an_count", k_an_count, dim3(an_grid((n + kAnCntItems - 1) / kAnCntItems, kAnHistGrid)), dim3(kAnWG), 0,
                             h->stream, (const unsigned long long*)src.tid, (unsigned long long)n, counts));
    if (timing) AN_HIP(h, hipEventRecord(h->oev[1], h->stream));
    h->counts_host.resize(kAnBins);
    AN_HIP(h, hipMemcpyAsync(h->counts_host.data(), counts, kAnBins * 4, hipMemcpyDeviceToHost, h->stream));
    AN_HIP(h, hipStreamSynchronize(h->stream));  // the call's one synchronisation (also: the staging copies are done)
    Segment g;
    g.off.assign(kAnBins + 1, 0);
    uint64_t total = 0;
    for (uint32_t b = 0; b < kAnBins; ++b) {
        total += h->counts_host[b];
        if (total > n) return afail(h, ZK_ERR_HIP, "the bucket counts exceed the batch");
        g.off[b + 1] = (uint32_t)total;
    }
    if (total != n) return afail(h, ZK_ERR_HIP, "the bucket counts do not add up to the batch");
    g.n = n;
    if (h->segs.size() >= ZK_AN_MAX_SEGMENTS && (st = merge_all(h)) != ZK_OK) return st;
    g.bytes = Segment::bytes_for(g.n);
    if ((st = alloc(h, &g.block, g.bytes, "a segment (44 B per entry)")) != ZK_OK) return st;
    const AnCols dst = g.cols();
    h->cursor_host.assign(g.off.begin(), g.off.begin() + kAnBins);
    h->off_host = g.off;
    uint32_t grid = (uint32_t)((n + kAnScatterPerWG - 1) / kAnScatterPerWG);
    grid = grid < 1 ? 1 : grid > kAnMaxGrid ? kAnMaxGrid : grid;
    const uint64_t chunk = ((n + grid - 1) / grid + kAnWG - 1) / kAnWG * kAnWG;
    hipError_t e = hipMemcpyAsync(cursor, h->cursor_host.data(), kAnBins * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dst.off, h->off_host.data(), (kAnBins + 1) * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && timing) e = hipEventRecord(h->oev[2], h->stream);
    if (e == hipSuccess)
        e = launch_checked("k_an_scatter", k_an_scatter, dim3(grid), dim3(kAnWG), 0, h->stream, src, (unsigned long long)chunk, cursor, dst);
    if (e == hipSuccess && timing) e = hipEventRecord(h->oev[3], h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(g.block);
        return afail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("k_an_scatter: ") + launch_error_str(e));
    }
    h->entries += g.n;
    h->segs.push_back(std::move(g));
    h->otimed = timing;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_an_observe_ms(zk_an* h, double out[3]) {
    ZK_GUARD_BEGIN
    if (!h || !out) return ZK_ERR_INVALID_ARG;
    if (!h->otimed) return afail(h, ZK_ERR_INVALID_ARG, "no timed observe has added a segment (zk_an_config.timing)");
    AN_HIP(h, hipSetDevice(h->device));
    AN_HIP(h, hipEventSynchronize(h->oev[3]));
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        AN_HIP(h, hipEventElapsedTime(&ms, h->oev[k], h->oev[k + 1]));
        out[k] = ms;
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_an_reset(zk_an* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (h->segs.empty()) return ZK_OK;
    AN_HIP(h, hipSetDevice(h->device));
    free_segments(h);
    h->entries = 0;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_an_compact(zk_an* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (h->segs.size() < 2) return ZK_OK;
    AN_HIP(h, hipSetDevice(h->device));
    return merge_all(h);
    ZK_GUARD_END
}

zk_status zk_an_expire(zk_an* h, int64_t min_end, const uint64_t* pin_ids, const int64_t* pin_min_end, uint32_t n_pins,
                       uint64_t* removed) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!removed) return afail(h, ZK_ERR_INVALID_ARG, "null argument");
    *removed = 0;
    if (n_pins > ZK_AN_MAX_PINS) return afail(h, ZK_ERR_INVALID_ARG, "more than ZK_AN_MAX_PINS pins");
    if (n_pins && (!pin_ids || !pin_min_end)) return afail(h, ZK_ERR_INVALID_ARG, "null argument");
    // the pins ascending by id (the mark pass searches them), their cuts as keys
    static thread_local std::vector<uint32_t> order;
    order.resize(n_pins);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [pin_ids](uint32_t x, uint32_t y) { return pin_ids[x] < pin_ids[y]; });
    for (uint32_t i = 1; i < n_pins; ++i)
        if (pin_ids[order[i - 1]] == pin_ids[order[i]]) return afail(h, ZK_ERR_INVALID_ARG, "a trace id is pinned twice");
    h->xtimed = false;
    if (h->segs.empty()) return ZK_OK;  // (a handle that never opened a device answers here)
    if (min_end == INT64_MIN && n_pins == 0) return ZK_OK;  // every end is >= INT64_MIN
    h->xpin_ids_host.resize(n_pins);
    h->xpin_cuts_host.resize(n_pins);
    for (uint32_t i = 0; i < n_pins; ++i) {
        h->xpin_ids_host[i] = pin_ids[order[i]];
        h->xpin_cuts_host[i] = (unsigned long long)pin_min_end[order[i]] ^ kAnSign;
    }
    AN_HIP(h, hipSetDevice(h->device));
    void *table = nullptr, *marks = nullptr;
    const zk_status st = expire(h, (unsigned long long)min_end ^ kAnSign, removed, &table, &marks);
    if (table || marks) (void)hipStreamSynchronize(h->stream);
    if (table) (void)hipFree(table);
    if (marks) (void)hipFree(marks);
    return st;
    ZK_GUARD_END
}

zk_status zk_an_expire_ms(zk_an* h, double out[3]) {
    ZK_GUARD_BEGIN
    if (!h || !out) return ZK_ERR_INVALID_ARG;
    if (!h->xtimed) return afail(h, ZK_ERR_INVALID_ARG, "no timed expiry has run a pass (zk_an_config.timing)");
    AN_HIP(h, hipSetDevice(h->device));
    AN_HIP(h, hipEventSynchronize(h->xev[3]));
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        AN_HIP(h, hipEventElapsedTime(&ms, h->xev[k], h->xev[k + 1]));
        out[k] = ms;
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_an_info(zk_an* h, uint64_t* entries, uint64_t* segments, uint64_t* bytes) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!h->segs.empty()) {
        AN_HIP(h, hipSetDevice(h->device));
        AN_HIP(h, hipStreamSynchronize(h->stream));
    }
    uint64_t b = 0;
    for (const Segment& g : h->segs) b += g.bytes;
    if (entries) *entries = h->entries;
    if (segments) *segments = h->segs.size();
    if (bytes) *bytes = b;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_an_gather(zk_an* h, const uint64_t* ids, uint32_t n, uint32_t flags, uint32_t* counts, zk_an_cols* out, uint64_t cap,
                       uint64_t* n_out) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!n_out) return afail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (flags & ~ZK_BATCH_DEVICE_PTRS) return afail(h, ZK_ERR_INVALID_ARG, "unknown flag");
    if (n > ZK_AN_MAX_IDS) return afail(h, ZK_ERR_INVALID_ARG, "more than ZK_AN_MAX_IDS ids");
    if (n && !ids) return afail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (n && !counts) return afail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (cap && (!out || !out->trace_id || !out->span_id || !out->ts || !out->value || !out->ipv4 || !out->service_id || !out->bits))
        return afail(h, ZK_ERR_INVALID_ARG, "null output column");
    *n_out = 0;
    if (n == 0) return ZK_OK;
    memset(counts, 0, (size_t)n * 4);
    if (h->segs.empty()) return ZK_OK;
    AN_HIP(h, hipSetDevice(h->device));
    zk_status st;
    uint32_t parts = 1;
    if ((st = find_count(h, ids, n, flags, counts, &parts)) != ZK_OK) return st;
    h->base_host.resize(n);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        h->base_host[i] = total;
        total += counts[i];
    }
    *n_out = total;
    if (total > cap) return afail(h, ZK_ERR_CAPACITY, "the output columns hold fewer rows than the asked traces have");
    if (total == 0) return ZK_OK;
    if ((st = grow(h, &h->rows, &h->rows_bytes, Block::cols_bytes(total), "the gathered rows (44 B each)")) != ZK_OK) return st;
    h->rows_host.resize(Block::cols_bytes(total));
    uint8_t* qb = (uint8_t*)h->q;
    const AnCols dev = Block::view(h->rows, total, false);
    const uint32_t G = (uint32_t)h->segs.size();
    AN_HIP(h, hipMemcpyAsync(qb + kQBaseAt, h->base_host.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    AN_HIP(h, hipMemsetAsync(qb + kQCursorAt, 0, (size_t)n * 4, h->stream));
    AN_HIP(h, launch_checked("k_an_find_write", k_an_find_write, dim3(n, G, parts), dim3(kAnWG), 0, h->stream,
                             (const AnCols*)(qb + kQSegsAt), (const unsigned long long*)(qb + kQIdsAt),
                             (const uint32_t*)(qb + kQCountsAt), (uint32_t*)(qb + kQCursorAt),
                             (const unsigned long long*)(qb + kQBaseAt), dev));
    // the seven columns lie back to back, each 256-B aligned, in the device block and in the host's copy
    AN_HIP(h, hipMemcpyAsync(h->rows_host.data(), h->rows, Block::cols_bytes(total), hipMemcpyDeviceToHost, h->stream));
    if (h->timing) AN_HIP(h, hipEventRecord(h->qev[1], h->stream));
    AN_HIP(h, hipStreamSynchronize(h->stream));
    h->qtimed = h->timing;
    // every trace's rows into CANONICAL order (the trace id is the asked one)
    const AnCols r = Block::view(h->rows_host.data(), total, false);
    static thread_local std::vector<uint64_t> perm;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t at = h->base_host[i], c = counts[i];
        if (!c) continue;
        perm.resize(c);
        std::iota(perm.begin(), perm.end(), at);
        std::sort(perm.begin(), perm.end(), [&r](uint64_t x, uint64_t y) {
            if (r.span[x] != r.span[y]) return r.span[x] < r.span[y];
            if (r.ts[x] != r.ts[y]) return r.ts[x] < r.ts[y];
            const uint32_t bx = r.bits[x], by = r.bits[y];
            if ((bx & ZK_AN_KIND_MASK) != (by & ZK_AN_KIND_MASK)) return (bx & ZK_AN_KIND_MASK) < (by & ZK_AN_KIND_MASK);
            if (r.val[x] != r.val[y]) return r.val[x] < r.val[y];
            if (r.ip[x] != r.ip[y]) return r.ip[x] < r.ip[y];
            if ((bx >> ZK_AN_PORT_SHIFT) != (by >> ZK_AN_PORT_SHIFT)) return (bx >> ZK_AN_PORT_SHIFT) < (by >> ZK_AN_PORT_SHIFT);
            if (r.svc[x] != r.svc[y]) return r.svc[x] < r.svc[y];
            if ((bx & ZK_AN_HAS_HOST) != (by & ZK_AN_HAS_HOST)) return (bx & ZK_AN_HAS_HOST) < (by & ZK_AN_HAS_HOST);
            return bx < by;
        });
        for (uint64_t k = 0; k < c; ++k) {
            const uint64_t s = perm[k], d = at + k;
            out->trace_id[d] = r.tid[s];
            out->span_id[d] = r.span[s];
            out->ts[d] = r.ts[s];
            out->value[d] = r.val[s];
            out->ipv4[d] = r.ip[s];
            out->service_id[d] = r.svc[s];
            out->bits[d] = r.bits[s];
        }
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_an_query_ms(zk_an* h, double* ms) {
    ZK_GUARD_BEGIN
    if (!h || !ms) return ZK_ERR_INVALID_ARG;
    if (!h->qtimed) return afail(h, ZK_ERR_INVALID_ARG, "no timed lookup has run a pass (zk_an_config.timing)");
    AN_HIP(h, hipSetDevice(h->device));
    float f = 0.f;
    AN_HIP(h, hipEventElapsedTime(&f, h->qev[0], h->qev[1]));
    *ms = f;
    return ZK_OK;
    ZK_GUARD_END
}

// ---- the binary-annotation store (zkbinannots.h): a typed facade over the core above --------------------
// A zk_bn IS a zk_an behind another name: zk_bn_cols is zk_an_cols with `key` where `ts` is, the canonical
// order reads the key as the signed 64-bit value the core sorts ts by, and the TYPE lies where the KIND does.
// No kernel and no store code of its own; the types keep a zk_bn out of zk_an_expire / zk_an_adjusted_*.
static_assert(sizeof(zk_bn_cols) == sizeof(zk_an_cols), "zk_bn_cols is zk_an_cols");
static_assert(offsetof(zk_bn_cols, trace_id) == offsetof(zk_an_cols, trace_id) && offsetof(zk_bn_cols, span_id) == offsetof(zk_an_cols, span_id) &&
                  offsetof(zk_bn_cols, key) == offsetof(zk_an_cols, ts) && offsetof(zk_bn_cols, value) == offsetof(zk_an_cols, value) &&
                  offsetof(zk_bn_cols, ipv4) == offsetof(zk_an_cols, ipv4) && offsetof(zk_bn_cols, service_id) == offsetof(zk_an_cols, service_id) &&
                  offsetof(zk_bn_cols, bits) == offsetof(zk_an_cols, bits),
              "zk_bn_cols: key in the place of ts");
static_assert(sizeof(uint64_t*) == sizeof(int64_t*), "a key column is read as a ts column");
static_assert(ZK_BN_TYPE_MASK == ZK_AN_KIND_MASK && ZK_BN_HAS_HOST == ZK_AN_HAS_HOST && ZK_BN_PORT_SHIFT == ZK_AN_PORT_SHIFT,
              "the bits word of a binary row is laid out as the core sorts it");

static zk_an* bn_core(zk_bn* b) { return reinterpret_cast<zk_an*>(b); }

zk_status zk_bn_create(const zk_an_config* cfg, zk_bn** out) {
    if (!cfg || !out) return ZK_ERR_INVALID_ARG;
    zk_an_config c = *cfg;
    c.expire_chunk = 0;  // (ignored: no expiry)
    zk_an* h = nullptr;
    const zk_status st = zk_an_create(&c, &h);
    *out = reinterpret_cast<zk_bn*>(h);
    return st;
}
zk_status zk_bn_destroy(zk_bn* b) { return zk_an_destroy(bn_core(b)); }
const char* zk_bn_last_error(const zk_bn* b) { return zk_an_last_error(reinterpret_cast<const zk_an*>(b)); }
zk_status zk_bn_observe(zk_bn* b, const zk_bn_cols* in, uint64_t n, uint32_t flags) {
    return zk_an_observe(bn_core(b), reinterpret_cast<const zk_an_cols*>(in), n, flags);
}
zk_status zk_bn_reset(zk_bn* b) { return zk_an_reset(bn_core(b)); }
zk_status zk_bn_compact(zk_bn* b) { return zk_an_compact(bn_core(b)); }
zk_status zk_bn_info(zk_bn* b, uint64_t* entries, uint64_t* segments, uint64_t* bytes) {
    return zk_an_info(bn_core(b), entries, segments, bytes);
}
zk_status zk_bn_gather(zk_bn* b, const uint64_t* ids, uint32_t n, uint32_t flags, uint32_t* counts, zk_bn_cols* out, uint64_t cap,
                       uint64_t* n_out) {
    return zk_an_gather(bn_core(b), ids, n, flags, counts, reinterpret_cast<zk_an_cols*>(out), cap, n_out);
}
zk_status zk_bn_observe_ms(zk_bn* b, double out[3]) { return zk_an_observe_ms(bn_core(b), out); }
zk_status zk_bn_query_ms(zk_bn* b, double* ms) { return zk_an_query_ms(bn_core(b), ms); }

}  // extern "C"

// ---- time-skew-adjusted summaries (zk_an_adjusted_summaries) ----------------------------------------------
//   k_an_adjust   one asked trace per wave (up to 64 rows and 64 spans) or per workgroup of 256, over BOTH
//                 stagings: the merged spans and services zk_sp_traces left in the span store's, and the rows
//                 this handle's write pass staged. 52 B of LDS per span and 26 B per row. The span ids are
//                 sorted once (in the rows' area, before the rows come in) for every span's parent and for the
//                 rank that breaks the ties of the span order; the rows are sorted by the full canonical key
//                 (value and service_id, read only on a tie of span, ts and kind, stay in HBM); every span
//                 finds its run of rows by binary search and takes its times from it; the spans are sorted
//                 into span order; the root is the first without a parent; the walk goes level by level, a
//                 thread per span of the level, and finds a span's level as it arrives (a span whose parent
//                 was visited in the round before is visited in this one), so no depths are computed ahead;
//                 then the times again, the span order again over the survivors, a prefix sum that places the
//                 entries. Every store is bounded: a trace that does not fit the launch's caps or whose
//                 stagings end before it is left alone (its head stays zero), and an entry at or past the
//                 trace's (span, service) pairs or the staging's end is dropped.
//                 The EMITTING instantiation (In = AdjEmitIn, zk_an_adjusted_traces) shares steps 1 to 7 and then
//                 writes the adjusted trace itself: for a trace without a parentless span the root-most span (one
//                 lane up the parents) and the depths (the walk's rounds without a shift); prefix sums over the
//                 sorted positions of every survivor's rows (its own and the two injected ones of a client-only
//                 span) and services; the spans and pairs a thread per position; the rows with all threads
//                 striding over the OUTPUT rows, each finding its span by binary search over the row offsets,
//                 which lie in LDS fields the walk has left dead. The summaries instantiation compiles to what
//                 it was before the template parameter.
namespace zk {
namespace {

constexpr int kAdjWave = ZK_AN_ADJ_WAVE_ROWS;
constexpr uint32_t kAdjMaxRows = ZK_AN_ADJ_MAX_ROWS;
constexpr uint32_t kAdjMaxSpans = ZK_SP_TRACE_MAX_ROWS;
constexpr uint32_t kAdjNone16 = 0xFFFFu, kAdjNone = 0xFFFFFFFFu;
constexpr uint32_t kAdjLoopback = 0x7F000001u;
constexpr uint32_t kAdjHasParent = 1u, kAdjTimed = 2u, kAdjGiveOwn = 4u, kAdjGiveClient = 8u, kAdjGiveEp = 16u;  // a span's bits in LDS
constexpr size_t kAdjLdsHead = 64;      // the counters [8 x 4 B], start, end [8 B], 16 B unused
constexpr size_t kAdjLdsPerSpan = 52;   // first, last, give [8 B], gip, bits, fc [4 B], par, run, len, ord, rank, pos, depth, svo [2 B]
constexpr size_t kAdjLdsPerRow = 26;    // span, ts [8 B], ip, bits [4 B], ord [2 B]
// the block: the heads, then the work list
constexpr size_t kAdjListAt = (size_t)ZK_AN_MAX_IDS * sizeof(zk_sp_summary);
constexpr size_t kAdjBytes = kAdjListAt + (size_t)ZK_AN_MAX_IDS * 4;

static_assert(kAdjWave == 64, "a wave holds one row or span per lane");
static_assert(kAdjMaxRows >= 1024 && (kAdjMaxRows & (kAdjMaxRows - 1)) == 0 && kAdjMaxRows < kAdjNone16, "16-bit row numbers over a power of two");
static_assert(kAdjMaxSpans < kAdjNone16 && (kAdjMaxSpans & (kAdjMaxSpans - 1)) == 0, "16-bit span numbers and levels");
static_assert(ZK_AN_MAX_IDS == ZK_SP_MAX_IDS, "one ask goes to both stores");
static_assert((ZK_AN_ADJ_ANNOTATED & (ZK_SP_SUM_FOUND | ZK_SP_SUM_TIMED | ZK_SP_SUM_OVERFLOW)) == 0 &&
                  (ZK_AN_ADJ_OVERFLOW & (ZK_SP_SUM_FOUND | ZK_SP_SUM_TIMED | ZK_SP_SUM_OVERFLOW | ZK_AN_ADJ_ANNOTATED)) == 0,
              "the new state bits lie beside the ZK_SP_SUM_* ones");

// LDS of one k_an_adjust workgroup whose launch admits `spans` spans and `rows` rows (powers of two >= 64):
// the rows' area first holds the span ids of the id sort
constexpr size_t adj_lds(uint32_t spans, uint32_t rows) {
    return kAdjLdsHead + kAdjLdsPerSpan * spans + (kAdjLdsPerRow * rows > 8 * (size_t)spans ? kAdjLdsPerRow * rows : 8 * (size_t)spans);
}
static_assert(adj_lds(kAdjMaxSpans, kAdjMaxRows) <= kLdsPerCU, "a trace at both bounds fits the 160 KiB of a CU");

struct AdjIn {
    AnCols rows;                            // this handle's staged rows
    const uint32_t* list;                   // the work list: asked indices
    const unsigned long long* ids;
    const uint32_t* counts;                 // the rows per asked id
    const unsigned long long* base;         // their bases in `rows`
    const zk_sp_trace* t_heads;             // the span store's staging (zk_sp_staged.h)
    const zk_sp_span* t_spans;
    const uint32_t* t_svc;
    const unsigned long long* t_base;
    unsigned long long t_total;             // its rows: the bound of t_spans, t_svc and of the entries written
    uint32_t cap_spans, cap_rows;           // what the launch's LDS admits
    zk_sp_summary* heads;
    uint32_t* o_svc;
    long long* o_first;
    long long* o_last;
    static constexpr bool kEmit = false;
};

// k_an_adjust's emitting instantiation (zk_an_adjusted_traces): the same inputs, and the adjusted trace's spans,
// pairs and rows. heads, o_svc, o_first and o_last of the base are not used.
struct AdjEmitIn : AdjIn {
    zk_an_trace* e_heads;
    zk_an_span* e_spans;                    // [t_total]: a trace's spans at its base in the span store's numbering
    uint32_t* e_svc;                        // [t_total]: its pairs at the same base
    unsigned long long* e_span;             // the rows, six columns of e_n entries: a trace's at base[q] + 2 * t_base[q]
    long long* e_ts;
    unsigned long long* e_val;
    uint32_t* e_ip;
    uint32_t* e_rsvc;
    uint32_t* e_bits;
    unsigned long long e_n;
    unsigned long long h_sr, h_ss;          // zk_hash_string("sr"), ("ss"): the injected rows' values
    static constexpr bool kEmit = true;
};

// a bitonic sort of ord[0, P) (P a power of two >= 2, the same for the whole workgroup). Ends behind a barrier.
template <int T, class Less>
__device__ inline void adj_sort(uint16_t* ord, uint32_t P, const Less& less) {
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t w = threadIdx.x; w < P / 2; w += T) {
                const uint32_t i = ((w & ~(j - 1u)) << 1) | (w & (j - 1u)), x = i | j;
                const uint16_t a = ord[i], b = ord[x];
                if ((i & k) == 0 ? less(b, a) : less(a, b)) {
                    ord[i] = b;
                    ord[x] = a;
                }
            }
            __syncthreads();
        }
}

// the exclusive prefix of `sum` over the workgroup's threads and the total; s_wave: T / 64 words. Every thread calls.
template <int T>
__device__ inline uint32_t adj_scan(uint32_t sum, uint32_t* s_wave, uint32_t* total) {
    uint32_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if ((int)lane_id() >= d) inc += o;
    }
    __syncthreads();
    if (lane_id() == 63) s_wave[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t before = inc - sum, all = 0u;
    for (uint32_t w = 0; w < (uint32_t)(T / 64); ++w) {
        if (w < (threadIdx.x >> 6)) before += s_wave[w];
        all += s_wave[w];
    }
    *total = all;
    return before;
}

// TimeSkewAdjuster's skew, the JVM's arithmetic (64-bit wrap, / 2 toward zero); false: none
__device__ inline bool adj_skew(long long cs, long long cr, long long sr, long long ss, unsigned long long* out) {
    const long long cd = (long long)((unsigned long long)cr - (unsigned long long)cs);
    const long long sd = (long long)((unsigned long long)ss - (unsigned long long)sr);
    if (sd > cd || (cs < sr && cr > ss)) return false;
    const long long lat = (long long)((unsigned long long)cd - (unsigned long long)sd) / 2;
    const unsigned long long sk = (unsigned long long)sr - (unsigned long long)lat - (unsigned long long)cs;
    if (sk == 0ull) return false;
    *out = sk;
    return true;
}

template <int T, class In>
__global__ __launch_bounds__(T) void k_an_adjust(In in) {
    constexpr bool EMIT = In::kEmit;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_adj[];
    uint32_t* s_cnt = (uint32_t*)s_adj;  // [0] the root's position, [1] a level's visits, [2] timed, [3] the survivors, [4..7] the scan's waves
    unsigned long long* s_lo = (unsigned long long*)(s_adj + 32);
    unsigned long long* s_hi = s_lo + 1;
    const uint32_t q = in.list[blockIdx.x];
    const zk_sp_trace th = in.t_heads[q];
    const uint32_t S = th.spans, A = in.counts[q];
    const uint32_t cs = in.cap_spans, cr = in.cap_rows;
    const unsigned long long sb0 = in.t_base[q], ab0 = in.base[q];
    // (the host lists only traces that fit; anything else is left alone, before any barrier)
    if (S == 0 || S > cs || S > kAdjMaxSpans || A > cr || A > kAdjMaxRows || sb0 + S > in.t_total ||
        sb0 + th.services > in.t_total || ab0 + A > in.rows.n)
        return;
    unsigned long long* f_first = (unsigned long long*)(s_adj + kAdjLdsHead);
    unsigned long long* f_last = f_first + cs;
    unsigned long long* f_give = f_last + cs;   // OWN: the skew; CLIENT: the sorted positions of its cs and cr
    uint32_t* f_gip = (uint32_t*)(f_give + cs);  // the ipv4 of what it hands down
    uint32_t* f_bits = f_gip + cs;
    uint32_t* f_fc = f_bits + cs;                // the first child's position in span order (kAdjNone: no child)
    uint16_t* f_par = (uint16_t*)(f_fc + cs);
    uint16_t* f_run = f_par + cs;
    uint16_t* f_len = f_run + cs;
    uint16_t* f_ord = f_len + cs;
    uint16_t* f_rank = f_ord + cs;
    uint16_t* f_pos = f_rank + cs;
    uint16_t* f_depth = f_pos + cs;
    uint16_t* f_svo = f_depth + cs;
    unsigned char* area = (unsigned char*)(f_svo + cs);
    unsigned long long* tmp_id = (unsigned long long*)area;
    unsigned long long* r_span = (unsigned long long*)area;
    unsigned long long* r_ts = r_span + cr;
    uint32_t* r_ip = (uint32_t*)(r_ts + cr);
    uint32_t* r_bits = r_ip + cr;
    uint16_t* r_ord = (uint16_t*)(r_bits + cr);
    const zk_sp_span* spans = in.t_spans + sb0;
    const bool annotated = A > 0u;
    uint32_t PS = 2, PA = 2;
    while (PS < S) PS <<= 1;
    while (PA < A) PA <<= 1;
    if (threadIdx.x == 0) {
        s_cnt[0] = kAdjNone;
        s_cnt[1] = s_cnt[2] = s_cnt[3] = 0u;
        *s_lo = kAnNone;
        *s_hi = 0ull;
    }
    // 1. the spans: record times, bits; the ids sorted for the parents and the ranks
    for (uint32_t i = threadIdx.x; i < PS; i += T) f_ord[i] = (uint16_t)i;
    for (uint32_t i = threadIdx.x; i < S; i += T) {
        const zk_sp_span sp = spans[i];
        const bool timed = sp.bits & ZK_SP_SPAN_TIMED;
        tmp_id[i] = sp.span_id;
        f_first[i] = timed ? (unsigned long long)sp.first ^ kAnSign : kAnNone;
        f_last[i] = timed ? (unsigned long long)sp.last ^ kAnSign : 0ull;
        f_bits[i] = ((sp.bits & ZK_SP_SPAN_HAS_PARENT) ? kAdjHasParent : 0u) | (timed ? kAdjTimed : 0u);
        f_fc[i] = kAdjNone;
        f_par[i] = (uint16_t)kAdjNone16;
        f_run[i] = f_len[i] = f_depth[i] = 0;
    }
    __syncthreads();
    if (annotated) {
        adj_sort<T>(f_ord, PS, [&](uint32_t a, uint32_t b) {
            if (b >= S) return a < S;
            if (a >= S) return false;
            return tmp_id[a] < tmp_id[b];
        });
        for (uint32_t p = threadIdx.x; p < S; p += T) f_rank[f_ord[p]] = (uint16_t)p;
        for (uint32_t i = threadIdx.x; i < S; i += T) {
            const zk_sp_span sp = spans[i];
            if ((sp.bits & ZK_SP_SPAN_HAS_PARENT) && (sp.bits & ZK_SP_SPAN_PARENT_FOUND)) {
                uint32_t a = 0, z = S;
                while (a < z) {
                    const uint32_t mid = (a + z) >> 1;
                    if (tmp_id[f_ord[mid]] < sp.parent_id) a = mid + 1; else z = mid;
                }
                if (a < S && tmp_id[f_ord[a]] == sp.parent_id) f_par[i] = f_ord[a];
            }
        }
    }
    // every span's place in the services column: the prefix sum of the spans' service counts
    {
        const uint32_t C = (S + T - 1) / T, p0 = threadIdx.x * C;
        uint32_t sum = 0u, all;
        for (uint32_t p = p0; p < p0 + C && p < S; ++p) sum += spans[p].services;
        uint32_t before = adj_scan<T>(sum, s_cnt + 4, &all);
        for (uint32_t p = p0; p < p0 + C && p < S; ++p) {
            f_svo[p] = (uint16_t)(before < kAdjNone16 ? before : kAdjNone16);
            before += spans[p].services;
        }
    }
    __syncthreads();  // (tmp_id is read no more: the rows take its place)
    bool has_root = false;
    if (annotated) {
        // 2. the rows, in canonical order
        for (uint32_t i = threadIdx.x; i < PA; i += T) r_ord[i] = (uint16_t)i;
        for (uint32_t i = threadIdx.x; i < A; i += T) {
            r_span[i] = in.rows.span[ab0 + i];
            r_ts[i] = (unsigned long long)in.rows.ts[ab0 + i] ^ kAnSign;
            r_ip[i] = in.rows.ip[ab0 + i];
            r_bits[i] = in.rows.bits[ab0 + i];
        }
        __syncthreads();
        adj_sort<T>(r_ord, PA, [&](uint32_t a, uint32_t b) {
            if (b >= A) return a < A;
            if (a >= A) return false;
            if (r_span[a] != r_span[b]) return r_span[a] < r_span[b];
            if (r_ts[a] != r_ts[b]) return r_ts[a] < r_ts[b];
            const uint32_t ba = r_bits[a], bb = r_bits[b];
            if ((ba & ZK_AN_KIND_MASK) != (bb & ZK_AN_KIND_MASK)) return (ba & ZK_AN_KIND_MASK) < (bb & ZK_AN_KIND_MASK);
            const unsigned long long va = in.rows.val[ab0 + a], vb = in.rows.val[ab0 + b];
            if (va != vb) return va < vb;
            if (r_ip[a] != r_ip[b]) return r_ip[a] < r_ip[b];
            if ((ba >> ZK_AN_PORT_SHIFT) != (bb >> ZK_AN_PORT_SHIFT)) return (ba >> ZK_AN_PORT_SHIFT) < (bb >> ZK_AN_PORT_SHIFT);
            const uint32_t sa = in.rows.svc[ab0 + a], sb = in.rows.svc[ab0 + b];
            if (sa != sb) return sa < sb;
            if ((ba & ZK_AN_HAS_HOST) != (bb & ZK_AN_HAS_HOST)) return (ba & ZK_AN_HAS_HOST) < (bb & ZK_AN_HAS_HOST);
            return ba < bb;
        });
        // 3. every span's run of rows, and its times from it
        for (uint32_t i = threadIdx.x; i < S; i += T) {
            const unsigned long long id = spans[i].span_id;
            uint32_t a = 0, z = A;
            while (a < z) {
                const uint32_t mid = (a + z) >> 1;
                if (r_span[r_ord[mid]] < id) a = mid + 1; else z = mid;
            }
            uint32_t e = a;
            z = A;
            while (e < z) {
                const uint32_t mid = (e + z) >> 1;
                if (r_span[r_ord[mid]] <= id) e = mid + 1; else z = mid;
            }
            f_run[i] = (uint16_t)a;
            f_len[i] = (uint16_t)(e - a);
            if (e > a) {
                f_first[i] = r_ts[r_ord[a]];
                f_last[i] = r_ts[r_ord[e - 1]];
                f_bits[i] |= kAdjTimed;
            }
        }
        __syncthreads();
        // 4. span order from these times; the root; every span's first child
        adj_sort<T>(f_ord, PS, [&](uint32_t a, uint32_t b) {
            if (b >= S) return a < S;
            if (a >= S) return false;
            if (f_first[a] != f_first[b]) return f_first[a] < f_first[b];
            return f_rank[a] < f_rank[b];
        });
        for (uint32_t p = threadIdx.x; p < S; p += T) {
            const uint32_t i = f_ord[p];
            f_pos[i] = (uint16_t)p;
            if (!(f_bits[i] & kAdjHasParent)) atomicMin(&s_cnt[0], p);
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < S; i += T)
            if (f_par[i] != kAdjNone16) atomicMin(&f_fc[f_par[i]], (uint32_t)f_pos[i]);
        __syncthreads();
        has_root = s_cnt[0] < S;
    }
    if (has_root) {
        // 5. the walk, a level per round: the root, then every span whose parent was visited the round before
        const uint32_t root = f_ord[s_cnt[0]];
        for (uint32_t level = 1; level <= S; ++level) {
            bool did = false;
            for (uint32_t i = threadIdx.x; i < S; i += T) {
                const uint32_t par = f_par[i];
                if (level == 1 ? i != root : (f_depth[i] != 0 || par == kAdjNone16 || par == i || f_depth[par] != level - 1)) continue;
                f_depth[i] = (uint16_t)level;
                did = true;
                const uint32_t r0 = f_run[i], len = f_len[i];
                // what the parent hands down: its own skew, or (a client-only parent) this child's own
                bool shift = false;
                uint32_t ip = 0u;
                unsigned long long sk = 0ull;
                uint32_t n1 = 0, n2 = 0, n3 = 0, n4 = 0, f1 = 0, f2 = 0, l1 = 0, l2 = 0, l3 = 0, l4 = 0;
                for (uint32_t k = 0; k < len; ++k) {
                    const uint32_t p = r0 + k, kind = r_bits[r_ord[p]] & ZK_AN_KIND_MASK;
                    if (kind == ZK_AN_KIND_CS) { if (!n1++) f1 = p; l1 = p; }
                    else if (kind == ZK_AN_KIND_CR) { if (!n2++) f2 = p; l2 = p; }
                    else if (kind == ZK_AN_KIND_SR) { ++n3; l3 = p; }
                    else if (kind == ZK_AN_KIND_SS) { ++n4; l4 = p; }
                }
                if (level > 1) {
                    const uint32_t pb = f_bits[par];
                    if (pb & kAdjGiveOwn) {
                        shift = true;
                        ip = f_gip[par];
                        sk = f_give[par];
                    } else if ((pb & kAdjGiveClient) && (pb & kAdjGiveEp) && n1 && n2) {
                        const uint32_t pcs = (uint32_t)(f_give[par] & 0xFFFFu), pcr = (uint32_t)(f_give[par] >> 16) & 0xFFFFu;
                        shift = adj_skew((long long)(r_ts[r_ord[pcs]] ^ kAnSign), (long long)(r_ts[r_ord[pcr]] ^ kAnSign),
                                         (long long)(r_ts[r_ord[f1]] ^ kAnSign), (long long)(r_ts[r_ord[f2]] ^ kAnSign), &sk);
                        ip = f_gip[par];
                    }
                }
                for (int pass = 0; pass < 2; ++pass) {
                    if (shift)
                        for (uint32_t k = 0; k < len; ++k) {
                            const uint32_t r = r_ord[r0 + k], b = r_bits[r], kind = b & ZK_AN_KIND_MASK;
                            if ((b & ZK_AN_HAS_HOST) && (r_ip[r] == ip || ((kind == ZK_AN_KIND_CS || kind == ZK_AN_KIND_CR) && r_ip[r] == kAdjLoopback)))
                                r_ts[r] -= sk;  // (held ^ sign: the difference is the same)
                        }
                    if (pass == 1) break;
                    shift = false;
                    if (n1 == 1 && n2 == 1 && n3 <= 1 && n4 <= 1 && !(n3 && n4) && f_fc[i] != kAdjNone) {
                        // client-only: the endpoint is the host of the first cs or cr of the first child's list
                        const uint32_t kid = f_ord[f_fc[i]];
                        uint32_t bits = kAdjGiveClient;
                        if constexpr (EMIT) f_pos[i] = (uint16_t)kAdjNone16;  // (dead behind step 4: the row that gives the injected rows' host)
                        for (uint32_t k = 0; k < f_len[kid]; ++k) {
                            const uint32_t r = r_ord[(uint32_t)f_run[kid] + k], b = r_bits[r], kind = b & ZK_AN_KIND_MASK;
                            if (kind == ZK_AN_KIND_CS || kind == ZK_AN_KIND_CR) {
                                if (b & ZK_AN_HAS_HOST) {
                                    bits |= kAdjGiveEp;
                                    f_gip[i] = r_ip[r];
                                    if constexpr (EMIT) f_pos[i] = (uint16_t)r;
                                }
                                break;
                            }
                        }
                        f_give[i] = (unsigned long long)f1 | ((unsigned long long)f2 << 16);
                        f_bits[i] |= bits;
                    } else if (n1 && n2 && n3 && n4) {
                        // its own skew, from the last of each kind; the endpoint is the sr's host
                        const uint32_t rs = r_ord[l3];
                        if ((r_bits[rs] & ZK_AN_HAS_HOST) &&
                            adj_skew((long long)(r_ts[r_ord[l1]] ^ kAnSign), (long long)(r_ts[r_ord[l2]] ^ kAnSign),
                                     (long long)(r_ts[rs] ^ kAnSign), (long long)(r_ts[r_ord[l4]] ^ kAnSign), &sk)) {
                            shift = true;
                            ip = r_ip[rs];
                            f_gip[i] = ip;
                            f_give[i] = sk;
                            f_bits[i] |= kAdjGiveOwn;
                        }
                    }
                }
            }
            if (did) s_cnt[1] = 1u;
            __syncthreads();
            const bool any = s_cnt[1] != 0u;
            __syncthreads();
            if (!any) break;  // (the same for the whole workgroup)
            if (threadIdx.x == 0) s_cnt[1] = 0u;
            __syncthreads();
        }
        // 6. the survivors' times from their lists again
        for (uint32_t i = threadIdx.x; i < S; i += T) {
            if (f_depth[i] == 0 || f_len[i] == 0) continue;
            unsigned long long lo = kAnNone, hi = 0ull;
            for (uint32_t k = 0; k < f_len[i]; ++k) {
                const unsigned long long t = r_ts[r_ord[(uint32_t)f_run[i] + k]];
                lo = t < lo ? t : lo;
                hi = t > hi ? t : hi;
            }
            f_first[i] = lo;
            f_last[i] = hi;
        }
        __syncthreads();
        // 7. span order again: the survivors, then the pruned spans, then the padding (the first S positions
        // stay the trace's spans)
        adj_sort<T>(f_ord, PS, [&](uint32_t a, uint32_t b) {
            const uint32_t ca = a >= S ? 2u : f_depth[a] == 0 ? 1u : 0u, cb = b >= S ? 2u : f_depth[b] == 0 ? 1u : 0u;
            if (ca != cb) return ca < cb;
            if (ca != 0u) return false;
            if (f_first[a] != f_first[b]) return f_first[a] < f_first[b];
            return f_rank[a] < f_rank[b];
        });
    }
    if constexpr (EMIT) {
        // 8e. the emitting instantiation: the adjusted trace itself instead of its summary
        uint32_t rm = kAdjNone;  // the root-most span of an annotated trace
        if (has_root) {
            // the root: the one span the walk visited at level 1 (behind step 7 it need not be the first)
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < S; i += T)
                if (f_depth[i] == 1) s_cnt[0] = i;
            __syncthreads();
            rm = s_cnt[0];
        } else if (annotated) {
            // every span has a parent: getRootMostSpan and toSpanDepths over the annotation-derived span order.
            // One lane walks up from the first span through the parents the trace holds, to where the chain
            // would repeat (f_depth marks the spans met); then the levels go down as in step 5, with no shift.
            __syncthreads();  // (every thread has read s_cnt[0] for has_root)
            if (threadIdx.x == 0) {
                uint32_t s = f_ord[0];
                for (uint32_t step = 0; step < S; ++step) {
                    const uint32_t par = f_par[s];
                    if (par == kAdjNone16 || f_depth[s] != 0) break;
                    f_depth[s] = 1;
                    s = par;
                }
                s_cnt[0] = s;
            }
            __syncthreads();
            rm = s_cnt[0];
            for (uint32_t i = threadIdx.x; i < S; i += T) f_depth[i] = 0;
            __syncthreads();
            for (uint32_t level = 1; level <= S; ++level) {
                bool did = false;
                for (uint32_t i = threadIdx.x; i < S; i += T) {
                    const uint32_t par = f_par[i];
                    if (level == 1 ? i != rm : (f_depth[i] != 0 || par == kAdjNone16 || par == i || f_depth[par] != level - 1)) continue;
                    f_depth[i] = (uint16_t)level;
                    did = true;
                }
                if (did) s_cnt[1] = 1u;
                __syncthreads();
                const bool any = s_cnt[1] != 0u;
                __syncthreads();
                if (!any) break;  // (the same for the whole workgroup)
                if (threadIdx.x == 0) s_cnt[1] = 0u;
                __syncthreads();
            }
        }
        // the head's reductions, and every survivor's place in the rows and in the pairs: prefix sums over the
        // sorted positions, consecutive ones per thread (the survivors are the first positions)
        const uint32_t C = (S + T - 1) / T, p0 = threadIdx.x * C;
        uint32_t n_rows = 0u, n_svc = 0u, kept = 0u, rows_all = 0u, svc_all = 0u;
        unsigned long long lo = kAnNone, hi = 0ull;
        bool timed_any = false;
        for (uint32_t p = p0; p < p0 + C && p < S; ++p) {
            const uint32_t i = f_ord[p];
            if (has_root && f_depth[i] == 0) continue;
            ++kept;
            n_rows += (uint32_t)f_len[i] + ((f_bits[i] & kAdjGiveClient) ? 2u : 0u);
            n_svc += spans[i].services;
            if (f_bits[i] & kAdjTimed) {
                lo = f_first[i] < lo ? f_first[i] : lo;
                hi = f_last[i] > hi ? f_last[i] : hi;
                timed_any = true;
            }
        }
        if (kept) atomicAdd(&s_cnt[3], kept);
        if (timed_any) {
            atomicMin(s_lo, lo);
            atomicMax(s_hi, hi);
            atomicOr(&s_cnt[2], 1u);
        }
        uint32_t r_at = adj_scan<T>(n_rows, s_cnt + 4, &rows_all);
        uint32_t v_at = adj_scan<T>(n_svc, s_cnt + 4, &svc_all);
        // (f_fc and f_gip are dead behind the walk: by POSITION now, the span's first output row and first pair)
        for (uint32_t p = p0; p < p0 + C && p < S; ++p) {
            const uint32_t i = f_ord[p];
            if (has_root && f_depth[i] == 0) continue;
            f_fc[p] = r_at;
            f_gip[p] = v_at;
            r_at += (uint32_t)f_len[i] + ((f_bits[i] & kAdjGiveClient) ? 2u : 0u);
            v_at += spans[i].services;
        }
        __syncthreads();
        const uint32_t K = s_cnt[3] <= S ? s_cnt[3] : S;
        const uint32_t R = rows_all <= A + 2u * S ? rows_all : A + 2u * S;  // (a trace's share of the row staging)
        const uint32_t V = svc_all <= th.services ? svc_all : th.services;
        // the spans and their pairs, a thread per position
        for (uint32_t p = threadIdx.x; p < K; p += T) {
            const uint32_t i = f_ord[p];
            const zk_sp_span sp = spans[i];
            const bool timed = f_bits[i] & kAdjTimed;
            const uint32_t inj = (f_bits[i] & kAdjGiveClient) ? 2u : 0u;
            zk_an_span o;
            o.span_id = sp.span_id;
            o.parent_id = sp.parent_id;
            o.first = timed ? (long long)(f_first[i] ^ kAnSign) : 0;
            o.last = timed ? (long long)(f_last[i] ^ kAnSign) : 0;
            o.name = sp.name;
            o.services = sp.services;
            if (annotated) {
                o.depth = f_depth[i];
                o.bits = (sp.bits & ZK_SP_SPAN_HAS_PARENT) | (timed ? ZK_SP_SPAN_TIMED : 0u) |
                         (f_par[i] != kAdjNone16 ? ZK_SP_SPAN_PARENT_FOUND : 0u) | (i == rm ? ZK_SP_SPAN_ROOT_MOST : 0u);
            } else {  // zk_sp_traces' span as it is
                o.depth = sp.depth;
                o.bits = sp.bits;
            }
            o.rows = (uint32_t)f_len[i] + inj;
            o.injected = inj;
            if (sb0 + p < in.t_total) in.e_spans[sb0 + p] = o;
            const uint32_t to = f_gip[p], from = f_svo[i];
            for (uint32_t k = 0; k < sp.services; ++k)
                if (to + k < V && from + k < th.services && sb0 + to + k < in.t_total) in.e_svc[sb0 + to + k] = in.t_svc[sb0 + from + k];
        }
        // the rows: all threads stride over the OUTPUT rows; a row finds its span by binary search over the offsets
        const unsigned long long rb0 = ab0 + 2ull * sb0;
        for (uint32_t o = threadIdx.x; o < R; o += T) {
            uint32_t a = 0, z = K;
            while (a < z) {
                const uint32_t mid = (a + z) >> 1;
                if (f_fc[mid] <= o) a = mid + 1; else z = mid;
            }
            const unsigned long long e = rb0 + o;
            if (a == 0 || e >= in.e_n) continue;
            const uint32_t p = a - 1, i = f_ord[p], k = o - f_fc[p], len = f_len[i];
            if (k < len) {
                const uint32_t r = r_ord[(uint32_t)f_run[i] + k];
                in.e_span[e] = r_span[r];
                in.e_ts[e] = (long long)(r_ts[r] ^ kAnSign);
                in.e_val[e] = in.rows.val[ab0 + r];
                in.e_ip[e] = r_ip[r];
                in.e_rsvc[e] = in.rows.svc[ab0 + r];
                in.e_bits[e] = r_bits[r];
            } else if (k < len + 2u && (f_bits[i] & kAdjGiveClient)) {
                // an injected row: sr at the span's first cs, ss at its first cr, on the lead's endpoint
                const unsigned long long g = f_give[i];
                const bool sr = k == len;
                const uint32_t at = sr ? (uint32_t)(g & 0xFFFFu) : (uint32_t)(g >> 16) & 0xFFFFu, lead = f_pos[i];
                const uint32_t kind = sr ? ZK_AN_KIND_SR : ZK_AN_KIND_SS;
                const bool hosted = lead < A;
                in.e_span[e] = spans[i].span_id;
                in.e_ts[e] = (long long)(r_ts[r_ord[at < A ? at : 0u]] ^ kAnSign);
                in.e_val[e] = sr ? in.h_sr : in.h_ss;
                in.e_ip[e] = hosted ? r_ip[lead] : 0u;
                in.e_rsvc[e] = hosted ? in.rows.svc[ab0 + lead] : 0u;
                in.e_bits[e] = hosted ? (kind | ZK_AN_HAS_HOST | (r_bits[lead] & (0xFFFFu << ZK_AN_PORT_SHIFT))) : kind;
            }
        }
        if (threadIdx.x == 0) {
            zk_an_trace hd;
            const bool timed = s_cnt[2] != 0u;
            hd.trace_id = in.ids[q];
            hd.start = timed ? (long long)(*s_lo ^ kAnSign) : 0;
            hd.end = timed ? (long long)(*s_hi ^ kAnSign) : 0;
            hd.root_most = !annotated ? th.root_most : rm < S ? spans[rm].span_id : 0ull;
            hd.fragments = th.fragments;
            hd.spans = K;
            hd.services = V;
            hd.state = ZK_SP_TR_FOUND | (timed ? ZK_SP_TR_TIMED : 0u) | (annotated ? ZK_AN_ADJ_ANNOTATED : 0u);
            hd.rows = R;
            hd.reserved = 0u;
            in.e_heads[q] = hd;
        }
        return;
    }
    // (not annotated: f_ord is still the spans' own order, which zk_sp_traces made)
    // 8. the head's reductions and the entries' places over the sorted positions, consecutive ones per thread
    const uint32_t C = (S + T - 1) / T, p0 = threadIdx.x * C;
    uint32_t sum = 0u, kept = 0u, total = 0u;
    unsigned long long lo = kAnNone, hi = 0ull;
    bool timed_any = false;
    for (uint32_t p = p0; p < p0 + C && p < S; ++p) {
        const uint32_t i = f_ord[p];
        if (has_root && f_depth[i] == 0) continue;
        ++kept;
        if (f_bits[i] & kAdjTimed) {
            sum += spans[i].services;
            lo = f_first[i] < lo ? f_first[i] : lo;
            hi = f_last[i] > hi ? f_last[i] : hi;
            timed_any = true;
        }
    }
    if (kept) atomicAdd(&s_cnt[3], kept);
    if (timed_any) {
        atomicMin(s_lo, lo);
        atomicMax(s_hi, hi);
        atomicOr(&s_cnt[2], 1u);
    }
    uint32_t before = adj_scan<T>(sum, s_cnt + 4, &total);
    for (uint32_t p = p0; p < p0 + C && p < S; ++p) {
        const uint32_t i = f_ord[p];
        if ((has_root && f_depth[i] == 0) || !(f_bits[i] & kAdjTimed)) continue;
        const uint32_t k_n = spans[i].services, at = f_svo[i];
        for (uint32_t k = 0; k < k_n; ++k) {
            const unsigned long long e = sb0 + before + k;
            if (before + k < th.services && at + k < th.services && e < in.t_total) {
                in.o_svc[e] = in.t_svc[sb0 + at + k];
                in.o_first[e] = (long long)(f_first[i] ^ kAnSign);
                in.o_last[e] = (long long)(f_last[i] ^ kAnSign);
            }
        }
        before += k_n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        zk_sp_summary hd;
        const bool timed = s_cnt[2] != 0u;
        hd.trace_id = in.ids[q];
        hd.start = timed ? (long long)(*s_lo ^ kAnSign) : 0;
        hd.end = timed ? (long long)(*s_hi ^ kAnSign) : 0;
        hd.fragments = th.fragments;
        hd.spans = s_cnt[3];
        hd.span_ts = total <= th.services ? total : th.services;
        hd.state = ZK_SP_SUM_FOUND | (timed ? ZK_SP_SUM_TIMED : 0u) | (annotated ? ZK_AN_ADJ_ANNOTATED : 0u);
        in.heads[q] = hd;
    }
}

}  // namespace
}  // namespace zk

extern "C" zk_status zk_an_adjusted_summaries(zk_an* h, zk_sp* sp, const uint64_t* ids, uint32_t n, uint32_t flags,
                                              zk_sp_summary* heads, zk_sp_span_ts* out, uint64_t cap, uint64_t* n_out) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!sp || !n_out) return afail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (flags & ~ZK_BATCH_DEVICE_PTRS) return afail(h, ZK_ERR_INVALID_ARG, "unknown flag");
    if (n > ZK_AN_MAX_IDS) return afail(h, ZK_ERR_INVALID_ARG, "more than ZK_AN_MAX_IDS ids");
    if (n && (!ids || !heads)) return afail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (cap && (!out || !out->service_id || !out->first || !out->last)) return afail(h, ZK_ERR_INVALID_ARG, "null output column");
    if (sp_device(sp) != h->device) return afail(h, ZK_ERR_INVALID_ARG, "the two handles are on different devices");
    *n_out = 0;
    if (n == 0) return ZK_OK;
    memset(heads, 0, (size_t)n * sizeof(zk_sp_summary));
    h->qtimed = false;  // (zk_an_query_ms answers for this call only once k_an_adjust has run)
    zk_status st;
    if (h->segs.empty()) {
        // no trace is annotated: every answer is zk_sp_summaries' own
        st = zk_sp_summaries(sp, ids, n, flags, heads, out, cap, n_out);
        if (st != ZK_OK) afail(h, st, zk_sp_last_error(sp));
        if (st == ZK_OK || st == ZK_ERR_CAPACITY)
            for (uint32_t i = 0; i < n; ++i)
                if (heads[i].state & ZK_SP_SUM_OVERFLOW) heads[i].state |= ZK_AN_ADJ_OVERFLOW;
        return st;
    }
    // the span store's part: zk_sp_traces' passes, its sizing call; the merged spans stay in its staging
    h->adj_traces_host.resize((size_t)n * sizeof(zk_sp_trace));
    zk_sp_trace* th = (zk_sp_trace*)h->adj_traces_host.data();
    uint64_t t_out[2] = {0, 0};
    st = zk_sp_traces(sp, ids, n, flags, th, nullptr, 0, nullptr, 0, t_out);
    if (st != ZK_OK && st != ZK_ERR_CAPACITY) return afail(h, st, zk_sp_last_error(sp));
    bool any = false;
    for (uint32_t i = 0; i < n; ++i) any = any || (th[i].state & ZK_SP_TR_FOUND);
    if (!any) return ZK_OK;
    SpStagedTraces sv;
    sp_staged_traces(sp, &sv);
    if (!sv.heads || sv.total == 0) return afail(h, ZK_ERR_HIP, "the span store's staging is not there");
    AN_HIP(h, hipSetDevice(h->device));
    // this handle's part: the rows of the asked traces into its staging
    uint32_t parts = 1;
    h->adj_counts_host.resize(n);
    uint32_t* counts = h->adj_counts_host.data();
    if ((st = find_count(h, ids, n, flags, counts, &parts)) != ZK_OK) return st;
    h->base_host.resize(n);
    uint64_t rows_total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        h->base_host[i] = rows_total;
        rows_total += counts[i];
    }
    // the overflowed traces are answered here; the others go on the two work lists
    h->adj_list_host.clear();
    uint32_t big_spans = kAdjWave, big_rows = kAdjWave;
    for (int pass = 0; pass < 2; ++pass) {
        for (uint32_t i = 0; i < n; ++i) {
            if (!(th[i].state & ZK_SP_TR_FOUND)) continue;
            const bool over = (th[i].state & ZK_SP_TR_OVERFLOW) || th[i].spans > kAdjMaxSpans || counts[i] > kAdjMaxRows;
            if (over) {
                if (pass) continue;
                zk_sp_summary& hd = heads[i];
                hd.trace_id = th[i].trace_id;
                hd.fragments = th[i].fragments;
                hd.state = ZK_SP_SUM_FOUND | ZK_AN_ADJ_OVERFLOW;
                if (counts[i]) {
                    hd.state |= ZK_AN_ADJ_ANNOTATED;
                } else {  // not annotated: zk_sp_summaries' head of a trace above its bound
                    hd.start = th[i].start;
                    hd.end = th[i].end;
                    hd.state |= ZK_SP_SUM_OVERFLOW | (th[i].state & ZK_SP_TR_TIMED ? ZK_SP_SUM_TIMED : 0u);
                }
                continue;
            }
            const bool small = counts[i] <= (uint32_t)kAdjWave && th[i].spans <= (uint32_t)kAdjWave;
            if (small != (pass == 0)) continue;
            h->adj_list_host.push_back(i);
            if (!small) {
                while (big_spans < th[i].spans) big_spans <<= 1;
                while (big_rows < counts[i]) big_rows <<= 1;
            }
        }
    }
    uint32_t n_wave = 0;
    for (uint32_t i : h->adj_list_host)
        if (counts[i] <= (uint32_t)kAdjWave && th[i].spans <= (uint32_t)kAdjWave) ++n_wave;
    const uint32_t n_group = (uint32_t)h->adj_list_host.size() - n_wave;
    if (h->adj_list_host.empty()) return ZK_OK;
    if (!h->adj && (st = alloc(h, &h->adj, kAdjBytes, "the adjusted summaries' heads and work lists")) != ZK_OK) return st;
    if ((st = grow(h, &h->rows, &h->rows_bytes, Block::cols_bytes(rows_total), "the gathered rows (44 B each)")) != ZK_OK) return st;
    const size_t e8 = Block::col8(sv.total);
    if ((st = grow(h, &h->adj_ents, &h->adj_ents_bytes, 2 * e8 + Block::col4(sv.total), "the adjusted summaries' entries (20 B per fragment)")) != ZK_OK)
        return st;
    uint8_t* qb = (uint8_t*)h->q;
    uint8_t* ab = (uint8_t*)h->adj;
    const AnCols dev = Block::view(h->rows, rows_total, false);
    if (rows_total) {
        AN_HIP(h, hipMemcpyAsync(qb + kQBaseAt, h->base_host.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
        AN_HIP(h, hipMemsetAsync(qb + kQCursorAt, 0, (size_t)n * 4, h->stream));
        AN_HIP(h, launch_checked("k_an_find_write", k_an_find_write, dim3(n, (uint32_t)h->segs.size(), parts), dim3(kAnWG), 0, h->stream,
                                 (const AnCols*)(qb + kQSegsAt), (const unsigned long long*)(qb + kQIdsAt),
                                 (const uint32_t*)(qb + kQCountsAt), (uint32_t*)(qb + kQCursorAt),
                                 (const unsigned long long*)(qb + kQBaseAt), dev));
    } else {
        AN_HIP(h, hipMemcpyAsync(qb + kQBaseAt, h->base_host.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    }
    AN_HIP(h, hipMemcpyAsync(ab + kAdjListAt, h->adj_list_host.data(), h->adj_list_host.size() * 4, hipMemcpyHostToDevice, h->stream));
    AN_HIP(h, hipMemsetAsync(ab, 0, (size_t)n * sizeof(zk_sp_summary), h->stream));
    AdjIn in;
    in.rows = dev;
    in.list = (const uint32_t*)(ab + kAdjListAt);
    in.ids = (const unsigned long long*)(qb + kQIdsAt);
    in.counts = (const uint32_t*)(qb + kQCountsAt);
    in.base = (const unsigned long long*)(qb + kQBaseAt);
    in.t_heads = sv.heads;
    in.t_spans = sv.spans;
    in.t_svc = sv.services;
    in.t_base = sv.base;
    in.t_total = sv.total;
    in.cap_spans = in.cap_rows = (uint32_t)kAdjWave;
    in.heads = (zk_sp_summary*)ab;
    in.o_first = (long long*)h->adj_ents;
    in.o_last = (long long*)((uint8_t*)h->adj_ents + e8);
    in.o_svc = (uint32_t*)((uint8_t*)h->adj_ents + 2 * e8);
    AN_HIP(h, launch_checked("k_an_adjust (a wave per trace)", k_an_adjust<kAdjWave, AdjIn>, dim3(n_wave), dim3(kAdjWave),
                             adj_lds(kAdjWave, kAdjWave), h->stream, in));
    in.list += n_wave;
    in.cap_spans = big_spans;
    in.cap_rows = big_rows;
    AN_HIP(h, launch_checked("k_an_adjust (a workgroup per trace)", k_an_adjust<kAnWG, AdjIn>, dim3(n_group), dim3(kAnWG),
                             adj_lds(big_spans, big_rows), h->stream, in));
    // only the heads cross before the entries' total is known
    h->adj_heads_host.resize((size_t)n * sizeof(zk_sp_summary));
    const zk_sp_summary* got = (const zk_sp_summary*)h->adj_heads_host.data();
    AN_HIP(h, hipMemcpyAsync(h->adj_heads_host.data(), ab, (size_t)n * sizeof(zk_sp_summary), hipMemcpyDeviceToHost, h->stream));
    if (h->timing) AN_HIP(h, hipEventRecord(h->qev[1], h->stream));
    AN_HIP(h, hipStreamSynchronize(h->stream));
    h->qtimed = h->timing;
    uint64_t need = 0;
    for (uint32_t i : h->adj_list_host) {
        if (!(got[i].state & ZK_SP_SUM_FOUND)) return afail(h, ZK_ERR_HIP, "a listed trace was not adjusted");
        if (got[i].span_ts > th[i].fragments) return afail(h, ZK_ERR_HIP, "an adjusted summary has more entries than its trace has fragments");
        heads[i] = got[i];
        need += got[i].span_ts;
    }
    *n_out = need;
    if (need > cap) return afail(h, ZK_ERR_CAPACITY, "the output columns hold fewer entries than the asked traces have");
    if (need == 0) return ZK_OK;
    // the staged entry columns in one copy, then each trace's entries packed behind the ones before it
    const size_t bytes = 2 * e8 + (size_t)sv.total * 4;
    h->adj_ents_host.resize(bytes);
    AN_HIP(h, hipMemcpyAsync(h->adj_ents_host.data(), h->adj_ents, bytes, hipMemcpyDeviceToHost, h->stream));
    if (h->timing) AN_HIP(h, hipEventRecord(h->qev[1], h->stream));
    AN_HIP(h, hipStreamSynchronize(h->stream));
    const int64_t* s_first = (const int64_t*)h->adj_ents_host.data();
    const int64_t* s_last = (const int64_t*)(h->adj_ents_host.data() + e8);
    const uint32_t* s_svc = (const uint32_t*)(h->adj_ents_host.data() + 2 * e8);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t c = heads[i].span_ts, from = sv.base_host[i];
        if (!c) continue;
        memcpy(out->service_id + at, s_svc + from, c * 4);
        memcpy(out->first + at, s_first + from, c * 8);
        memcpy(out->last + at, s_last + from, c * 8);
        at += c;
    }
    return ZK_OK;
    ZK_GUARD_END
}

// ---- time-skew-adjusted traces (zk_an_adjusted_traces) ------------------------------------------------------
namespace zk {
namespace {

// the block: the heads (56 B), then the work list
constexpr size_t kAdjtListAt = (size_t)ZK_AN_MAX_IDS * sizeof(zk_an_trace);
constexpr size_t kAdjtBytes = kAdjtListAt + (size_t)ZK_AN_MAX_IDS * 4;

static_assert(sizeof(zk_an_trace) == 56 && sizeof(zk_an_span) == 56, "the ABI's layouts");
static_assert(offsetof(zk_an_trace, rows) == sizeof(zk_sp_trace) && offsetof(zk_an_span, rows) == sizeof(zk_sp_span),
              "zk_sp_trace and zk_sp_span are the first 48 bytes");
static_assert(ZK_SP_TR_FOUND == ZK_SP_SUM_FOUND && ZK_SP_TR_TIMED == ZK_SP_SUM_TIMED && ZK_SP_TR_OVERFLOW == ZK_SP_SUM_OVERFLOW &&
                  (ZK_AN_ADJ_ANNOTATED & (ZK_SP_TR_FOUND | ZK_SP_TR_TIMED | ZK_SP_TR_OVERFLOW)) == 0 &&
                  (ZK_AN_ADJ_OVERFLOW & (ZK_SP_TR_FOUND | ZK_SP_TR_TIMED | ZK_SP_TR_OVERFLOW | ZK_AN_ADJ_ANNOTATED)) == 0,
              "the ZK_AN_ADJ_* bits lie beside the ZK_SP_TR_* ones");

// the head of a trace that zk_sp_traces answered alone: its 48 bytes, no rows
zk_an_trace adjt_head_of(const zk_sp_trace& t) {
    zk_an_trace hd;
    memset(&hd, 0, sizeof hd);
    memcpy(&hd, &t, sizeof t);
    if (hd.state & ZK_SP_TR_OVERFLOW) hd.state |= ZK_AN_ADJ_OVERFLOW;
    return hd;
}

// An empty annotation store: every answer is zk_sp_traces' own, span for span.
zk_status adjt_plain(zk_an* h, zk_sp* sp, const uint64_t* ids, uint32_t n, uint32_t flags, zk_an_trace* heads, zk_an_span* spans,
                     uint64_t cap_spans, uint32_t* services, uint64_t cap_services, uint64_t totals[3]) {
    h->adj_traces_host.resize((size_t)n * sizeof(zk_sp_trace));
    zk_sp_trace* th = (zk_sp_trace*)h->adj_traces_host.data();
    uint64_t t_out[2] = {0, 0};
    zk_status st = zk_sp_traces(sp, ids, n, flags, th, nullptr, 0, nullptr, 0, t_out);
    if (st != ZK_OK && st != ZK_ERR_CAPACITY) return afail(h, st, zk_sp_last_error(sp));
    for (uint32_t i = 0; i < n; ++i) heads[i] = adjt_head_of(th[i]);
    totals[0] = t_out[0];
    totals[1] = t_out[1];
    if (t_out[0] > cap_spans || t_out[1] > cap_services)
        return afail(h, ZK_ERR_CAPACITY, "an output holds fewer entries than the asked traces have");
    if (st == ZK_OK) return ZK_OK;  // (nothing to emit)
    h->adjt_spans_host.resize((size_t)t_out[0] * sizeof(zk_sp_span));
    h->adjt_svc_host.resize((size_t)t_out[1] * 4 + 4);
    zk_sp_span* ts = (zk_sp_span*)h->adjt_spans_host.data();
    st = zk_sp_traces(sp, ids, n, flags, th, ts, t_out[0], (uint32_t*)h->adjt_svc_host.data(), t_out[1], t_out);
    if (st != ZK_OK) return afail(h, st, zk_sp_last_error(sp));
    for (uint64_t k = 0; k < t_out[0]; ++k) {
        zk_an_span o;
        memset(&o, 0, sizeof o);
        memcpy(&o, &ts[k], sizeof ts[k]);
        spans[k] = o;
    }
    if (t_out[1]) memcpy(services, h->adjt_svc_host.data(), (size_t)t_out[1] * 4);
    return ZK_OK;
}

}  // namespace
}  // namespace zk

extern "C" zk_status zk_an_adjusted_traces(zk_an* h, zk_sp* sp, const uint64_t* ids, uint32_t n, uint32_t flags, zk_an_trace* heads,
                                           zk_an_span* spans, uint64_t cap_spans, uint32_t* services, uint64_t cap_services,
                                           zk_an_cols* rows, uint64_t cap_rows, uint64_t totals[3]) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!sp || !totals) return afail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (flags & ~ZK_BATCH_DEVICE_PTRS) return afail(h, ZK_ERR_INVALID_ARG, "unknown flag");
    if (n > ZK_AN_MAX_IDS) return afail(h, ZK_ERR_INVALID_ARG, "more than ZK_AN_MAX_IDS ids");
    if (n && (!ids || !heads)) return afail(h, ZK_ERR_INVALID_ARG, "null argument");
    if ((cap_spans && !spans) || (cap_services && !services)) return afail(h, ZK_ERR_INVALID_ARG, "null output");
    if (cap_rows && (!rows || !rows->trace_id || !rows->span_id || !rows->ts || !rows->value || !rows->ipv4 || !rows->service_id || !rows->bits))
        return afail(h, ZK_ERR_INVALID_ARG, "null output column");
    if (sp_device(sp) != h->device) return afail(h, ZK_ERR_INVALID_ARG, "the two handles are on different devices");
    totals[0] = totals[1] = totals[2] = 0;
    if (n == 0) return ZK_OK;
    memset(heads, 0, (size_t)n * sizeof(zk_an_trace));
    h->qtimed = false;  // (zk_an_query_ms answers for this call only once k_an_adjust has run)
    if (h->segs.empty()) return adjt_plain(h, sp, ids, n, flags, heads, spans, cap_spans, services, cap_services, totals);
    zk_status st;
    // the span store's part: zk_sp_traces' passes, its sizing call; the merged spans stay in its staging
    h->adj_traces_host.resize((size_t)n * sizeof(zk_sp_trace));
    zk_sp_trace* th = (zk_sp_trace*)h->adj_traces_host.data();
    uint64_t t_out[2] = {0, 0};
    st = zk_sp_traces(sp, ids, n, flags, th, nullptr, 0, nullptr, 0, t_out);
    if (st != ZK_OK && st != ZK_ERR_CAPACITY) return afail(h, st, zk_sp_last_error(sp));
    bool any = false;
    for (uint32_t i = 0; i < n; ++i) any = any || (th[i].state & ZK_SP_TR_FOUND);
    if (!any) return ZK_OK;
    SpStagedTraces sv;
    sp_staged_traces(sp, &sv);
    if (!sv.heads || sv.total == 0) return afail(h, ZK_ERR_HIP, "the span store's staging is not there");
    AN_HIP(h, hipSetDevice(h->device));
    // this handle's part: the rows of the asked traces into its staging
    uint32_t parts = 1;
    h->adj_counts_host.resize(n);
    uint32_t* counts = h->adj_counts_host.data();
    if ((st = find_count(h, ids, n, flags, counts, &parts)) != ZK_OK) return st;
    h->base_host.resize(n);
    uint64_t rows_total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        h->base_host[i] = rows_total;
        rows_total += counts[i];
    }
    // the overflowed traces are answered here; the others go on the two work lists, the wave-sized ones first
    h->adj_list_host.clear();
    uint32_t big_spans = kAdjWave, big_rows = kAdjWave, n_wave = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (uint32_t i = 0; i < n; ++i) {
            if (!(th[i].state & ZK_SP_TR_FOUND)) continue;
            const bool over = (th[i].state & ZK_SP_TR_OVERFLOW) || th[i].spans > kAdjMaxSpans || counts[i] > kAdjMaxRows;
            if (over) {
                if (pass) continue;
                zk_an_trace& hd = heads[i];
                hd.trace_id = th[i].trace_id;
                hd.fragments = th[i].fragments;
                hd.state = ZK_SP_TR_FOUND | ZK_AN_ADJ_OVERFLOW;
                if (counts[i]) {
                    hd.state |= ZK_AN_ADJ_ANNOTATED;
                } else {  // not annotated: zk_sp_traces' head of a trace above its bound
                    hd.start = th[i].start;
                    hd.end = th[i].end;
                    hd.state |= ZK_SP_TR_OVERFLOW | (th[i].state & ZK_SP_TR_TIMED);
                }
                continue;
            }
            const bool small = counts[i] <= (uint32_t)kAdjWave && th[i].spans <= (uint32_t)kAdjWave;
            if (small != (pass == 0)) continue;
            h->adj_list_host.push_back(i);
            if (small) ++n_wave;
            if (!small) {
                while (big_spans < th[i].spans) big_spans <<= 1;
                while (big_rows < counts[i]) big_rows <<= 1;
            }
        }
    }
    const uint32_t n_group = (uint32_t)h->adj_list_host.size() - n_wave;
    if (h->adj_list_host.empty()) return ZK_OK;
    // the stagings: a trace emits at most A + 2 S rows, at its row base plus twice its span base
    const uint64_t e_n = rows_total + 2 * sv.total;
    const size_t r8 = Block::col8(e_n), r4 = Block::col4(e_n);
    if (!h->adjt && (st = alloc(h, &h->adjt, kAdjtBytes, "the adjusted traces' heads and work lists")) != ZK_OK) return st;
    if ((st = grow(h, &h->rows, &h->rows_bytes, Block::cols_bytes(rows_total), "the gathered rows (44 B each)")) != ZK_OK) return st;
    if ((st = grow(h, &h->adjt_spans, &h->adjt_spans_bytes, (size_t)sv.total * sizeof(zk_an_span), "the adjusted traces' spans (56 B per fragment)")) != ZK_OK)
        return st;
    if ((st = grow(h, &h->adjt_svc, &h->adjt_svc_bytes, (size_t)sv.total * 4, "the adjusted traces' services (4 B per fragment)")) != ZK_OK) return st;
    if ((st = grow(h, &h->adjt_rows, &h->adjt_rows_bytes, 3 * r8 + 3 * r4, "the adjusted traces' rows (36 B each)")) != ZK_OK) return st;
    uint8_t* qb = (uint8_t*)h->q;
    uint8_t* ab = (uint8_t*)h->adjt;
    const AnCols dev = Block::view(h->rows, rows_total, false);
    AN_HIP(h, hipMemcpyAsync(qb + kQBaseAt, h->base_host.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    if (rows_total) {
        AN_HIP(h, hipMemsetAsync(qb + kQCursorAt, 0, (size_t)n * 4, h->stream));
        AN_HIP(h, launch_checked("k_an_find_write", k_an_find_write, dim3(n, (uint32_t)h->segs.size(), parts), dim3(kAnWG), 0, h->stream,
                                 (const AnCols*)(qb + kQSegsAt), (const unsigned long long*)(qb + kQIdsAt),
                                 (const uint32_t*)(qb + kQCountsAt), (uint32_t*)(qb + kQCursorAt),
                                 (const unsigned long long*)(qb + kQBaseAt), dev));
    }
    AN_HIP(h, hipMemcpyAsync(ab + kAdjtListAt, h->adj_list_host.data(), h->adj_list_host.size() * 4, hipMemcpyHostToDevice, h->stream));
    AN_HIP(h, hipMemsetAsync(ab, 0, (size_t)n * sizeof(zk_an_trace), h->stream));
    AdjEmitIn in;
    in.rows = dev;
    in.list = (const uint32_t*)(ab + kAdjtListAt);
    in.ids = (const unsigned long long*)(qb + kQIdsAt);
    in.counts = (const uint32_t*)(qb + kQCountsAt);
    in.base = (const unsigned long long*)(qb + kQBaseAt);
    in.t_heads = sv.heads;
    in.t_spans = sv.spans;
    in.t_svc = sv.services;
    in.t_base = sv.base;
    in.t_total = sv.total;
    in.cap_spans = in.cap_rows = (uint32_t)kAdjWave;
    in.heads = nullptr;
    in.o_svc = nullptr;
    in.o_first = in.o_last = nullptr;
    in.e_heads = (zk_an_trace*)ab;
    in.e_spans = (zk_an_span*)h->adjt_spans;
    in.e_svc = (uint32_t*)h->adjt_svc;
    uint8_t* rb = (uint8_t*)h->adjt_rows;
    in.e_span = (unsigned long long*)rb;
    in.e_ts = (long long*)(rb + r8);
    in.e_val = (unsigned long long*)(rb + 2 * r8);
    in.e_ip = (uint32_t*)(rb + 3 * r8);
    in.e_rsvc = (uint32_t*)(rb + 3 * r8 + r4);
    in.e_bits = (uint32_t*)(rb + 3 * r8 + 2 * r4);
    in.e_n = e_n;
    in.h_sr = zk_hash_string("sr", 2);
    in.h_ss = zk_hash_string("ss", 2);
    AN_HIP(h, launch_checked("k_an_adjust (emitting, a wave per trace)", k_an_adjust<kAdjWave, AdjEmitIn>, dim3(n_wave), dim3(kAdjWave),
                             adj_lds(kAdjWave, kAdjWave), h->stream, in));
    in.list += n_wave;
    in.cap_spans = big_spans;
    in.cap_rows = big_rows;
    AN_HIP(h, launch_checked("k_an_adjust (emitting, a workgroup per trace)", k_an_adjust<kAnWG, AdjEmitIn>, dim3(n_group), dim3(kAnWG),
                             adj_lds(big_spans, big_rows), h->stream, in));
    // only the heads cross before the totals are known
    h->adjt_heads_host.resize((size_t)n * sizeof(zk_an_trace));
    const zk_an_trace* got = (const zk_an_trace*)h->adjt_heads_host.data();
    AN_HIP(h, hipMemcpyAsync(h->adjt_heads_host.data(), ab, (size_t)n * sizeof(zk_an_trace), hipMemcpyDeviceToHost, h->stream));
    if (h->timing) AN_HIP(h, hipEventRecord(h->qev[1], h->stream));
    AN_HIP(h, hipStreamSynchronize(h->stream));
    h->qtimed = h->timing;
    for (uint32_t i : h->adj_list_host) {
        if (!(got[i].state & ZK_SP_TR_FOUND)) return afail(h, ZK_ERR_HIP, "a listed trace was not adjusted");
        if (got[i].spans > th[i].spans || got[i].services > th[i].services || got[i].rows > (uint64_t)counts[i] + 2ull * th[i].spans)
            return afail(h, ZK_ERR_HIP, "an adjusted trace is larger than its share of the staging");
        heads[i] = got[i];
        totals[0] += got[i].spans;
        totals[1] += got[i].services;
        totals[2] += got[i].rows;
    }
    if (totals[0] > cap_spans || totals[1] > cap_services || totals[2] > cap_rows)
        return afail(h, ZK_ERR_CAPACITY, "an output holds fewer entries than the asked traces have");
    // one copy per output, then each trace's share packed behind the ones before it
    h->adjt_spans_host.resize((size_t)sv.total * sizeof(zk_an_span));
    h->adjt_svc_host.resize((size_t)sv.total * 4);
    AN_HIP(h, hipMemcpyAsync(h->adjt_spans_host.data(), h->adjt_spans, h->adjt_spans_host.size(), hipMemcpyDeviceToHost, h->stream));
    AN_HIP(h, hipMemcpyAsync(h->adjt_svc_host.data(), h->adjt_svc, h->adjt_svc_host.size(), hipMemcpyDeviceToHost, h->stream));
    if (totals[2]) {
        h->adjt_rows_host.resize(3 * r8 + 3 * r4);
        AN_HIP(h, hipMemcpyAsync(h->adjt_rows_host.data(), h->adjt_rows, 3 * r8 + 3 * r4, hipMemcpyDeviceToHost, h->stream));
    }
    if (h->timing) AN_HIP(h, hipEventRecord(h->qev[1], h->stream));
    AN_HIP(h, hipStreamSynchronize(h->stream));
    const zk_an_span* s_spans = (const zk_an_span*)h->adjt_spans_host.data();
    const uint32_t* s_svc = (const uint32_t*)h->adjt_svc_host.data();
    const uint8_t* hr = h->adjt_rows_host.data();
    uint64_t at_s = 0, at_v = 0, at_r = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const zk_an_trace& hd = heads[i];
        const uint64_t from = sv.base_host[i], rfrom = h->base_host[i] + 2 * sv.base_host[i];
        if (hd.spans) memcpy(spans + at_s, s_spans + from, (size_t)hd.spans * sizeof(zk_an_span));
        if (hd.services) memcpy(services + at_v, s_svc + from, (size_t)hd.services * 4);
        if (hd.rows) {
            std::fill(rows->trace_id + at_r, rows->trace_id + at_r + hd.rows, hd.trace_id);
            memcpy(rows->span_id + at_r, (const uint64_t*)hr + rfrom, (size_t)hd.rows * 8);
            memcpy(rows->ts + at_r, (const int64_t*)(hr + r8) + rfrom, (size_t)hd.rows * 8);
            memcpy(rows->value + at_r, (const uint64_t*)(hr + 2 * r8) + rfrom, (size_t)hd.rows * 8);
            memcpy(rows->ipv4 + at_r, (const uint32_t*)(hr + 3 * r8) + rfrom, (size_t)hd.rows * 4);
            memcpy(rows->service_id + at_r, (const uint32_t*)(hr + 3 * r8 + r4) + rfrom, (size_t)hd.rows * 4);
            memcpy(rows->bits + at_r, (const uint32_t*)(hr + 3 * r8 + 2 * r4) + rfrom, (size_t)hd.rows * 4);
        }
        at_s += hd.spans;
        at_v += hd.services;
        at_r += hd.rows;
    }
    return ZK_OK;
    ZK_GUARD_END
}
