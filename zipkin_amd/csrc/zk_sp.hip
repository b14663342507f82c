// zk_sp.hip — the span store by trace id (include/zkspans.h): segments of whole 48-B records grouped by
// a 12-bit hash of the trace id in HBM, and the lookup of asked traces' fragments.
//
// A segment is one allocation of seven columns, trace_id, span_id, parent_id, first_ts, last_ts [8 B],
// service_id, flags [4 B], each 256-B aligned, then off[4097] (u32): the entries of bucket b lie at
// [off[b], off[b + 1]). The host keeps the same offsets.
//
//   k_sp_count    the batch's records per bucket: a per-workgroup LDS histogram of 4096 bins (16 KB),
//                 lanes of a wave that share a bin added once, flushed with atomics. 8 B per record.
//   (host)        the counts' exclusive scan = the segment's offsets; they also start the cursors.
//   k_sp_scatter  a workgroup owns a stretch of the batch and walks it twice: an LDS histogram of its
//                 records' buckets, ONE returning atomic per workgroup and bucket with records to claim
//                 that many places behind the bucket's cursor, then every record again, its rank inside
//                 the workgroup from LDS (zk_ix.hip's k_ix_scatter with the hash for the service; 32 KB of
//                 LDS, so five workgroups share a CU). trace_id is read twice, 48 B per record read and
//                 48 B written.
//   k_sp_merge    one old segment's entries into the merged one: an entry's bucket from its trace id,
//                 its place = the bucket's base for this segment + the entry's index in the old slice.
//   k_sp_find_count, k_sp_find_write   zk_sp_exist's and zk_sp_gather's passes: a workgroup per (asked
//                 id, segment, part of the slice) walks the trace_id slice of the id's bucket; the write
//                 pass appends a wave's matching rows behind the asked id's offset with one returning
//                 atomic per wave. Nothing of a trace is held in LDS: a trace may be of any length.
//   k_sp_summarize   zk_sp_summaries' pass over the rows the write pass staged: one trace per wave (up to 64
//                 rows) or per workgroup (up to ZK_SP_SUM_MAX_ROWS). The head's start, end and counts are
//                 plain reductions; the trace's rows are sorted by (span id, service) in LDS (bitonic, over
//                 16-bit row numbers), first / last / timed folded into each span's first row with LDS
//                 atomics, the first row of every (span, service) pair of a timed span marked as an ENTRY,
//                 and the rows sorted again by (entry, first, span id, service): the entries are then the
//                 leading rows, written behind the trace's row base. 31 B of LDS per row.
//   k_sp_trace    zk_sp_traces' pass over the same staged rows, on the same two work lists: the merged spans
//                 themselves. The rows are sorted by the full canonical key, every span folded onto its
//                 first row (times, the first fragment with a parent, the first named one), its parent found
//                 by binary search, the rows sorted again into span order, the root-most span chosen, the
//                 depths computed by pointer doubling, and a prefix sum over the sorted rows places every span
//                 (48 B) and every (span, service) pair behind the trace's row base. 66 B of LDS per row.
//   k_sp_end_fold, k_sp_end_pins, k_sp_end_mark, k_sp_expire_rewrite   zk_sp_expire's passes: per range of
//                 buckets a scratch table trace id -> end in HBM (the fold over every segment's slice of
//                 the range, 20 B per entry), the pins' verdicts, then one mark bit per entry and the
//                 survivors per (segment, bucket) (8 B per entry); after the sizing synchronisation the
//                 survivors of the mixed segments are scattered into one new segment (k_sp_scatter with the
//                 mark bit as the predicate). The table and the marks are scratch of the call.
//
// Every store is bounded: the scatter, the merge and the rewrite drop a place outside the bucket's slice
// of the segment they write (it cannot arise while the columns stay as they were between the count and the
// scatter, which the header asks of the caller), the lookups clamp a slice to its segment and drop a row
// at or past its asked id's count or the output's size, and the expiry's probes stay inside their table
// and end after `slots` steps.
#include <hip/hip_runtime.h>
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
#include "zkspans.h"

namespace zk {
namespace {

constexpr int kSpWG = 256;
constexpr uint32_t kSpBins = ZK_SP_BUCKETS;
constexpr uint32_t kSpMaxGrid = 4096;
constexpr uint32_t kSpHistGrid = 1024;        // k_sp_count: every workgroup flushes up to 4096 bins
constexpr uint32_t kSpScatterPerWG = 16384;   // k_sp_scatter: records per workgroup at least (4096 atomics each at most)
constexpr uint64_t kSpMaxEntries = 0xFFFFFFFFull;
constexpr int kSpCntItems = 4;                // k_sp_count: records per thread and step
constexpr uint32_t kSpCntTile = kSpWG * kSpCntItems;
constexpr uint32_t kSpPart = 4096;            // the lookups: a slice longer than this is split over workgroups
constexpr uint32_t kSpMaxParts = 64;
constexpr uint64_t kSpMaxFindGrid = 1ull << 20;
constexpr unsigned long long kSpSalt = ZK_SP_SALT;
constexpr unsigned long long kSpEndSalt = ZK_SP_END_SALT;
constexpr unsigned long long kSpSign = 1ull << 63;   // ts ^ sign: the unsigned order is the signed one
constexpr unsigned long long kSpNone = ~0ull;
constexpr uint64_t kSpExpireChunk = 1ull << 24;      // zk_sp_config.expire_chunk's default
constexpr uint64_t kSpEndMinSlots = 1024;
constexpr uint32_t kSpEndGrid = 4096;                // the end-table passes: workgroups per segment at most
constexpr uint32_t kSpMaxItems = 4096;               // the rewrite's work items at most, plus one per segment
constexpr uint32_t kSpSumMaxRows = ZK_SP_SUM_MAX_ROWS;  // the summaries: the longest trace merged on the device
constexpr int kSpSumWave = ZK_SP_SUM_WAVE_ROWS;                     // a trace of up to this many rows gets a wave, a longer one a workgroup
constexpr int kSpSumItems = kSpSumMaxRows / kSpWG;   // rows per thread of the workgroup at most
constexpr uint32_t kSumTimed = 1u, kSumSvc = 2u, kSumSpanTimed = 4u, kSumEntry = 8u;  // a row's byte in LDS
constexpr size_t kSumLdsHead = 32;                   // start, end [8 B], timed, spans, entries [4 B], 4 B unused
constexpr size_t kSumLdsPerRow = 31;                 // span, first, last [8 B], service [4 B], order [2 B], bits [1 B]

static_assert(kSpBins == 4096, "the bucket is the hash's 12 highest bits");
static_assert(kSpSumMaxRows >= 2048 && kSpSumMaxRows <= 65536 && (kSpSumMaxRows & (kSpSumMaxRows - 1)) == 0 &&
                  kSpSumItems * kSpWG == (int)kSpSumMaxRows,
              "the summaries sort 16-bit row numbers over a power of two");
static_assert(kSumLdsHead + kSumLdsPerRow * kSpSumMaxRows <= 65536, "a trace of ZK_SP_SUM_MAX_ROWS rows fits 64 KiB of LDS");
static_assert(sizeof(zk_sp_summary) == 40, "zk_sp_summary's layout");
static_assert(kSpSumWave == 64, "a wave holds one row per lane");

// the merged traces (k_sp_trace): the same bound, work lists and thread shapes as the summaries
constexpr uint32_t kSpTrMaxRows = ZK_SP_TRACE_MAX_ROWS;
constexpr uint32_t kTrNone = 0xFFFFFFFFu;             // no sorted position
constexpr uint32_t kTrNoRow = 0xFFFFu;                // no row number (a 16-bit index)
constexpr uint32_t kTrHead = 1u, kTrSpanTimed = 2u, kTrSeen = 4u;  // a head's bits in LDS
constexpr size_t kTrLdsHead = 64;    // start, end [8 B], timed, spans, root position, root [4 B], the waves' totals [4 x 4 B]
constexpr size_t kTrLdsPerRow = 66;  // span, parent, first, last [8 B], svc, fl, ppos, npos, nsvc, bits [4 B], ord, head, phead, jump, dist [2 B]
static_assert(kSpTrMaxRows == kSpSumMaxRows, "both device merges overflow at the same length");
static_assert(kTrLdsHead + kTrLdsPerRow * kSpTrMaxRows <= 160 * 1024, "a trace of ZK_SP_TRACE_MAX_ROWS rows fits the 160 KiB of a CU");
static_assert(kSpTrMaxRows < kTrNoRow && kSpTrMaxRows < 0x10000u, "row numbers and both prefix sums fit 16 bits");
static_assert(sizeof(zk_sp_trace) == 48 && sizeof(zk_sp_span) == 48, "zk_sp_trace's and zk_sp_span's layouts");
constexpr size_t sp_tr_lds(uint32_t rows) { return kTrLdsHead + kTrLdsPerRow * rows; }

// LDS of one k_sp_summarize workgroup whose launch admits traces of up to `rows` rows (a power of two >= 64)
constexpr size_t sp_sum_lds(uint32_t rows) { return kSumLdsHead + kSumLdsPerRow * rows; }

__host__ __device__ inline uint32_t sp_bucket(unsigned long long id) { return (uint32_t)(zk_mix64(id ^ kSpSalt) >> 52); }

// a segment's columns and offsets as the kernels see them (const), or as the scatter and the merge
// write them
struct SpCols {
    unsigned long long* tid;
    unsigned long long* span;
    unsigned long long* parent;
    long long* first;
    long long* last;
    uint32_t* svc;
    uint32_t* fl;
    uint32_t* off;  // [kSpBins + 1] (a segment), or nullptr (a batch, the lookups' output)
    unsigned long long n;
};
static_assert(sizeof(SpCols) == 72, "the segment table's stride");

// the lookups' block: the asked ids, their counts, the write pass's cursors, the rows' bases, the segments,
// the summaries' work lists
constexpr size_t kQIdsAt = 0;
constexpr size_t kQCountsAt = kQIdsAt + ZK_SP_MAX_IDS * 8;
constexpr size_t kQCursorAt = kQCountsAt + ZK_SP_MAX_IDS * 4;
constexpr size_t kQBaseAt = kQCursorAt + ZK_SP_MAX_IDS * 4;
constexpr size_t kQSegsAt = kQBaseAt + ZK_SP_MAX_IDS * 8;
constexpr size_t kQListAt = kQSegsAt + ZK_SP_MAX_SEGMENTS * sizeof(SpCols);  // the summaries' work lists (asked indices)
constexpr size_t kQBytes = kQListAt + ZK_SP_MAX_IDS * 4;
// the observe's block: the counts, then the cursors
constexpr size_t kObsCursorAt = kSpBins * 4;
constexpr size_t kObsBytes = 2 * kSpBins * 4;
// the expiry's block: the segments (80 B each), the survivors [segment][bucket], the new segment's
// cursors, the full-table counter, the pins (ids ascending, cuts, verdicts), the rewrite's work items
constexpr size_t kXSegsAt = 0;
constexpr size_t kXSurvAt = kXSegsAt + ZK_SP_MAX_SEGMENTS * 80;
constexpr size_t kXCursorAt = kXSurvAt + (size_t)ZK_SP_MAX_SEGMENTS * kSpBins * 4;
constexpr size_t kXFullAt = kXCursorAt + kSpBins * 4;
constexpr size_t kXPinIdsAt = kXFullAt + 256;
constexpr size_t kXPinCutsAt = kXPinIdsAt + ZK_SP_MAX_PINS * 8;
constexpr size_t kXVerdictAt = kXPinCutsAt + ZK_SP_MAX_PINS * 8;
constexpr size_t kXItemsAt = kXVerdictAt + ZK_SP_MAX_PINS * 4;
constexpr size_t kXBytes = kXItemsAt + (size_t)(kSpMaxItems + ZK_SP_MAX_SEGMENTS) * 8;
static_assert(kXSurvAt % 256 == 0 && kXPinIdsAt % 256 == 0 && kXItemsAt % 8 == 0, "the expiry block's alignment");

uint32_t sp_grid(uint64_t items, uint32_t cap = kSpMaxGrid) {
    const uint64_t g = (items + kSpWG - 1) / kSpWG;
    return (uint32_t)(g < 1 ? 1 : g > cap ? cap : g);
}

// ---- observe -------------------------------------------------------------------------------------------
// counts[b] += the records of bucket b. The loop's bounds are the same for all threads of a workgroup,
// so every lane reaches the ballots.
__global__ __launch_bounds__(kSpWG) void k_sp_count(const unsigned long long* __restrict__ tid, unsigned long long n,
                                                    uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_hist[kSpBins];
    for (uint32_t b = threadIdx.x; b < kSpBins; b += kSpWG) s_hist[b] = 0u;
    __syncthreads();
    const unsigned long long stride = (unsigned long long)gridDim.x * kSpCntTile;
    for (unsigned long long base = (unsigned long long)blockIdx.x * kSpCntTile; base < n; base += stride) {
        unsigned long long t[kSpCntItems];  // (the tile's loads first, then the ballots)
#pragma unroll
        for (int j = 0; j < kSpCntItems; ++j) {
            const unsigned long long i = base + (unsigned long long)j * kSpWG + threadIdx.x;
            t[j] = i < n ? tid[i] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < kSpCntItems; ++j)
            hist_add(s_hist, base + (unsigned long long)j * kSpWG + threadIdx.x < n, sp_bucket(t[j]));
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kSpBins; b += kSpWG) {
        const uint32_t c = s_hist[b];
        if (c) atomicAdd(&counts[b], c);
    }
}

// Workgroup w owns records [w * chunk, (w + 1) * chunk) (chunk a multiple of the workgroup). cursor[b]
// starts at the segment's off[b]; a place at or past off[b + 1] is dropped.
__global__ __launch_bounds__(kSpWG) void k_sp_scatter(SpCols in, unsigned long long chunk, uint32_t* __restrict__ cursor, SpCols out) {
    __shared__ uint32_t s_cnt[kSpBins];   // the stretch's records per bucket, then the ranks given out
    __shared__ uint32_t s_base[kSpBins];  // where the workgroup's places of a bucket begin
    const unsigned long long lo = (unsigned long long)blockIdx.x * chunk;
    const unsigned long long hi = lo + chunk < in.n ? lo + chunk : in.n;
    for (uint32_t b = threadIdx.x; b < kSpBins; b += kSpWG) s_cnt[b] = 0u;
    __syncthreads();
    for (unsigned long long base = lo; base < hi; base += kSpCntTile) {
        unsigned long long t[kSpCntItems];
#pragma unroll
        for (int j = 0; j < kSpCntItems; ++j) {
            const unsigned long long i = base + (unsigned long long)j * kSpWG + threadIdx.x;
            t[j] = i < hi ? in.tid[i] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < kSpCntItems; ++j)
            hist_add(s_cnt, base + (unsigned long long)j * kSpWG + threadIdx.x < hi, sp_bucket(t[j]));
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kSpBins; b += kSpWG) {
        const uint32_t c = s_cnt[b];
        s_base[b] = c ? atomicAdd(&cursor[b], c) : 0u;
        s_cnt[b] = 0u;
    }
    __syncthreads();
    for (unsigned long long base = lo; base < hi; base += kSpWG) {
        const unsigned long long i = base + threadIdx.x;
        const bool valid = i < hi;
        const unsigned long long t = valid ? in.tid[i] : 0ull;
        const uint32_t b = sp_bucket(t);
        const uint32_t rank = hist_rank(s_cnt, valid, b);
        if (valid) {
            const unsigned long long at = (unsigned long long)s_base[b] + rank;
            if (at < (unsigned long long)out.off[b + 1] && at < out.n) {
                out.tid[at] = t;
                out.span[at] = in.span[i];
                out.parent[at] = in.parent[i];
                out.first[at] = in.first[i];
                out.last[at] = in.last[i];
                out.svc[at] = in.svc[i];
                out.fl[at] = in.fl[i];
            }
        }
    }
}

// dst_base[b]: where this old segment's slice of bucket b begins in the merged segment
__global__ __launch_bounds__(kSpWG) void k_sp_merge(SpCols src, const uint32_t* __restrict__ dst_base, SpCols dst) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kSpWG;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kSpWG + threadIdx.x; i < src.n; i += stride) {
        const unsigned long long t = src.tid[i];
        const uint32_t b = sp_bucket(t);
        const unsigned long long so = src.off[b];
        if (i < so || i >= (unsigned long long)src.off[b + 1]) continue;  // (not in its bucket's slice: never a scattered entry)
        const unsigned long long at = (unsigned long long)dst_base[b] + (i - so);
        if (at < (unsigned long long)dst.off[b + 1] && at < dst.n) {
            dst.tid[at] = t;
            dst.span[at] = src.span[i];
            dst.parent[at] = src.parent[i];
            dst.first[at] = src.first[i];
            dst.last[at] = src.last[i];
            dst.svc[at] = src.svc[i];
            dst.fl[at] = src.fl[i];
        }
    }
}

// ---- the lookups ---------------------------------------------------------------------------------------
// The grid: x the asked id, y the segment, z the part of the slice. [*a, *e) = this workgroup's stretch
// of the trace_id slice of the id's bucket, clamped to the segment; false when it is empty. The same for
// all threads of a workgroup.
__device__ inline bool sp_stretch(const SpCols& sg, unsigned long long id, unsigned long long* a, unsigned long long* e) {
    const uint32_t b = sp_bucket(id);
    unsigned long long lo = sg.off[b], hi = sg.off[b + 1];
    if (hi > sg.n) hi = sg.n;
    if (lo >= hi) return false;
    const unsigned long long parts = gridDim.z;
    const unsigned long long part = (((hi - lo) + parts - 1) / parts + kSpWG - 1) / kSpWG * kSpWG;
    *a = lo + (unsigned long long)blockIdx.z * part;
    if (*a >= hi) return false;
    *e = *a + part < hi ? *a + part : hi;
    return true;
}

// counts[q] += the entries of segment blockIdx.y whose trace id is ids[q]
__global__ __launch_bounds__(kSpWG) void k_sp_find_count(const SpCols* __restrict__ segs, const unsigned long long* __restrict__ ids,
                                                         uint32_t* __restrict__ counts) {
    const SpCols sg = segs[blockIdx.y];
    const unsigned long long id = ids[blockIdx.x];
    unsigned long long a, e;
    if (!sp_stretch(sg, id, &a, &e)) return;
    uint32_t c = 0;
    for (unsigned long long i = a + threadIdx.x; i < e; i += kSpWG) c += sg.tid[i] == id ? 1u : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if (lane_id() == 0 && c) atomicAdd(&counts[blockIdx.x], c);
}

// The matching rows behind base[q]: a wave draws its matches' places with one returning atomic on
// cursor[q] (from 0); a place at or past counts[q], or a row at or past out.n, is dropped. The loop's
// bounds are the same for all threads of a workgroup, so every lane reaches the ballot and the shuffle.
__global__ __launch_bounds__(kSpWG) void k_sp_find_write(const SpCols* __restrict__ segs, const unsigned long long* __restrict__ ids,
                                                         const uint32_t* __restrict__ counts, uint32_t* __restrict__ cursor,
                                                         const unsigned long long* __restrict__ base, SpCols out) {
    const SpCols sg = segs[blockIdx.y];
    const uint32_t q = blockIdx.x;
    const unsigned long long id = ids[q];
    unsigned long long a, e;
    if (!sp_stretch(sg, id, &a, &e)) return;
    const uint32_t limit = counts[q];
    const unsigned long long row0 = base[q];
    for (unsigned long long tile = a; tile < e; tile += kSpWG) {
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
                out.parent[at] = sg.parent[i];
                out.first[at] = sg.first[i];
                out.last[at] = sg.last[i];
                out.svc[at] = sg.svc[i];
                out.fl[at] = sg.fl[i];
            }
        }
    }
}

// ---- the summaries -------------------------------------------------------------------------------------
// One trace's rows in LDS, by ROW NUMBER (the row's place among the trace's staged rows): span, first and
// last ([8 B]; a time is held ^ sign, an untimed row's first as all ones and its last as 0, the folds'
// neutral values), svc [4 B], bits (one byte: kSumTimed, kSumSvc of the row, then kSumSpanTimed on a span's
// first row and kSumEntry), and ord [2 B]: the row numbers in sorted order; a number at or past n is padding.
struct SpSumRows {
    unsigned long long* span;
    unsigned long long* first;
    unsigned long long* last;
    uint32_t* svc;
    uint16_t* ord;
    uint8_t* bits;
    uint32_t n;
};

// (span id, then the service-bearing rows by service, then the rows without a service); padding last
__device__ inline bool sp_sum_by_span(const SpSumRows& t, uint32_t a, uint32_t b) {
    if (b >= t.n) return a < t.n;
    if (a >= t.n) return false;
    if (t.span[a] != t.span[b]) return t.span[a] < t.span[b];
    const bool sa = t.bits[a] & kSumSvc, sb = t.bits[b] & kSumSvc;
    if (sa != sb) return sa;
    return sa && t.svc[a] < t.svc[b];
}

// the entries first, by (first signed, span id unsigned, service); everything else behind them, in any order
__device__ inline bool sp_sum_by_first(const SpSumRows& t, uint32_t a, uint32_t b) {
    const bool ea = a < t.n && (t.bits[a] & kSumEntry), eb = b < t.n && (t.bits[b] & kSumEntry);
    if (ea != eb) return ea;
    if (!ea) return false;
    if (t.first[a] != t.first[b]) return t.first[a] < t.first[b];
    if (t.span[a] != t.span[b]) return t.span[a] < t.span[b];
    return t.svc[a] < t.svc[b];
}

// A bitonic sort of ord[0, P) (P a power of two >= 2, the same for the whole workgroup): every thread takes
// pairs (i, i | j). Ends behind a barrier.
template <int T, bool (*Less)(const SpSumRows&, uint32_t, uint32_t)>
__device__ inline void sp_sum_sort(const SpSumRows& t, uint32_t P) {
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t w = threadIdx.x; w < P / 2; w += T) {
                const uint32_t i = ((w & ~(j - 1u)) << 1) | (w & (j - 1u)), x = i | j;
                const uint16_t a = t.ord[i], b = t.ord[x];
                if ((i & k) == 0 ? Less(t, b, a) : Less(t, a, b)) {
                    t.ord[i] = b;
                    t.ord[x] = a;
                }
            }
            __syncthreads();
        }
}

// The summary of asked id list[blockIdx.x] from its staged rows [base[q], base[q] + counts[q]): the head
// into heads[q], the entries behind the rows' own base in the entry columns (a trace has at most as many
// entries as rows). T threads hold up to T * I rows; the launch's LDS admits `cap` rows. A trace above
// either, or above ZK_SP_SUM_MAX_ROWS, gets the reductions (fragments, start, end, FOUND, TIMED) and
// OVERFLOW: nothing of it goes to LDS. Every bound that guards a barrier is the same for the whole
// workgroup. The first_ts / last_ts of an untimed row are not loaded.
template <int T, int I>
__global__ __launch_bounds__(T) void k_sp_summarize(SpCols rows, const uint32_t* __restrict__ list,
                                                    const unsigned long long* __restrict__ ids,
                                                    const uint32_t* __restrict__ counts,
                                                    const unsigned long long* __restrict__ base, uint32_t cap,
                                                    zk_sp_summary* __restrict__ heads, uint32_t* __restrict__ e_svc,
                                                    long long* __restrict__ e_first, long long* __restrict__ e_last) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_sum[];
    unsigned long long* s_start = (unsigned long long*)s_sum;
    unsigned long long* s_end = s_start + 1;
    uint32_t* s_cnt = (uint32_t*)(s_sum + 16);  // timed, spans, entries
    const uint32_t q = list[blockIdx.x];
    const uint32_t n = counts[q];
    const unsigned long long r0 = base[q];
    if (n == 0 || r0 + n > rows.n) return;  // (not a staged trace: never on a work list)
    const bool fits = n <= cap && n <= kSpSumMaxRows && n <= (uint32_t)(T * I);
    SpSumRows t;
    t.span = (unsigned long long*)(s_sum + kSumLdsHead);
    t.first = t.span + cap;
    t.last = t.first + cap;
    t.svc = (uint32_t*)(t.last + cap);
    t.ord = (uint16_t*)(t.svc + cap);
    t.bits = (uint8_t*)(t.ord + cap);
    t.n = n;
    uint32_t P = 2;
    while (P < n && P < cap) P <<= 1;
    if (threadIdx.x == 0) {
        *s_start = kSpNone;
        *s_end = 0ull;
        s_cnt[0] = s_cnt[1] = s_cnt[2] = 0u;
    }
    __syncthreads();
    unsigned long long lo = kSpNone, hi = 0ull;
    bool any = false;
    for (uint32_t i = threadIdx.x; i < n; i += T) {
        const unsigned long long at = r0 + i;
        const uint32_t f = rows.fl[at];
        const bool timed = f & ZK_F_HAS_ANNOTATIONS;
        const unsigned long long a = timed ? (unsigned long long)rows.first[at] ^ kSpSign : kSpNone;
        const unsigned long long z = timed ? (unsigned long long)rows.last[at] ^ kSpSign : 0ull;
        lo = a < lo ? a : lo;
        hi = z > hi ? z : hi;
        any |= timed;
        if (fits) {
            t.span[i] = rows.span[at];
            t.first[i] = a;
            t.last[i] = z;
            t.svc[i] = rows.svc[at];
            t.bits[i] = (uint8_t)((timed ? kSumTimed : 0u) | (f & (ZK_F_SVC_CLIENT | ZK_F_SVC_SERVER) ? kSumSvc : 0u));
        }
    }
    if (fits)
        for (uint32_t i = threadIdx.x; i < P; i += T) t.ord[i] = (uint16_t)i;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ol = __shfl_down(lo, off), oh = __shfl_down(hi, off);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    const bool wave_any = __ballot(any) != 0ull;
    if (lane_id() == 0 && wave_any) {
        atomicMin(s_start, lo);
        atomicMax(s_end, hi);
        atomicOr(&s_cnt[0], 1u);
    }
    __syncthreads();
    if (!fits) {
        if (threadIdx.x == 0) {
            const bool timed = s_cnt[0] != 0u;
            zk_sp_summary hd;
            hd.trace_id = ids[q];
            hd.start = timed ? (long long)(*s_start ^ kSpSign) : 0;
            hd.end = timed ? (long long)(*s_end ^ kSpSign) : 0;
            hd.fragments = n;
            hd.spans = 0u;
            hd.span_ts = 0u;
            hd.state = ZK_SP_SUM_FOUND | (timed ? ZK_SP_SUM_TIMED : 0u) | ZK_SP_SUM_OVERFLOW;
            heads[q] = hd;
        }
        return;
    }
    sp_sum_sort<T, sp_sum_by_span>(t, P);
    // The fold: a row finds its span's first row in the sorted order (a binary search over the span ids) and
    // folds its times into that row's. Only first rows are updated, and only with atomics; what the others
    // read here (their own times, every row's span id and low bits) does not change. The bits' atomic is on
    // the byte's 32-bit word and sets kSumSpanTimed alone.
    uint32_t* bits_w = (uint32_t*)t.bits;
    uint32_t head_of[I];
#pragma unroll
    for (int k = 0; k < I; ++k) {
        const uint32_t p = threadIdx.x + (uint32_t)k * T;
        head_of[k] = 0u;
        if (p < n) {
            const uint32_t r = t.ord[p];
            const unsigned long long s = t.span[r];
            uint32_t a = 0, z = p;
            while (a < z) {
                const uint32_t mid = (a + z) >> 1;
                if (t.span[t.ord[mid]] < s) a = mid + 1; else z = mid;
            }
            const uint32_t h = t.ord[a];
            head_of[k] = h;
            if (a == p) atomicAdd(&s_cnt[1], 1u);
            if (t.bits[r] & kSumTimed) {
                if (a != p) {
                    atomicMin(&t.first[h], t.first[r]);
                    atomicMax(&t.last[h], t.last[r]);
                }
                atomicOr(&bits_w[h >> 2], kSumSpanTimed << (8u * (h & 3u)));
            }
        }
    }
    __syncthreads();
    // every row takes its span's times; the first row of a (span, service) pair of a timed span is an entry
    unsigned long long sf[I], sl[I];
    bool entry[I];
#pragma unroll
    for (int k = 0; k < I; ++k) {
        const uint32_t p = threadIdx.x + (uint32_t)k * T;
        sf[k] = sl[k] = 0ull;
        entry[k] = false;
        if (p < n) {
            const uint32_t r = t.ord[p], h = head_of[k];
            sf[k] = t.first[h];
            sl[k] = t.last[h];
            bool e = (t.bits[r] & kSumSvc) && (t.bits[h] & kSumSpanTimed);
            if (e && p > 0) {
                const uint32_t prev = t.ord[p - 1];
                if (t.span[prev] == t.span[r] && (t.bits[prev] & kSumSvc) && t.svc[prev] == t.svc[r]) e = false;
            }
            entry[k] = e;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < I; ++k) {
        const uint32_t p = threadIdx.x + (uint32_t)k * T;
        if (p < n) {
            const uint32_t r = t.ord[p];
            t.first[r] = sf[k];
            t.last[r] = sl[k];
            if (entry[k]) {
                t.bits[r] = (uint8_t)(t.bits[r] | kSumEntry);
                atomicAdd(&s_cnt[2], 1u);
            }
        }
    }
    __syncthreads();
    sp_sum_sort<T, sp_sum_by_first>(t, P);
    const uint32_t E = s_cnt[2] < n ? s_cnt[2] : n;
    for (uint32_t p = threadIdx.x; p < E; p += T) {
        const uint32_t r = t.ord[p];
        const unsigned long long at = r0 + p;  // (p < n: inside the trace's own rows, r0 + n <= rows.n)
        if (r < n) {
            e_svc[at] = t.svc[r];
            e_first[at] = (long long)(t.first[r] ^ kSpSign);
            e_last[at] = (long long)(t.last[r] ^ kSpSign);
        }
    }
    if (threadIdx.x == 0) {
        const bool timed = s_cnt[0] != 0u;
        zk_sp_summary hd;
        hd.trace_id = ids[q];
        hd.start = timed ? (long long)(*s_start ^ kSpSign) : 0;
        hd.end = timed ? (long long)(*s_end ^ kSpSign) : 0;
        hd.fragments = n;
        hd.spans = s_cnt[1];
        hd.span_ts = E;
        hd.state = ZK_SP_SUM_FOUND | (timed ? ZK_SP_SUM_TIMED : 0u);
        heads[q] = hd;
    }
}

// ---- the merged traces ---------------------------------------------------------------------------------
// One trace's rows in LDS for k_sp_trace, by ROW NUMBER. Of every row: span, parent, first, last ([8 B]; the
// times RAW ^ sign until the first sort is done, then the row's contribution to its span's times, all ones /
// 0 for an untimed row), svc, fl [4 B], head [2 B]: the row number of its span's HEAD, the span's first row in
// canonical order. A head carries its span: first / last folded, parent = the span's parent id, ppos / npos
// [4 B]: the first sorted position of a fragment with a parent / with a name (all ones: none; npos then
// becomes the name id), nsvc [4 B]: the span's (span, service) pairs, bits [4 B], phead [2 B]: the head of
// its parent (kTrNoRow: not a span of the trace), jump / dist [2 B]: the pointer doubling's state. ord
// [2 B]: the row numbers in sorted order; a number at or past n is padding.
struct SpTrRows {
    unsigned long long* span;
    unsigned long long* parent;
    unsigned long long* first;
    unsigned long long* last;
    uint32_t* svc;
    uint32_t* fl;
    uint32_t* ppos;
    uint32_t* npos;
    uint32_t* nsvc;
    uint32_t* bits;
    uint16_t* ord;
    uint16_t* head;
    uint16_t* phead;
    uint16_t* jump;
    uint16_t* dist;
    uint32_t n;
};

__device__ inline bool sp_tr_has_svc(uint32_t fl) { return (fl & (ZK_F_SVC_CLIENT | ZK_F_SVC_SERVER)) != 0u; }

// the header's canonical order inside a trace (the times are held ^ sign); padding last
__device__ inline bool sp_tr_canonical(const SpTrRows& t, uint32_t a, uint32_t b) {
    if (b >= t.n) return a < t.n;
    if (a >= t.n) return false;
    if (t.span[a] != t.span[b]) return t.span[a] < t.span[b];
    if (t.parent[a] != t.parent[b]) return t.parent[a] < t.parent[b];
    if (t.first[a] != t.first[b]) return t.first[a] < t.first[b];
    if (t.last[a] != t.last[b]) return t.last[a] < t.last[b];
    if (t.svc[a] != t.svc[b]) return t.svc[a] < t.svc[b];
    return t.fl[a] < t.fl[b];
}

// SPAN ORDER over all rows: (the span's first, an untimed span's being all ones = INT64_MAX ^ sign; span id),
// inside a span the service-bearing rows by service, then the rest; padding last
__device__ inline bool sp_tr_span_order(const SpTrRows& t, uint32_t a, uint32_t b) {
    if (b >= t.n) return a < t.n;
    if (a >= t.n) return false;
    const uint32_t ha = t.head[a], hb = t.head[b];
    if (ha != hb) {
        if (t.first[ha] != t.first[hb]) return t.first[ha] < t.first[hb];
        return t.span[a] < t.span[b];
    }
    const bool sa = sp_tr_has_svc(t.fl[a]), sb = sp_tr_has_svc(t.fl[b]);
    if (sa != sb) return sa;
    return sa && t.svc[a] < t.svc[b];
}

// sp_sum_sort over SpTrRows: a bitonic sort of ord[0, P) (P a power of two >= 2, the same for the whole
// workgroup). Ends behind a barrier.
template <int T, bool (*Less)(const SpTrRows&, uint32_t, uint32_t)>
__device__ inline void sp_tr_sort(const SpTrRows& t, uint32_t P) {
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t w = threadIdx.x; w < P / 2; w += T) {
                const uint32_t i = ((w & ~(j - 1u)) << 1) | (w & (j - 1u)), x = i | j;
                const uint16_t a = t.ord[i], b = t.ord[x];
                if ((i & k) == 0 ? Less(t, b, a) : Less(t, a, b)) {
                    t.ord[i] = b;
                    t.ord[x] = a;
                }
            }
            __syncthreads();
        }
}

// the first sorted position in [0, hi) whose row's span id is not below s (ord in canonical order)
__device__ inline uint32_t sp_tr_lower(const SpTrRows& t, unsigned long long s, uint32_t hi) {
    uint32_t a = 0, z = hi;
    while (a < z) {
        const uint32_t mid = (a + z) >> 1;
        if (t.span[t.ord[mid]] < s) a = mid + 1; else z = mid;
    }
    return a;
}

// The merged trace of asked id list[blockIdx.x] from its staged rows [base[q], base[q] + counts[q]): the head
// into heads[q]; its spans, in span order, and its (span, service) pairs behind the rows' OWN base in o_spans
// and o_svc (a trace has at most as many spans, and as many pairs, as rows: no prefix sum over the traces is
// needed, and the host packs per trace). T threads hold up to T * I rows; the launch's LDS admits `cap` rows.
// A trace above either, or above ZK_SP_TRACE_MAX_ROWS, gets the reductions and OVERFLOW: nothing of it goes to
// LDS. Every bound that guards a barrier (n, cap, P, the span count) is the same for the whole workgroup.
template <int T, int I>
__global__ __launch_bounds__(T) void k_sp_trace(SpCols rows, const uint32_t* __restrict__ list,
                                                const unsigned long long* __restrict__ ids,
                                                const uint32_t* __restrict__ counts,
                                                const unsigned long long* __restrict__ base, uint32_t cap,
                                                zk_sp_trace* __restrict__ heads, zk_sp_span* __restrict__ o_spans,
                                                uint32_t* __restrict__ o_svc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_tr[];
    unsigned long long* s_start = (unsigned long long*)s_tr;
    unsigned long long* s_end = s_start + 1;
    uint32_t* s_cnt = (uint32_t*)(s_tr + 16);   // timed, spans, the root-most span's sorted position, its head
    uint32_t* s_wave = (uint32_t*)(s_tr + 32);  // the prefix sum's totals per wave (T / 64 <= 4 of them)
    const uint32_t q = list[blockIdx.x];
    const uint32_t n = counts[q];
    const unsigned long long r0 = base[q];
    if (n == 0 || r0 + n > rows.n) return;  // (not a staged trace: never on a work list)
    const bool fits = n <= cap && n <= kSpTrMaxRows && n <= (uint32_t)(T * I);
    SpTrRows t;
    t.span = (unsigned long long*)(s_tr + kTrLdsHead);
    t.parent = t.span + cap;
    t.first = t.parent + cap;
    t.last = t.first + cap;
    t.svc = (uint32_t*)(t.last + cap);
    t.fl = t.svc + cap;
    t.ppos = t.fl + cap;
    t.npos = t.ppos + cap;
    t.nsvc = t.npos + cap;
    t.bits = t.nsvc + cap;
    t.ord = (uint16_t*)(t.bits + cap);
    t.head = t.ord + cap;
    t.phead = t.head + cap;
    t.jump = t.phead + cap;
    t.dist = t.jump + cap;
    t.n = n;
    uint32_t P = 2;
    while (P < n && P < cap) P <<= 1;
    if (threadIdx.x == 0) {
        *s_start = kSpNone;
        *s_end = 0ull;
        s_cnt[0] = s_cnt[1] = 0u;
        s_cnt[2] = s_cnt[3] = kTrNone;
    }
    __syncthreads();
    // 1. the rows into LDS (the raw times of untimed rows too: the canonical order reads them), the reductions
    unsigned long long lo = kSpNone, hi = 0ull;
    bool any = false;
    for (uint32_t i = threadIdx.x; i < n; i += T) {
        const unsigned long long at = r0 + i;
        const uint32_t f = rows.fl[at];
        const bool timed = f & ZK_F_HAS_ANNOTATIONS;
        if (timed || fits) {
            const unsigned long long a = (unsigned long long)rows.first[at] ^ kSpSign;
            const unsigned long long z = (unsigned long long)rows.last[at] ^ kSpSign;
            if (timed) {
                lo = a < lo ? a : lo;
                hi = z > hi ? z : hi;
                any = true;
            }
            if (fits) {
                t.span[i] = rows.span[at];
                t.parent[i] = rows.parent[at];
                t.first[i] = a;
                t.last[i] = z;
                t.svc[i] = rows.svc[at];
                t.fl[i] = f;
                t.ppos[i] = t.npos[i] = kTrNone;
                t.nsvc[i] = 0u;
                t.bits[i] = 0u;
                t.phead[i] = kTrNoRow;
            }
        }
    }
    if (fits)
        for (uint32_t i = threadIdx.x; i < P; i += T) t.ord[i] = (uint16_t)i;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ol = __shfl_down(lo, off), oh = __shfl_down(hi, off);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    const bool wave_any = __ballot(any) != 0ull;
    if (lane_id() == 0 && wave_any) {
        atomicMin(s_start, lo);
        atomicMax(s_end, hi);
        atomicOr(&s_cnt[0], 1u);
    }
    __syncthreads();
    zk_sp_trace hd;
    hd.trace_id = ids[q];
    hd.start = s_cnt[0] ? (long long)(*s_start ^ kSpSign) : 0;
    hd.end = s_cnt[0] ? (long long)(*s_end ^ kSpSign) : 0;
    hd.root_most = 0ull;
    hd.fragments = n;
    hd.spans = hd.services = 0u;
    hd.state = ZK_SP_TR_FOUND | (s_cnt[0] ? ZK_SP_TR_TIMED : 0u);
    if (!fits) {
        hd.state |= ZK_SP_TR_OVERFLOW;
        if (threadIdx.x == 0) heads[q] = hd;
        return;
    }
    // 2. canonical order: the rows of a span lie together, the first with a parent and the first named first
    sp_tr_sort<T, sp_tr_canonical>(t, P);
    // 3. the fold. Every row finds its span's head; its own times become its contribution to the span's.
    uint32_t head_of[I];
#pragma unroll
    for (int k = 0; k < I; ++k) {
        const uint32_t p = threadIdx.x + (uint32_t)k * T;
        head_of[k] = kTrNoRow;
        if (p < n) {
            const uint32_t r = t.ord[p];
            const uint32_t a = sp_tr_lower(t, t.span[r], p);
            const uint32_t h = t.ord[a];
            head_of[k] = h;
            t.head[r] = (uint16_t)h;
            if (!(t.fl[r] & ZK_F_HAS_ANNOTATIONS)) {
                t.first[r] = kSpNone;
                t.last[r] = 0ull;
            }
            if (a == p) {
                t.bits[r] = kTrHead;
                atomicAdd(&s_cnt[1], 1u);
            }
        }
    }
    __syncthreads();
    // only heads are updated, and only with atomics; what the others read here does not change
#pragma unroll
    for (int k = 0; k < I; ++k) {
        const uint32_t p = threadIdx.x + (uint32_t)k * T;
        if (p < n) {
            const uint32_t r = t.ord[p], h = head_of[k], f = t.fl[r];
            if (f & ZK_F_HAS_ANNOTATIONS) {
                if (h != r) {
                    atomicMin(&t.first[h], t.first[r]);
                    atomicMax(&t.last[h], t.last[r]);
                }
                atomicOr(&t.bits[h], kTrSpanTimed);
            }
            if (f & ZK_F_HAS_PARENT) atomicMin(&t.ppos[h], p);
            if (f >> ZK_F_NAME_SHIFT) atomicMin(&t.npos[h], p);
        }
    }
    __syncthreads();
    // 4. per span (its head's thread): the parent id, the parent's head by binary search, the name id. A head
    // reads and writes rows of its own span alone, and every head's span id.
#pragma unroll
    for (int k = 0; k < I; ++k) {
        const uint32_t p = threadIdx.x + (uint32_t)k * T;
        if (p < n && head_of[k] == t.ord[p]) {
            const uint32_t h = head_of[k];
            const uint32_t pp = t.ppos[h], np = t.npos[h];
            if (pp < n) {
                const unsigned long long pid = t.parent[t.ord[pp]];
                t.parent[h] = pid;
                const uint32_t a = sp_tr_lower(t, pid, n);
                if (a < n && t.span[t.ord[a]] == pid) t.phead[h] = t.ord[a];
            }
            t.npos[h] = np < n ? t.fl[t.ord[np]] >> ZK_F_NAME_SHIFT : 0u;
        }
    }
    __syncthreads();
    // 5. span order; equal (span, service) pairs lie together
    sp_tr_sort<T, sp_tr_span_order>(t, P);
    // 6. over the sorted positions, I consecutive ones per thread: a span's first position, a pair's first
    // position (counted into the span), the first span without a parent; the prefix sum of both marks
    // (16 bits each in one word: at most n <= 2048 of either)
    uint32_t mark[I], sum = 0u;
#pragma unroll
    for (int k = 0; k < I; ++k) {
        const uint32_t p = threadIdx.x * (uint32_t)I + (uint32_t)k;
        mark[k] = 0u;
        if (p < n) {
            const uint32_t r = t.ord[p], h = t.head[r];
            const uint32_t prev = p ? t.ord[p - 1] : r;
            const bool start = p == 0 || t.head[prev] != h;
            const bool pair = sp_tr_has_svc(t.fl[r]) && (start || !sp_tr_has_svc(t.fl[prev]) || t.svc[prev] != t.svc[r]);
            if (pair) atomicAdd(&t.nsvc[h], 1u);
            if (start && t.ppos[h] == kTrNone) atomicMin(&s_cnt[2], p);
            mark[k] = (start ? 1u : 0u) | (pair ? 0x10000u : 0u);
            sum += mark[k];
        }
    }
    uint32_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if ((int)lane_id() >= d) inc += o;
    }
    if (lane_id() == 63) s_wave[threadIdx.x >> 6] = inc;
    __syncthreads();
    // 7. the root-most span: the first span in span order without a parent, else one lane walks up from the
    // first span through the parents the trace holds, to a span without one here or to the first it meets twice
    if (threadIdx.x == 0) {
        uint32_t s;
        if (s_cnt[2] < n) {
            s = t.head[t.ord[s_cnt[2]]];
        } else {
            s = t.head[t.ord[0]];
            for (uint32_t step = 0; step < n && t.phead[s] != kTrNoRow && !(t.bits[s] & kTrSeen); ++step) {
                t.bits[s] |= kTrSeen;
                s = t.phead[s];
            }
        }
        s_cnt[3] = s;
    }
    __syncthreads();
    const uint32_t root = s_cnt[3], S = s_cnt[1];
    // 8. the depths by pointer doubling over the heads: (jump, dist) = an ancestor and the hops to it. The
    // root-most span and a span whose parent is not in the trace (or is itself) are terminals, jump = self.
    // After ceil(log2(S)) rounds every chain that ends has reached its terminal; one that does not (a cycle
    // away from the root-most span) has dist <= 2^rounds <= 2048.
    for (uint32_t r = threadIdx.x; r < n; r += T)
        if (t.bits[r] & kTrHead) {
            const bool term = r == root || t.phead[r] == kTrNoRow;
            t.jump[r] = (uint16_t)(term ? r : t.phead[r]);
            t.dist[r] = term ? 0 : 1;
        }
    __syncthreads();
    for (uint32_t reach = 1; reach < S; reach <<= 1) {
        uint16_t nj[I], nd[I];
#pragma unroll
        for (int k = 0; k < I; ++k) {
            const uint32_t r = threadIdx.x + (uint32_t)k * T;
            nj[k] = kTrNoRow;
            nd[k] = 0;
            if (r < n && (t.bits[r] & kTrHead)) {
                const uint32_t j = t.jump[r], jj = t.jump[j];
                if (jj != j) {
                    nj[k] = (uint16_t)jj;
                    nd[k] = (uint16_t)(t.dist[r] + t.dist[j]);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < I; ++k) {
            const uint32_t r = threadIdx.x + (uint32_t)k * T;
            if (nj[k] != kTrNoRow) {
                t.jump[r] = nj[k];
                t.dist[r] = nd[k];
            }
        }
        __syncthreads();
    }
    // 9. the spans and the pairs behind the trace's own row base (places < n: r0 + n <= rows.n)
    uint32_t before = inc - sum;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) before += s_wave[w];
#pragma unroll
    for (int k = 0; k < I; ++k) {
        const uint32_t p = threadIdx.x * (uint32_t)I + (uint32_t)k;
        if (p < n) {
            const uint32_t r = t.ord[p];
            const uint32_t si = before & 0xFFFFu, pi = before >> 16;
            if ((mark[k] & 1u) && si < n) {
                const uint32_t h = t.head[r];
                const bool timed = t.bits[h] & kTrSpanTimed, has_parent = t.ppos[h] != kTrNone;
                zk_sp_span o;
                o.span_id = t.span[h];
                o.parent_id = has_parent ? t.parent[h] : 0ull;
                o.first = timed ? (long long)(t.first[h] ^ kSpSign) : 0;
                o.last = timed ? (long long)(t.last[h] ^ kSpSign) : 0;
                o.name = t.npos[h];
                o.depth = t.jump[h] == root ? (uint32_t)t.dist[h] + 1u : 0u;
                o.services = t.nsvc[h];
                o.bits = (has_parent ? ZK_SP_SPAN_HAS_PARENT : 0u) | (timed ? ZK_SP_SPAN_TIMED : 0u) |
                         (t.phead[h] != kTrNoRow ? ZK_SP_SPAN_PARENT_FOUND : 0u) | (h == root ? ZK_SP_SPAN_ROOT_MOST : 0u);
                o_spans[r0 + si] = o;
            }
            if ((mark[k] & 0x10000u) && pi < n) o_svc[r0 + pi] = t.svc[r];
            before += mark[k];
        }
    }
    if (threadIdx.x == 0) {
        uint32_t all = 0u;
        for (uint32_t w = 0; w < (uint32_t)(T / 64); ++w) all += s_wave[w];
        hd.root_most = t.span[root];
        hd.spans = all & 0xFFFFu;
        hd.services = all >> 16;
        heads[q] = hd;
    }
}

// ---- expiry --------------------------------------------------------------------------------------------
// A segment as the expiry's passes see it: its columns and where its mark words begin.
struct SpXSeg {
    SpCols c;
    unsigned long long mark_at;
};
struct SpItem {
    uint32_t seg, chunk;
};
static_assert(sizeof(SpXSeg) == 80 && sizeof(SpItem) == 8, "the expiry plan's layouts");

__device__ inline unsigned long long sp_end_home(unsigned long long id, unsigned long long slots) {
    return zk_mix64(id ^ kSpEndSalt) & (slots - 1ull);
}

// [*lo, *hi): the slice of buckets [b0, b1) (b0 < b1 <= kSpBins) in the segment, clamped to it
__device__ inline void sp_range(const SpCols& sg, uint32_t b0, uint32_t b1, unsigned long long* lo, unsigned long long* hi) {
    unsigned long long a = sg.off[b0], e = sg.off[b1];
    if (e > sg.n) e = sg.n;
    if (a > e) a = e;
    *lo = a;
    *hi = e;
}

// The slot of `id` in the scratch table (slots a power of two; tab[2 * s] the key, tab[2 * s + 1] the end;
// trace id 0 has the slot behind the table, its key held as 1), or kAllOnes when it is not there. A probe
// ends at an empty slot or after `slots` steps.
__device__ inline unsigned long long sp_end_find(const unsigned long long* tab, unsigned long long slots, unsigned long long id) {
    if (id == 0ull) return tab[2 * slots] != 0ull ? slots : kSpNone;
    unsigned long long s = sp_end_home(id, slots);
    for (unsigned long long tries = 0; tries < slots; ++tries) {
        const unsigned long long k = tab[2 * s];
        if (k == id) return s;
        if (k == 0ull) return kSpNone;
        s = (s + 1ull) & (slots - 1ull);
    }
    return kSpNone;
}

// end[trace] = max over the TIMED entries of the range's slices of last_ts ^ sign; an untimed entry claims
// its key and leaves the end at its floor, 0 (the table is cleared to zeros). grid.y = the segment.
// A wave owns rows of 64 consecutive entries and folds each RUN of equal trace ids in a row first (a
// segmented max over the lanes, log2 steps): only a run's first lane goes to the table. The scatter keeps
// a batch's neighbours neighbours inside a bucket's slice, so a trace's fragments mostly form runs, and
// without this every fragment of a trace in flight pays a CAS and a max on the same two words. The plain
// loads are hints: a key never changes once claimed and an end only rises, so a stale word costs an atomic,
// never an answer. A table that ran full (it cannot at load <= 1/2) is counted in *full. The rows' bounds
// are wave-uniform, so every lane reaches the shuffles.
__global__ __launch_bounds__(kSpWG) void k_sp_end_fold(const SpXSeg* __restrict__ segs, uint32_t b0, uint32_t b1,
                                                       unsigned long long* tab, unsigned long long slots,
                                                       unsigned long long* __restrict__ full) {
    const SpCols sg = segs[blockIdx.y].c;
    unsigned long long lo, hi;
    sp_range(sg, b0, b1, &lo, &hi);
    const unsigned long long stride = (unsigned long long)gridDim.x * kSpWG;
    const uint32_t lane = lane_id();
    for (unsigned long long base = lo + (unsigned long long)blockIdx.x * kSpWG + (threadIdx.x - lane); base < hi; base += stride) {
        const unsigned long long i = base + lane;
        const bool valid = i < hi;
        const unsigned long long id = valid ? sg.tid[i] : 0ull;
        unsigned long long val = valid && (sg.fl[i] & ZK_F_HAS_ANNOTATIONS) ? (unsigned long long)sg.last[i] ^ kSpSign : 0ull;
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
        unsigned long long s = id ? sp_end_home(id, slots) : slots, tries = 0;
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
// 1 = goes, 2 = stays (0: never met), and its end becomes kAllOnes, which sends the mark pass to the
// verdicts. A pin's id lies in one bucket, so in one range: a verdict is written once.
__global__ __launch_bounds__(kSpWG) void k_sp_end_pins(const unsigned long long* __restrict__ ids,
                                                       const unsigned long long* __restrict__ cuts, uint32_t n, uint32_t b0,
                                                       uint32_t b1, unsigned long long* tab, unsigned long long slots,
                                                       uint32_t* __restrict__ verdict) {
    const uint32_t p = blockIdx.x * kSpWG + threadIdx.x;
    if (p >= n) return;
    const unsigned long long id = ids[p];
    const uint32_t b = sp_bucket(id);
    if (b < b0 || b >= b1) return;
    const unsigned long long s = sp_end_find(tab, slots, id);
    if (s == kSpNone) return;
    verdict[p] = tab[2 * s + 1] >= cuts[p] ? 2u : 1u;
    tab[2 * s + 1] = kSpNone;
}

// Entry i of the range's slice of segment blockIdx.y survives when its trace's end is >= cut, or by its
// pin's verdict. A wave owns the 64 entries of one mark word (the slice's edges inside a word are masked
// out, and words of different ranges are ORed: the ranges run one after another), writes its ballot with
// one atomic and adds its survivors to surv[segment][bucket], the lanes of one bucket at once. All bounds
// of the loop are wave-uniform, so every lane reaches the ballots.
__global__ __launch_bounds__(kSpWG) void k_sp_end_mark(const SpXSeg* __restrict__ segs, uint32_t b0, uint32_t b1,
                                                       const unsigned long long* __restrict__ tab, unsigned long long slots,
                                                       unsigned long long cut, const unsigned long long* __restrict__ pin_ids,
                                                       const uint32_t* __restrict__ verdict, uint32_t n_pins,
                                                       unsigned long long* __restrict__ marks, uint32_t* __restrict__ surv) {
    const SpXSeg xs = segs[blockIdx.y];
    const SpCols sg = xs.c;
    unsigned long long lo, hi;
    sp_range(sg, b0, b1, &lo, &hi);
    if (lo >= hi) return;
    const unsigned long long w_hi = (hi + 63ull) >> 6, wstride = (unsigned long long)gridDim.x * (kSpWG / 64);
    for (unsigned long long w = (lo >> 6) + (unsigned long long)blockIdx.x * (kSpWG / 64) + (threadIdx.x >> 6); w < w_hi; w += wstride) {
        const unsigned long long i = (w << 6) + lane_id();
        bool alive = false;
        uint32_t b = 0;
        if (i >= lo && i < hi) {
            const unsigned long long id = sg.tid[i];
            b = sp_bucket(id);
            const unsigned long long s = b >= b0 && b < b1 ? sp_end_find(tab, slots, id) : kSpNone;
            if (s != kSpNone) {
                const unsigned long long e = tab[2 * s + 1];
                alive = e >= cut;
                if (e == kSpNone && n_pins) {  // a pinned trace, or an end at INT64_MAX (which stays at any cut)
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
            if ((int)lane_id() == lead) atomicAdd(&surv[(size_t)blockIdx.y * kSpBins + lb], (uint32_t)__popcll(same));  // (lb < kSpBins)
            if (b == lb) todo = false;
        }
    }
}

// k_sp_scatter over a stretch of an old segment, for the marked entries only: the mark bits are read for
// every entry, trace_id (twice) and the other six columns for survivors. cursor[b] starts at the new
// segment's off[b]; a place at or past off[b + 1] is dropped.
__global__ __launch_bounds__(kSpWG) void k_sp_expire_rewrite(const SpXSeg* __restrict__ segs, const SpItem* __restrict__ items,
                                                             unsigned long long chunk, const unsigned long long* __restrict__ marks,
                                                             uint32_t* __restrict__ cursor, SpCols out) {
    __shared__ uint32_t s_cnt[kSpBins];
    __shared__ uint32_t s_base[kSpBins];
    const SpItem it = items[blockIdx.x];
    const SpXSeg xs = segs[it.seg];
    const SpCols in = xs.c;
    const unsigned long long lo = (unsigned long long)it.chunk * chunk;  // (a multiple of the workgroup: a wave's 64 entries share a mark word)
    if (lo >= in.n) return;  // (the same for the whole workgroup)
    const unsigned long long hi = lo + chunk < in.n ? lo + chunk : in.n;
    for (uint32_t b = threadIdx.x; b < kSpBins; b += kSpWG) s_cnt[b] = 0u;
    __syncthreads();
    for (unsigned long long base = lo; base < hi; base += kSpWG) {
        const unsigned long long i = base + threadIdx.x;
        const bool keep = i < hi && ((marks[xs.mark_at + (i >> 6)] >> (i & 63ull)) & 1ull);
        const unsigned long long t = keep ? in.tid[i] : 0ull;
        hist_add(s_cnt, keep, sp_bucket(t));
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kSpBins; b += kSpWG) {
        const uint32_t c = s_cnt[b];
        s_base[b] = c ? atomicAdd(&cursor[b], c) : 0u;
        s_cnt[b] = 0u;
    }
    __syncthreads();
    for (unsigned long long base = lo; base < hi; base += kSpWG) {
        const unsigned long long i = base + threadIdx.x;
        const bool keep = i < hi && ((marks[xs.mark_at + (i >> 6)] >> (i & 63ull)) & 1ull);
        const unsigned long long t = keep ? in.tid[i] : 0ull;
        const uint32_t b = sp_bucket(t);
        const uint32_t rank = hist_rank(s_cnt, keep, b);
        if (keep) {
            const unsigned long long at = (unsigned long long)s_base[b] + rank;
            if (at < (unsigned long long)out.off[b + 1] && at < out.n) {
                out.tid[at] = t;
                out.span[at] = in.span[i];
                out.parent[at] = in.parent[i];
                out.first[at] = in.first[i];
                out.last[at] = in.last[i];
                out.svc[at] = in.svc[i];
                out.fl[at] = in.fl[i];
            }
        }
    }
}

size_t al256(size_t b) { return (b + 255) / 256 * 256; }

// seven columns of n entries in one block, each 256-B aligned; with_off: off[4097] behind them
struct Block {
    static size_t col8(uint64_t n) { return al256((size_t)n * 8); }
    static size_t col4(uint64_t n) { return al256((size_t)n * 4); }
    static size_t cols_bytes(uint64_t n) { return 5 * col8(n) + 2 * col4(n); }
    static SpCols view(void* block, uint64_t n, bool with_off) {
        uint8_t* p = (uint8_t*)block;
        const size_t a8 = col8(n), a4 = col4(n);
        return SpCols{(unsigned long long*)p, (unsigned long long*)(p + a8), (unsigned long long*)(p + 2 * a8),
                      (long long*)(p + 3 * a8), (long long*)(p + 4 * a8), (uint32_t*)(p + 5 * a8), (uint32_t*)(p + 5 * a8 + a4),
                      with_off ? (uint32_t*)(p + 5 * a8 + 2 * a4) : nullptr, (unsigned long long)n};
    }
};

struct Segment {
    void* block = nullptr;
    size_t bytes = 0;
    uint64_t n = 0;
    std::vector<uint32_t> off;  // kSpBins + 1

    static size_t bytes_for(uint64_t n) { return Block::cols_bytes(n) + al256((kSpBins + 1) * 4); }
    SpCols cols() const { return Block::view(block, n, true); }
};

}  // namespace
}  // namespace zk

using namespace zk;

struct zk_sp {
    int device = 0;
    hipStream_t stream = nullptr, own = nullptr;
    bool timing = false;
    std::vector<Segment> segs;
    uint64_t entries = 0;
    void* obs = nullptr;     // the observe's counts and cursors (kObsBytes)
    void* stage = nullptr;   // the seven columns of a host batch
    void* mplan = nullptr;   // a merge's bases, per old segment
    void* q = nullptr;       // the lookups' block (kQBytes)
    void* rows = nullptr;    // the write pass's rows, seven columns
    void* sum_heads = nullptr;  // the summaries' heads (ZK_SP_MAX_IDS of them)
    void* ents = nullptr;       // the summaries' entries at their rows' bases: first, last [8 B], service [4 B]
    void* tr_heads = nullptr;   // the merged traces' heads (ZK_SP_MAX_IDS of them)
    void* tr_out = nullptr;     // their spans [48 B], then their services [4 B], at their rows' bases
    size_t stage_bytes = 0, mplan_bytes = 0, rows_bytes = 0, ents_bytes = 0, tr_bytes = 0;
    std::vector<uint8_t> tr_host;
    std::vector<uint32_t> sum_counts_host, sum_list_host;
    std::vector<uint8_t> ents_host;
    std::vector<uint32_t> counts_host, cursor_host, off_host;  // (queued copies read the last two: they change only behind a synchronisation)
    std::vector<uint32_t> mplan_host, moff_host;
    std::vector<uint64_t> ids_host, base_host;
    std::vector<SpCols> segs_host;
    std::vector<uint8_t> rows_host;
    hipEvent_t oev[4] = {};  // around the passes of the last observe (zk_sp_observe_ms)
    hipEvent_t qev[2] = {};  // around the last lookup (zk_sp_query_ms)
    hipEvent_t xev[4] = {};  // around the passes of the last expiry (zk_sp_expire_ms)
    bool otimed = false, qtimed = false, xtimed = false;
    uint64_t expire_chunk = 0;  // entries per range of buckets at most
    void* xplan = nullptr;      // the expiry's block (kXBytes)
    std::vector<SpXSeg> xsegs_host;
    std::vector<SpItem> xitems_host;
    std::vector<uint32_t> xsurv_host, xcursor_host, xoff_host;
    std::vector<unsigned long long> xpin_ids_host, xpin_cuts_host;
    std::string err;
};

namespace {

zk_status sfail(zk_sp* h, zk_status s, const std::string& m) {
    if (h) h->err = m;
    return s;
}

#define SP_HIP(h, call)                                                                            \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess) return sfail(h, is_refusal(_e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP,       \
                                           std::string(#call) + ": " + launch_error_str(_e));      \
    } while (0)

// a fresh block of `need` bytes; a refused allocation is ZK_ERR_CAPACITY
zk_status alloc(zk_sp* h, void** p, size_t need, const char* what) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, need ? need : 8);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (e != hipErrorOutOfMemory) return sfail(h, ZK_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        return sfail(h, ZK_ERR_CAPACITY, std::string("no device memory for ") + what);
    }
    *p = q;
    return ZK_OK;
}

// at least `need` bytes behind *p: a larger block first, then the old one freed (its content is not
// kept); a refused allocation leaves *p as it was
zk_status grow(zk_sp* h, void** p, size_t* have, size_t need, const char* what) {
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

void free_segments(zk_sp* h) {
    if (!h->segs.empty()) (void)hipStreamSynchronize(h->stream);
    for (Segment& g : h->segs)
        if (g.block) (void)hipFree(g.block);
    h->segs.clear();
}

// All segments into one: each bucket's slices concatenated in segment order. Anything refused leaves
// the store as it was. Synchronises.
zk_status merge_all(zk_sp* h) {
    const uint32_t G = (uint32_t)h->segs.size();
    if (G < 2) return ZK_OK;
    Segment m;
    m.n = h->entries;
    m.off.assign(kSpBins + 1, 0);
    std::vector<uint64_t> wide(kSpBins + 1, 0);
    for (uint32_t b = 0; b < kSpBins; ++b) {
        uint64_t c = 0;
        for (const Segment& sg : h->segs) c += sg.off[b + 1] - sg.off[b];
        wide[b + 1] = wide[b] + c;
    }
    if (wide[kSpBins] != m.n || m.n > kSpMaxEntries) return sfail(h, ZK_ERR_HIP, "the segments' offsets do not add up");
    for (uint32_t b = 0; b <= kSpBins; ++b) m.off[b] = (uint32_t)wide[b];
    // per old segment: the bases of its slices in the merged segment [kSpBins]
    h->mplan_host.assign((size_t)kSpBins * G, 0);
    std::vector<uint32_t> next(m.off.begin(), m.off.begin() + kSpBins);
    for (uint32_t g = 0; g < G; ++g) {
        const Segment& sg = h->segs[g];
        for (uint32_t b = 0; b < kSpBins; ++b) {
            h->mplan_host[(size_t)kSpBins * g + b] = next[b];
            next[b] += sg.off[b + 1] - sg.off[b];
        }
    }
    zk_status st = grow(h, &h->mplan, &h->mplan_bytes, (size_t)kSpBins * G * 4, "a merge's bases");
    if (st != ZK_OK) return st;
    m.bytes = Segment::bytes_for(m.n);
    if ((st = alloc(h, &m.block, m.bytes, "the merged segment (48 B per entry)")) != ZK_OK) return st;
    const SpCols dst = m.cols();
    h->moff_host = m.off;
    hipError_t e = hipMemcpyAsync(h->mplan, h->mplan_host.data(), (size_t)kSpBins * G * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dst.off, h->moff_host.data(), (kSpBins + 1) * 4, hipMemcpyHostToDevice, h->stream);
    for (uint32_t g = 0; g < G && e == hipSuccess; ++g) {
        const Segment& sg = h->segs[g];
        e = launch_checked("k_sp_merge", k_sp_merge, dim3(sp_grid(sg.n)), dim3(kSpWG), 0, h->stream, sg.cols(),
                           (const uint32_t*)h->mplan + (size_t)kSpBins * g, dst);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(m.block);
        return sfail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("merging the segments: ") + launch_error_str(e));
    }
    free_segments(h);
    h->segs.push_back(std::move(m));
    return ZK_OK;
}

// The lookups' count pass: the ids into the block (from the host or the device), counts[n] back.
// *parts = the grid's z of both passes. Synchronises; needs a store with segments.
zk_status find_count(zk_sp* h, const uint64_t* ids, uint32_t n, uint32_t flags, uint32_t* counts, uint32_t* parts) {
    zk_status st;
    if (!h->q && (st = alloc(h, &h->q, kQBytes, "the lookups' block")) != ZK_OK) return st;
    uint8_t* qb = (uint8_t*)h->q;
    unsigned long long* d_ids = (unsigned long long*)(qb + kQIdsAt);
    uint32_t* d_counts = (uint32_t*)(qb + kQCountsAt);
    const uint32_t G = (uint32_t)h->segs.size();
    // the host needs the ids too: it sizes the grid by the longest asked slice
    h->ids_host.resize(n);
    if (flags & ZK_BATCH_DEVICE_PTRS) {
        SP_HIP(h, hipMemcpyAsync(d_ids, ids, (size_t)n * 8, hipMemcpyDeviceToDevice, h->stream));
        SP_HIP(h, hipMemcpyAsync(h->ids_host.data(), ids, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
        SP_HIP(h, hipStreamSynchronize(h->stream));
    } else {
        memcpy(h->ids_host.data(), ids, (size_t)n * 8);
        SP_HIP(h, hipMemcpyAsync(d_ids, h->ids_host.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    }
    uint64_t longest = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t b = sp_bucket(h->ids_host[i]);
        for (const Segment& sg : h->segs) longest = std::max<uint64_t>(longest, sg.off[b + 1] - sg.off[b]);
    }
    uint64_t z = std::min<uint64_t>(kSpMaxParts, std::max<uint64_t>(1, (longest + kSpPart - 1) / kSpPart));
    z = std::max<uint64_t>(1, std::min<uint64_t>(z, kSpMaxFindGrid / ((uint64_t)n * G)));
    *parts = (uint32_t)z;
    h->segs_host.clear();
    for (const Segment& sg : h->segs) h->segs_host.push_back(sg.cols());
    SP_HIP(h, hipMemcpyAsync(qb + kQSegsAt, h->segs_host.data(), G * sizeof(SpCols), hipMemcpyHostToDevice, h->stream));
    SP_HIP(h, hipMemsetAsync(d_counts, 0, (size_t)n * 4, h->stream));
    for (hipEvent_t& e : h->qev)
        if (h->timing && !e) SP_HIP(h, hipEventCreate(&e));
    h->qtimed = false;
    if (h->timing) SP_HIP(h, hipEventRecord(h->qev[0], h->stream));
    SP_HIP(h, launch_checked("k_sp_find_count", k_sp_find_count, dim3(n, G, *parts), dim3(kSpWG), 0, h->stream,
                             (const SpCols*)(qb + kQSegsAt), (const unsigned long long*)d_ids, d_counts));
    SP_HIP(h, hipMemcpyAsync(counts, d_counts, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    SP_HIP(h, hipStreamSynchronize(h->stream));
    return ZK_OK;
}

zk_status check_ask(zk_sp* h, const uint64_t* ids, uint32_t n, uint32_t flags) {
    if (flags & ~ZK_BATCH_DEVICE_PTRS) return sfail(h, ZK_ERR_INVALID_ARG, "unknown flag");
    if (n > ZK_SP_MAX_IDS) return sfail(h, ZK_ERR_INVALID_ARG, "more than ZK_SP_MAX_IDS ids");
    if (n && !ids) return sfail(h, ZK_ERR_INVALID_ARG, "null argument");
    return ZK_OK;
}

// The passes zk_sp_summaries and zk_sp_traces share: the count pass, the rows' bases, the two work lists (the
// traces a wave takes, then the ones a workgroup takes; big_rows = the LDS rows of the workgroups' launch,
// sized by the longest trace among them of at most max_rows rows), and the write pass into the handle's
// staging, queued. total == 0: nothing was found and nothing is queued. counts = h->sum_counts_host.
struct SpStaged {
    uint64_t total = 0;
    uint32_t n_wave = 0, n_group = 0, big_rows = kSpSumWave;
    SpCols dev = {};
};

zk_status stage_traces(zk_sp* h, const uint64_t* ids, uint32_t n, uint32_t flags, uint32_t max_rows, SpStaged* s) {
    zk_status st;
    uint32_t parts = 1;
    h->sum_counts_host.resize(n);
    const uint32_t* counts = h->sum_counts_host.data();
    if ((st = find_count(h, ids, n, flags, h->sum_counts_host.data(), &parts)) != ZK_OK) return st;
    h->base_host.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        h->base_host[i] = s->total;
        s->total += counts[i];
    }
    if (s->total == 0) return ZK_OK;
    h->sum_list_host.clear();
    for (uint32_t i = 0; i < n; ++i)
        if (counts[i] && counts[i] <= (uint32_t)kSpSumWave) h->sum_list_host.push_back(i);
    s->n_wave = (uint32_t)h->sum_list_host.size();
    for (uint32_t i = 0; i < n; ++i)
        if (counts[i] > (uint32_t)kSpSumWave) {
            h->sum_list_host.push_back(i);
            if (counts[i] <= max_rows)
                while (s->big_rows < counts[i]) s->big_rows <<= 1;
        }
    s->n_group = (uint32_t)h->sum_list_host.size() - s->n_wave;
    if ((st = grow(h, &h->rows, &h->rows_bytes, Block::cols_bytes(s->total), "the gathered rows (48 B each)")) != ZK_OK) return st;
    uint8_t* qb = (uint8_t*)h->q;
    s->dev = Block::view(h->rows, s->total, false);
    SP_HIP(h, hipMemcpyAsync(qb + kQBaseAt, h->base_host.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    SP_HIP(h, hipMemcpyAsync(qb + kQListAt, h->sum_list_host.data(), h->sum_list_host.size() * 4, hipMemcpyHostToDevice, h->stream));
    SP_HIP(h, hipMemsetAsync(qb + kQCursorAt, 0, (size_t)n * 4, h->stream));
    SP_HIP(h, launch_checked("k_sp_find_write", k_sp_find_write, dim3(n, (uint32_t)h->segs.size(), parts), dim3(kSpWG), 0, h->stream,
                             (const SpCols*)(qb + kQSegsAt), (const unsigned long long*)(qb + kQIdsAt),
                             (const uint32_t*)(qb + kQCountsAt), (uint32_t*)(qb + kQCursorAt),
                             (const unsigned long long*)(qb + kQBaseAt), s->dev));
    return ZK_OK;
}

// a range of buckets [b0, b1) and its entries over all segments
struct SpRange {
    uint32_t b0, b1;
    uint64_t entries;
};

// zk_sp_expire behind its argument checks (a store with segments; the pins ascending by id, their cuts
// as keys, in the handle's vectors). Per range of buckets the end table's three passes, then the one
// synchronisation that sizes the rest, then the segments sorted into untouched (no entry goes: not read
// again), gone (every entry goes: freed) and mixed (their survivors rewritten into ONE new segment, which
// takes the place of the first of them). Nothing is freed and no bookkeeping changes before the new
// segment is complete; anything refused leaves the store as it was. The table and the marks are scratch
// of this call.
zk_status expire(zk_sp* h, unsigned long long cut, uint64_t* removed_out, void** table, void** marks) {
    const uint32_t G = (uint32_t)h->segs.size(), P = (uint32_t)h->xpin_ids_host.size();
    // the ranges: consecutive buckets while their entries over all segments stay inside the chunk
    std::vector<SpRange> ranges;
    uint64_t most = 0;
    for (uint32_t b = 0; b < kSpBins; ++b) {
        uint64_t c = 0;
        for (const Segment& sg : h->segs) c += sg.off[b + 1] - sg.off[b];
        if (ranges.empty() || (ranges.back().entries && ranges.back().entries + c > h->expire_chunk))
            ranges.push_back(SpRange{b, b + 1, c});
        else {
            ranges.back().b1 = b + 1;
            ranges.back().entries += c;
        }
        most = std::max(most, ranges.back().entries);
    }
    const auto slots_for = [](uint64_t entries) {
        uint64_t s = kSpEndMinSlots;
        while (s < 2 * entries) s <<= 1;
        return s;
    };
    zk_status st;
    if (!h->xplan && (st = alloc(h, &h->xplan, kXBytes, "the expiry's block")) != ZK_OK) return st;
    if ((st = alloc(h, table, (size_t)(slots_for(most) + 1) * 16, "the expiry's end table (16 B per slot)")) != ZK_OK) return st;
    h->xsegs_host.clear();
    uint64_t words = 0;
    for (const Segment& sg : h->segs) {
        h->xsegs_host.push_back(SpXSeg{sg.cols(), (unsigned long long)words});
        words += (sg.n + 63) / 64;
    }
    if ((st = alloc(h, marks, (size_t)words * 8, "the expiry's marks (1 bit per entry)")) != ZK_OK) return st;
    uint8_t* xp = (uint8_t*)h->xplan;
    const SpXSeg* segs = (const SpXSeg*)(xp + kXSegsAt);
    uint32_t* surv = (uint32_t*)(xp + kXSurvAt);
    uint32_t* cursor = (uint32_t*)(xp + kXCursorAt);
    unsigned long long* full = (unsigned long long*)(xp + kXFullAt);
    const unsigned long long* pin_ids = (const unsigned long long*)(xp + kXPinIdsAt);
    const unsigned long long* pin_cuts = (const unsigned long long*)(xp + kXPinCutsAt);
    uint32_t* verdict = (uint32_t*)(xp + kXVerdictAt);
    const SpItem* items = (const SpItem*)(xp + kXItemsAt);
    unsigned long long* tab = (unsigned long long*)*table;
    unsigned long long* mk = (unsigned long long*)*marks;
    const bool timing = h->timing;
    for (hipEvent_t& e : h->xev)
        if (timing && !e) SP_HIP(h, hipEventCreate(&e));
    SP_HIP(h, hipMemcpyAsync(xp + kXSegsAt, h->xsegs_host.data(), G * sizeof(SpXSeg), hipMemcpyHostToDevice, h->stream));
    SP_HIP(h, hipMemsetAsync(surv, 0, (size_t)G * kSpBins * 4, h->stream));
    SP_HIP(h, hipMemsetAsync(full, 0, 8, h->stream));
    SP_HIP(h, hipMemsetAsync(mk, 0, (size_t)words * 8, h->stream));
    if (P) {
        SP_HIP(h, hipMemcpyAsync(xp + kXPinIdsAt, h->xpin_ids_host.data(), (size_t)P * 8, hipMemcpyHostToDevice, h->stream));
        SP_HIP(h, hipMemcpyAsync(xp + kXPinCutsAt, h->xpin_cuts_host.data(), (size_t)P * 8, hipMemcpyHostToDevice, h->stream));
        SP_HIP(h, hipMemsetAsync(verdict, 0, (size_t)P * 4, h->stream));
    }
    if (timing) SP_HIP(h, hipEventRecord(h->xev[0], h->stream));
    for (const SpRange& r : ranges) {
        if (!r.entries) continue;
        const uint64_t slots = slots_for(r.entries);
        uint64_t longest = 0;  // the range's longest slice in one segment sizes the grid's x
        for (const Segment& sg : h->segs) longest = std::max<uint64_t>(longest, sg.off[r.b1] - sg.off[r.b0]);
        const dim3 grid(sp_grid(longest, kSpEndGrid), G);
        SP_HIP(h, hipMemsetAsync(tab, 0, (size_t)(slots + 1) * 16, h->stream));
        SP_HIP(h, launch_checked("k_sp_end_fold", k_sp_end_fold, grid, dim3(kSpWG), 0, h->stream, segs, r.b0, r.b1, tab,
                                 (unsigned long long)slots, full));
        if (P)
            SP_HIP(h, launch_checked("k_sp_end_pins", k_sp_end_pins, dim3(sp_grid(P)), dim3(kSpWG), 0, h->stream, pin_ids, pin_cuts, P,
                                     r.b0, r.b1, tab, (unsigned long long)slots, verdict));
        SP_HIP(h, launch_checked("k_sp_end_mark", k_sp_end_mark, grid, dim3(kSpWG), 0, h->stream, segs, r.b0, r.b1,
                                 (const unsigned long long*)tab, (unsigned long long)slots, cut, pin_ids, (const uint32_t*)verdict, P, mk,
                                 surv));
    }
    if (timing) SP_HIP(h, hipEventRecord(h->xev[1], h->stream));
    h->xsurv_host.resize((size_t)G * kSpBins);
    unsigned long long ran_full = 0;
    SP_HIP(h, hipMemcpyAsync(h->xsurv_host.data(), surv, (size_t)G * kSpBins * 4, hipMemcpyDeviceToHost, h->stream));
    SP_HIP(h, hipMemcpyAsync(&ran_full, full, 8, hipMemcpyDeviceToHost, h->stream));
    SP_HIP(h, hipStreamSynchronize(h->stream));  // the sizing synchronisation
    if (ran_full) return sfail(h, ZK_ERR_HIP, "the expiry's end table ran full (the sizing rule was broken)");
    std::vector<uint64_t> keep(G, 0);
    std::vector<uint32_t> mixed;
    uint64_t removed = 0;
    for (uint32_t g = 0; g < G; ++g) {
        const Segment& sg = h->segs[g];
        for (uint32_t b = 0; b < kSpBins; ++b) {
            const uint64_t c = h->xsurv_host[(size_t)g * kSpBins + b];
            if (c > (uint64_t)(sg.off[b + 1] - sg.off[b])) return sfail(h, ZK_ERR_HIP, "the expiry counted more survivors than a slice holds");
            keep[g] += c;
        }
        removed += sg.n - keep[g];
        if (keep[g] != 0 && keep[g] != sg.n) mixed.push_back(g);
    }
    if (removed == 0) {  // nothing goes: nothing is rewritten, reallocated or freed
        if (timing) SP_HIP(h, hipEventRecord(h->xev[2], h->stream));
        if (timing) SP_HIP(h, hipEventRecord(h->xev[3], h->stream));
        h->xtimed = timing;
        return ZK_OK;
    }
    Segment m;
    uint64_t chunk = kSpScatterPerWG;
    if (!mixed.empty()) {
        m.off.assign(kSpBins + 1, 0);
        for (uint32_t b = 0; b < kSpBins; ++b) {
            uint64_t c = 0;
            for (uint32_t g : mixed) c += h->xsurv_host[(size_t)g * kSpBins + b];
            m.off[b + 1] = (uint32_t)(m.off[b] + c);  // (below the store's entries, which fit)
        }
        m.n = m.off[kSpBins];
        m.bytes = Segment::bytes_for(m.n);
        const auto items_at = [&](uint64_t c) {
            uint64_t w = 0;
            for (uint32_t g : mixed) w += (h->segs[g].n + c - 1) / c;
            return w;
        };
        while (items_at(chunk) > kSpMaxItems + mixed.size()) chunk *= 2;
        h->xitems_host.clear();
        for (uint32_t g : mixed)
            for (uint64_t c = 0; c * chunk < h->segs[g].n; ++c) h->xitems_host.push_back(SpItem{g, (uint32_t)c});
        if ((st = alloc(h, &m.block, m.bytes, "the survivors' segment (48 B per entry)")) != ZK_OK) return st;
        h->xcursor_host.assign(m.off.begin(), m.off.begin() + kSpBins);
        h->xoff_host = m.off;
    }
    hipError_t e = hipSuccess;
    if (!mixed.empty()) {
        const SpCols dst = m.cols();
        e = hipMemcpyAsync(xp + kXItemsAt, h->xitems_host.data(), h->xitems_host.size() * sizeof(SpItem), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cursor, h->xcursor_host.data(), kSpBins * 4, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dst.off, h->xoff_host.data(), (kSpBins + 1) * 4, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess && timing) e = hipEventRecord(h->xev[2], h->stream);
        if (e == hipSuccess)
            e = launch_checked("k_sp_expire_rewrite", k_sp_expire_rewrite, dim3((uint32_t)h->xitems_host.size()), dim3(kSpWG), 0,
                               h->stream, segs, items, (unsigned long long)chunk, (const unsigned long long*)mk, cursor, dst);
    } else if (timing) {
        e = hipEventRecord(h->xev[2], h->stream);
    }
    if (e == hipSuccess && timing) e = hipEventRecord(h->xev[3], h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        if (m.block) (void)hipFree(m.block);
        return sfail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("rewriting the survivors: ") + launch_error_str(e));
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

zk_status zk_sp_create(const zk_sp_config* cfg, zk_sp** out) {
    ZK_GUARD_BEGIN
    if (!cfg || !out) return ZK_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || cfg->device < 0 || cfg->device >= ndev) return ZK_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return ZK_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return ZK_ERR_NO_DEVICE;
    if (hipSetDevice(cfg->device) != hipSuccess) return ZK_ERR_HIP;
    zk_sp* h = new zk_sp();
    h->device = cfg->device;
    h->timing = cfg->timing != 0;
    h->expire_chunk = cfg->expire_chunk ? cfg->expire_chunk : kSpExpireChunk;
    if (cfg->stream) {
        h->stream = (hipStream_t)cfg->stream;
    } else if (hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return ZK_ERR_HIP;
    } else {
        h->stream = h->own;
    }
    *out = h;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_sp_destroy(zk_sp* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_segments(h);
    for (void* p : {h->obs, h->stage, h->mplan, h->q, h->rows, h->xplan, h->sum_heads, h->ents, h->tr_heads, h->tr_out})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : h->oev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->qev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->xev)
        if (e) (void)hipEventDestroy(e);
    if (h->own) (void)hipStreamDestroy(h->own);
    delete h;
    return ZK_OK;
    ZK_GUARD_END
}

const char* zk_sp_last_error(const zk_sp* h) { return h ? h->err.c_str() : "null handle"; }

zk_status zk_sp_observe(zk_sp* h, const zk_span_cols* in, uint32_t flags) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!in) return sfail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (flags & ~(ZK_BATCH_DEVICE_PTRS | ZK_BATCH_TRACE_CLUSTERED)) return sfail(h, ZK_ERR_INVALID_ARG, "unknown batch flag");
    const uint64_t n = in->n;
    if (n >= (1ull << 32)) return sfail(h, ZK_ERR_UNSUPPORTED, "2^32 records or more in one batch");
    if (n == 0) return ZK_OK;
    if (!in->trace_id || !in->span_id || !in->parent_id || !in->first_ts || !in->last_ts || !in->service_id || !in->flags)
        return sfail(h, ZK_ERR_INVALID_ARG, "null column");
    if (h->entries + n > kSpMaxEntries) return sfail(h, ZK_ERR_CAPACITY, "more than 2^32 - 1 entries in one store");
    SP_HIP(h, hipSetDevice(h->device));
    zk_status st;
    if (!h->obs && (st = alloc(h, &h->obs, kObsBytes, "the observe's counters")) != ZK_OK) return st;
    SpCols src{(unsigned long long*)in->trace_id, (unsigned long long*)in->span_id, (unsigned long long*)in->parent_id,
               (long long*)in->first_ts, (long long*)in->last_ts, (uint32_t*)in->service_id, (uint32_t*)in->flags, nullptr,
               (unsigned long long)n};
    if (!(flags & ZK_BATCH_DEVICE_PTRS)) {
        // a host batch: the seven columns staged (each 256-B aligned)
        if ((st = grow(h, &h->stage, &h->stage_bytes, Block::cols_bytes(n), "staging a host batch (48 B per record)")) != ZK_OK)
            return st;
        const SpCols s = Block::view(h->stage, n, false);
        SP_HIP(h, hipMemcpyAsync(s.tid, in->trace_id, n * 8, hipMemcpyHostToDevice, h->stream));
        SP_HIP(h, hipMemcpyAsync(s.span, in->span_id, n * 8, hipMemcpyHostToDevice, h->stream));
        SP_HIP(h, hipMemcpyAsync(s.parent, in->parent_id, n * 8, hipMemcpyHostToDevice, h->stream));
        SP_HIP(h, hipMemcpyAsync(s.first, in->first_ts, n * 8, hipMemcpyHostToDevice, h->stream));
        SP_HIP(h, hipMemcpyAsync(s.last, in->last_ts, n * 8, hipMemcpyHostToDevice, h->stream));
        SP_HIP(h, hipMemcpyAsync(s.svc, in->service_id, n * 4, hipMemcpyHostToDevice, h->stream));
        SP_HIP(h, hipMemcpyAsync(s.fl, in->flags, n * 4, hipMemcpyHostToDevice, h->stream));
        src = s;
    }
    uint32_t* counts = (uint32_t*)h->obs;
    uint32_t* cursor = (uint32_t*)((uint8_t*)h->obs + kObsCursorAt);
    const bool timing = h->timing;
    for (hipEvent_t& e : h->oev)
        if (timing && !e) SP_HIP(h, hipEventCreate(&e));
    h->otimed = false;
    SP_HIP(h, hipMemsetAsync(counts, 0, kSpBins * 4, h->stream));
    if (timing) SP_HIP(h, hipEventRecord(h->oev[0], h->stream));
    SP_HIP(h, launch_checked("k_sp_count", k_sp_count, dim3(sp_grid((n + kSpCntItems - 1) / kSpCntItems, kSpHistGrid)), dim3(kSpWG), 0,
                             h->stream, (const unsigned long long*)src.tid, (unsigned long long)n, counts));
    if (timing) SP_HIP(h, hipEventRecord(h->oev[1], h->stream));
    h->counts_host.resize(kSpBins);
    SP_HIP(h, hipMemcpyAsync(h->counts_host.data(), counts, kSpBins * 4, hipMemcpyDeviceToHost, h->stream));
    SP_HIP(h, hipStreamSynchronize(h->stream));  // the call's one synchronisation (also: the staging copies are done)
    Segment g;
    g.off.assign(kSpBins + 1, 0);
    uint64_t total = 0;
    for (uint32_t b = 0; b < kSpBins; ++b) {
        total += h->counts_host[b];
        if (total > n) return sfail(h, ZK_ERR_HIP, "the bucket counts exceed the batch");
        g.off[b + 1] = (uint32_t)total;
    }
    if (total != n) return sfail(h, ZK_ERR_HIP, "the bucket counts do not add up to the batch");
    g.n = n;
    if (h->segs.size() >= ZK_SP_MAX_SEGMENTS && (st = merge_all(h)) != ZK_OK) return st;
    g.bytes = Segment::bytes_for(g.n);
    if ((st = alloc(h, &g.block, g.bytes, "a segment (48 B per entry)")) != ZK_OK) return st;
    const SpCols dst = g.cols();
    h->cursor_host.assign(g.off.begin(), g.off.begin() + kSpBins);
    h->off_host = g.off;
    uint32_t grid = (uint32_t)((n + kSpScatterPerWG - 1) / kSpScatterPerWG);
    grid = grid < 1 ? 1 : grid > kSpMaxGrid ? kSpMaxGrid : grid;
    const uint64_t chunk = ((n + grid - 1) / grid + kSpWG - 1) / kSpWG * kSpWG;
    hipError_t e = hipMemcpyAsync(cursor, h->cursor_host.data(), kSpBins * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dst.off, h->off_host.data(), (kSpBins + 1) * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && timing) e = hipEventRecord(h->oev[2], h->stream);
    if (e == hipSuccess)
        e = launch_checked("k_sp_scatter", k_sp_scatter, dim3(grid), dim3(kSpWG), 0, h->stream, src, (unsigned long long)chunk, cursor, dst);
    if (e == hipSuccess && timing) e = hipEventRecord(h->oev[3], h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(g.block);
        return sfail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("k_sp_scatter: ") + launch_error_str(e));
    }
    h->entries += g.n;
    h->segs.push_back(std::move(g));
    h->otimed = timing;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_sp_observe_ms(zk_sp* h, double out[3]) {
    ZK_GUARD_BEGIN
    if (!h || !out) return ZK_ERR_INVALID_ARG;
    if (!h->otimed) return sfail(h, ZK_ERR_INVALID_ARG, "no timed observe has added a segment (zk_sp_config.timing)");
    SP_HIP(h, hipSetDevice(h->device));
    SP_HIP(h, hipEventSynchronize(h->oev[3]));
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        SP_HIP(h, hipEventElapsedTime(&ms, h->oev[k], h->oev[k + 1]));
        out[k] = ms;
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_sp_reset(zk_sp* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (h->segs.empty()) return ZK_OK;
    SP_HIP(h, hipSetDevice(h->device));
    free_segments(h);
    h->entries = 0;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_sp_compact(zk_sp* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (h->segs.size() < 2) return ZK_OK;
    SP_HIP(h, hipSetDevice(h->device));
    return merge_all(h);
    ZK_GUARD_END
}

zk_status zk_sp_expire(zk_sp* h, int64_t min_end, const uint64_t* pin_ids, const int64_t* pin_min_end, uint32_t n_pins,
                       uint64_t* removed) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!removed) return sfail(h, ZK_ERR_INVALID_ARG, "null argument");
    *removed = 0;
    if (n_pins > ZK_SP_MAX_PINS) return sfail(h, ZK_ERR_INVALID_ARG, "more than ZK_SP_MAX_PINS pins");
    if (n_pins && (!pin_ids || !pin_min_end)) return sfail(h, ZK_ERR_INVALID_ARG, "null argument");
    // the pins ascending by id (the mark pass searches them), their cuts as keys
    static thread_local std::vector<uint32_t> order;
    order.resize(n_pins);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [pin_ids](uint32_t x, uint32_t y) { return pin_ids[x] < pin_ids[y]; });
    for (uint32_t i = 1; i < n_pins; ++i)
        if (pin_ids[order[i - 1]] == pin_ids[order[i]]) return sfail(h, ZK_ERR_INVALID_ARG, "a trace id is pinned twice");
    h->xtimed = false;
    if (h->segs.empty()) return ZK_OK;
    if (min_end == INT64_MIN && n_pins == 0) return ZK_OK;  // every end is >= INT64_MIN
    h->xpin_ids_host.resize(n_pins);
    h->xpin_cuts_host.resize(n_pins);
    for (uint32_t i = 0; i < n_pins; ++i) {
        h->xpin_ids_host[i] = pin_ids[order[i]];
        h->xpin_cuts_host[i] = (unsigned long long)pin_min_end[order[i]] ^ kSpSign;
    }
    SP_HIP(h, hipSetDevice(h->device));
    void *table = nullptr, *marks = nullptr;
    const zk_status st = expire(h, (unsigned long long)min_end ^ kSpSign, removed, &table, &marks);
    if (table || marks) (void)hipStreamSynchronize(h->stream);
    if (table) (void)hipFree(table);
    if (marks) (void)hipFree(marks);
    return st;
    ZK_GUARD_END
}

zk_status zk_sp_expire_ms(zk_sp* h, double out[3]) {
    ZK_GUARD_BEGIN
    if (!h || !out) return ZK_ERR_INVALID_ARG;
    if (!h->xtimed) return sfail(h, ZK_ERR_INVALID_ARG, "no timed expiry has run a pass (zk_sp_config.timing)");
    SP_HIP(h, hipSetDevice(h->device));
    SP_HIP(h, hipEventSynchronize(h->xev[3]));
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        SP_HIP(h, hipEventElapsedTime(&ms, h->xev[k], h->xev[k + 1]));
        out[k] = ms;
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_sp_info(zk_sp* h, uint64_t* entries, uint64_t* segments, uint64_t* bytes) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!h->segs.empty()) {
        SP_HIP(h, hipSetDevice(h->device));
        SP_HIP(h, hipStreamSynchronize(h->stream));
    }
    uint64_t b = 0;
    for (const Segment& g : h->segs) b += g.bytes;
    if (entries) *entries = h->entries;
    if (segments) *segments = h->segs.size();
    if (bytes) *bytes = b;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_sp_exist(zk_sp* h, const uint64_t* ids, uint32_t n, uint32_t flags, uint8_t* found) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    zk_status st = check_ask(h, ids, n, flags);
    if (st != ZK_OK) return st;
    if (n == 0) return ZK_OK;
    if (!found) return sfail(h, ZK_ERR_INVALID_ARG, "null argument");
    memset(found, 0, n);
    if (h->segs.empty()) return ZK_OK;
    SP_HIP(h, hipSetDevice(h->device));
    static thread_local std::vector<uint32_t> counts;
    counts.resize(n);
    uint32_t parts = 1;
    if ((st = find_count(h, ids, n, flags, counts.data(), &parts)) != ZK_OK) return st;
    if (h->timing) {
        SP_HIP(h, hipEventRecord(h->qev[1], h->stream));
        SP_HIP(h, hipEventSynchronize(h->qev[1]));
        h->qtimed = true;
    }
    for (uint32_t i = 0; i < n; ++i) found[i] = counts[i] ? 1 : 0;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_sp_gather(zk_sp* h, const uint64_t* ids, uint32_t n, uint32_t flags, uint32_t* counts, zk_sp_rows* out, uint64_t cap,
                       uint64_t* n_out) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!n_out) return sfail(h, ZK_ERR_INVALID_ARG, "null argument");
    zk_status st = check_ask(h, ids, n, flags);
    if (st != ZK_OK) return st;
    if (n && !counts) return sfail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (cap && (!out || !out->trace_id || !out->span_id || !out->parent_id || !out->first_ts || !out->last_ts ||
                !out->service_id || !out->flags))
        return sfail(h, ZK_ERR_INVALID_ARG, "null output column");
    *n_out = 0;
    if (n == 0) return ZK_OK;
    memset(counts, 0, (size_t)n * 4);
    if (h->segs.empty()) return ZK_OK;
    SP_HIP(h, hipSetDevice(h->device));
    uint32_t parts = 1;
    if ((st = find_count(h, ids, n, flags, counts, &parts)) != ZK_OK) return st;
    h->base_host.resize(n);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        h->base_host[i] = total;
        total += counts[i];
    }
    *n_out = total;
    if (total > cap) return sfail(h, ZK_ERR_CAPACITY, "the output columns hold fewer rows than the asked traces have");
    if (total == 0) return ZK_OK;
    if ((st = grow(h, &h->rows, &h->rows_bytes, Block::cols_bytes(total), "the gathered rows (48 B each)")) != ZK_OK) return st;
    h->rows_host.resize(Block::cols_bytes(total));
    uint8_t* qb = (uint8_t*)h->q;
    const SpCols dev = Block::view(h->rows, total, false);
    const uint32_t G = (uint32_t)h->segs.size();
    SP_HIP(h, hipMemcpyAsync(qb + kQBaseAt, h->base_host.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    SP_HIP(h, hipMemsetAsync(qb + kQCursorAt, 0, (size_t)n * 4, h->stream));
    SP_HIP(h, launch_checked("k_sp_find_write", k_sp_find_write, dim3(n, G, parts), dim3(kSpWG), 0, h->stream,
                             (const SpCols*)(qb + kQSegsAt), (const unsigned long long*)(qb + kQIdsAt),
                             (const uint32_t*)(qb + kQCountsAt), (uint32_t*)(qb + kQCursorAt),
                             (const unsigned long long*)(qb + kQBaseAt), dev));
    // the seven columns lie back to back, each 256-B aligned, in the device block and in the host's copy
    SP_HIP(h, hipMemcpyAsync(h->rows_host.data(), h->rows, Block::cols_bytes(total), hipMemcpyDeviceToHost, h->stream));
    if (h->timing) SP_HIP(h, hipEventRecord(h->qev[1], h->stream));
    SP_HIP(h, hipStreamSynchronize(h->stream));
    h->qtimed = h->timing;
    // every trace's rows into CANONICAL order (the trace id is the asked one)
    const SpCols r = Block::view(h->rows_host.data(), total, false);
    static thread_local std::vector<uint64_t> perm;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t at = h->base_host[i], c = counts[i];
        if (!c) continue;
        perm.resize(c);
        std::iota(perm.begin(), perm.end(), at);
        std::sort(perm.begin(), perm.end(), [&r](uint64_t x, uint64_t y) {
            if (r.span[x] != r.span[y]) return r.span[x] < r.span[y];
            if (r.parent[x] != r.parent[y]) return r.parent[x] < r.parent[y];
            if (r.first[x] != r.first[y]) return r.first[x] < r.first[y];
            if (r.last[x] != r.last[y]) return r.last[x] < r.last[y];
            if (r.svc[x] != r.svc[y]) return r.svc[x] < r.svc[y];
            return r.fl[x] < r.fl[y];
        });
        for (uint64_t k = 0; k < c; ++k) {
            const uint64_t s = perm[k], d = at + k;
            out->trace_id[d] = r.tid[s];
            out->span_id[d] = r.span[s];
            out->parent_id[d] = r.parent[s];
            out->first_ts[d] = r.first[s];
            out->last_ts[d] = r.last[s];
            out->service_id[d] = r.svc[s];
            out->flags[d] = r.fl[s];
        }
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_sp_summaries(zk_sp* h, const uint64_t* ids, uint32_t n, uint32_t flags, zk_sp_summary* heads, zk_sp_span_ts* out,
                          uint64_t cap, uint64_t* n_out) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!n_out) return sfail(h, ZK_ERR_INVALID_ARG, "null argument");
    zk_status st = check_ask(h, ids, n, flags);
    if (st != ZK_OK) return st;
    if (n && !heads) return sfail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (cap && (!out || !out->service_id || !out->first || !out->last)) return sfail(h, ZK_ERR_INVALID_ARG, "null output column");
    *n_out = 0;
    if (n == 0) return ZK_OK;
    memset(heads, 0, (size_t)n * sizeof(zk_sp_summary));
    if (h->segs.empty()) return ZK_OK;
    SP_HIP(h, hipSetDevice(h->device));
    // the two passes of zk_sp_gather and the work lists: the rows of the asked traces into the handle's staging
    if (!h->sum_heads && (st = alloc(h, &h->sum_heads, ZK_SP_MAX_IDS * sizeof(zk_sp_summary), "the summaries' heads")) != ZK_OK) return st;
    SpStaged sg;
    if ((st = stage_traces(h, ids, n, flags, kSpSumMaxRows, &sg)) != ZK_OK) return st;
    const uint64_t total = sg.total;
    if (total == 0) return ZK_OK;
    const uint32_t* counts = h->sum_counts_host.data();
    const size_t e8 = Block::col8(total);
    if ((st = grow(h, &h->ents, &h->ents_bytes, 2 * e8 + Block::col4(total), "the summaries' entries (20 B per row)")) != ZK_OK) return st;
    uint8_t* qb = (uint8_t*)h->q;
    const SpCols dev = sg.dev;
    const uint32_t n_wave = sg.n_wave, n_group = sg.n_group, big_rows = sg.big_rows;
    zk_sp_summary* d_heads = (zk_sp_summary*)h->sum_heads;
    long long* d_first = (long long*)h->ents;
    long long* d_last = (long long*)((uint8_t*)h->ents + e8);
    uint32_t* d_svc = (uint32_t*)((uint8_t*)h->ents + 2 * e8);
    const uint32_t* d_list = (const uint32_t*)(qb + kQListAt);
    const unsigned long long* d_ids = (const unsigned long long*)(qb + kQIdsAt);
    const uint32_t* d_counts = (const uint32_t*)(qb + kQCountsAt);
    const unsigned long long* d_base = (const unsigned long long*)(qb + kQBaseAt);
    SP_HIP(h, hipMemsetAsync(d_heads, 0, (size_t)n * sizeof(zk_sp_summary), h->stream));
    SP_HIP(h, launch_checked("k_sp_summarize (a wave per trace)", k_sp_summarize<kSpSumWave, 1>, dim3(n_wave), dim3(kSpSumWave),
                             sp_sum_lds(kSpSumWave), h->stream, dev, d_list, d_ids, d_counts, d_base, (uint32_t)kSpSumWave, d_heads,
                             d_svc, d_first, d_last));
    SP_HIP(h, launch_checked("k_sp_summarize (a workgroup per trace)", k_sp_summarize<kSpWG, kSpSumItems>, dim3(n_group), dim3(kSpWG),
                             sp_sum_lds(big_rows), h->stream, dev, d_list + n_wave, d_ids, d_counts, d_base, big_rows, d_heads, d_svc,
                             d_first, d_last));
    // only the heads cross before the entries' total is known
    SP_HIP(h, hipMemcpyAsync(heads, d_heads, (size_t)n * sizeof(zk_sp_summary), hipMemcpyDeviceToHost, h->stream));
    if (h->timing) SP_HIP(h, hipEventRecord(h->qev[1], h->stream));
    SP_HIP(h, hipStreamSynchronize(h->stream));
    h->qtimed = h->timing;
    uint64_t need = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (heads[i].span_ts > counts[i]) return sfail(h, ZK_ERR_HIP, "a summary has more entries than its trace has rows");
        need += heads[i].span_ts;
    }
    *n_out = need;
    if (need > cap) return sfail(h, ZK_ERR_CAPACITY, "the output columns hold fewer entries than the asked traces have");
    if (need == 0) return ZK_OK;
    // the staged entry columns in one copy, then each trace's entries packed behind the ones before it
    const size_t bytes = 2 * e8 + (size_t)total * 4;
    h->ents_host.resize(bytes);
    SP_HIP(h, hipMemcpyAsync(h->ents_host.data(), h->ents, bytes, hipMemcpyDeviceToHost, h->stream));
    if (h->timing) SP_HIP(h, hipEventRecord(h->qev[1], h->stream));
    SP_HIP(h, hipStreamSynchronize(h->stream));
    const int64_t* s_first = (const int64_t*)h->ents_host.data();
    const int64_t* s_last = (const int64_t*)(h->ents_host.data() + e8);
    const uint32_t* s_svc = (const uint32_t*)(h->ents_host.data() + 2 * e8);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t c = heads[i].span_ts, from = h->base_host[i];
        if (!c) continue;
        memcpy(out->service_id + at, s_svc + from, c * 4);
        memcpy(out->first + at, s_first + from, c * 8);
        memcpy(out->last + at, s_last + from, c * 8);
        at += c;
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_sp_traces(zk_sp* h, const uint64_t* ids, uint32_t n, uint32_t flags, zk_sp_trace* heads, zk_sp_span* spans,
                       uint64_t cap_spans, uint32_t* services, uint64_t cap_services, uint64_t n_out[2]) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!n_out) return sfail(h, ZK_ERR_INVALID_ARG, "null argument");
    zk_status st = check_ask(h, ids, n, flags);
    if (st != ZK_OK) return st;
    if (n && !heads) return sfail(h, ZK_ERR_INVALID_ARG, "null argument");
    if ((cap_spans && !spans) || (cap_services && !services)) return sfail(h, ZK_ERR_INVALID_ARG, "null output column");
    n_out[0] = n_out[1] = 0;
    if (n == 0) return ZK_OK;
    memset(heads, 0, (size_t)n * sizeof(zk_sp_trace));
    if (h->segs.empty()) return ZK_OK;
    SP_HIP(h, hipSetDevice(h->device));
    // zk_sp_summaries' passes and work lists: the rows of the asked traces into the handle's staging
    if (!h->tr_heads && (st = alloc(h, &h->tr_heads, ZK_SP_MAX_IDS * sizeof(zk_sp_trace), "the merged traces' heads")) != ZK_OK) return st;
    SpStaged sg;
    if ((st = stage_traces(h, ids, n, flags, kSpTrMaxRows, &sg)) != ZK_OK) return st;
    const uint64_t total = sg.total;
    if (total == 0) return ZK_OK;
    const uint32_t* counts = h->sum_counts_host.data();
    const size_t span_bytes = al256((size_t)total * sizeof(zk_sp_span));
    if ((st = grow(h, &h->tr_out, &h->tr_bytes, span_bytes + Block::col4(total), "the merged spans and their services (52 B per row)")) != ZK_OK) return st;
    uint8_t* qb = (uint8_t*)h->q;
    const SpCols dev = sg.dev;
    const uint32_t n_wave = sg.n_wave, n_group = sg.n_group, big_rows = sg.big_rows;
    zk_sp_trace* d_heads = (zk_sp_trace*)h->tr_heads;
    zk_sp_span* d_spans = (zk_sp_span*)h->tr_out;
    uint32_t* d_svc = (uint32_t*)((uint8_t*)h->tr_out + span_bytes);
    const uint32_t* d_list = (const uint32_t*)(qb + kQListAt);
    const unsigned long long* d_ids = (const unsigned long long*)(qb + kQIdsAt);
    const uint32_t* d_counts = (const uint32_t*)(qb + kQCountsAt);
    const unsigned long long* d_base = (const unsigned long long*)(qb + kQBaseAt);
    SP_HIP(h, hipMemsetAsync(d_heads, 0, (size_t)n * sizeof(zk_sp_trace), h->stream));
    SP_HIP(h, launch_checked("k_sp_trace (a wave per trace)", k_sp_trace<kSpSumWave, 1>, dim3(n_wave), dim3(kSpSumWave),
                             sp_tr_lds(kSpSumWave), h->stream, dev, d_list, d_ids, d_counts, d_base, (uint32_t)kSpSumWave, d_heads,
                             d_spans, d_svc));
    SP_HIP(h, launch_checked("k_sp_trace (a workgroup per trace)", k_sp_trace<kSpWG, kSpSumItems>, dim3(n_group), dim3(kSpWG),
                             sp_tr_lds(big_rows), h->stream, dev, d_list + n_wave, d_ids, d_counts, d_base, big_rows, d_heads,
                             d_spans, d_svc));
    // only the heads cross before both totals are known
    SP_HIP(h, hipMemcpyAsync(heads, d_heads, (size_t)n * sizeof(zk_sp_trace), hipMemcpyDeviceToHost, h->stream));
    if (h->timing) SP_HIP(h, hipEventRecord(h->qev[1], h->stream));
    SP_HIP(h, hipStreamSynchronize(h->stream));
    h->qtimed = h->timing;
    uint64_t need_spans = 0, need_svc = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (heads[i].spans > counts[i] || heads[i].services > counts[i])
            return sfail(h, ZK_ERR_HIP, "a merged trace has more spans or services than its trace has rows");
        need_spans += heads[i].spans;
        need_svc += heads[i].services;
    }
    n_out[0] = need_spans;
    n_out[1] = need_svc;
    if (need_spans > cap_spans || need_svc > cap_services)
        return sfail(h, ZK_ERR_CAPACITY, "the outputs hold fewer spans or services than the asked traces have");
    if (need_spans == 0) return ZK_OK;
    // the staged spans and services in one copy, then each trace's packed behind the ones before it
    const size_t bytes = span_bytes + (size_t)total * 4;
    h->tr_host.resize(bytes);
    SP_HIP(h, hipMemcpyAsync(h->tr_host.data(), h->tr_out, bytes, hipMemcpyDeviceToHost, h->stream));
    if (h->timing) SP_HIP(h, hipEventRecord(h->qev[1], h->stream));
    SP_HIP(h, hipStreamSynchronize(h->stream));
    const zk_sp_span* s_spans = (const zk_sp_span*)h->tr_host.data();
    const uint32_t* s_svc = (const uint32_t*)(h->tr_host.data() + span_bytes);
    uint64_t at = 0, at_svc = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t c = heads[i].spans, v = heads[i].services, from = h->base_host[i];
        if (c) memcpy(spans + at, s_spans + from, c * sizeof(zk_sp_span));
        if (v) memcpy(services + at_svc, s_svc + from, v * 4);
        at += c;
        at_svc += v;
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_sp_query_ms(zk_sp* h, double* ms) {
    ZK_GUARD_BEGIN
    if (!h || !ms) return ZK_ERR_INVALID_ARG;
    if (!h->qtimed) return sfail(h, ZK_ERR_INVALID_ARG, "no timed lookup has run a pass (zk_sp_config.timing)");
    SP_HIP(h, hipSetDevice(h->device));
    float f = 0.f;
    SP_HIP(h, hipEventElapsedTime(&f, h->qev[0], h->qev[1]));
    *ms = f;
    return ZK_OK;
    ZK_GUARD_END
}

}  // extern "C"

// ---- the staging, for the joint kernels (zk_sp_staged.h) -------------------------------------------------
namespace zk {

int sp_device(const zk_sp* h) { return h->device; }

// zk_sp_traces' staging as it stands: the layout is that call's (the spans, then the services 256-B aligned
// behind them, both at the traces' row bases).
void sp_staged_traces(const zk_sp* h, SpStagedTraces* out) {
    *out = SpStagedTraces();
    out->device = h->device;
    if (!h->q || !h->tr_heads || !h->tr_out || h->base_host.empty() || h->base_host.size() != h->sum_counts_host.size()) return;
    const uint64_t total = h->base_host.back() + h->sum_counts_host.back();
    if (total == 0 || al256((size_t)total * sizeof(zk_sp_span)) + Block::col4(total) > h->tr_bytes) return;
    out->heads = (const zk_sp_trace*)h->tr_heads;
    out->spans = (const zk_sp_span*)h->tr_out;
    out->services = (const uint32_t*)((const uint8_t*)h->tr_out + al256((size_t)total * sizeof(zk_sp_span)));
    out->base = (const unsigned long long*)((const uint8_t*)h->q + kQBaseAt);
    out->base_host = h->base_host.data();
    out->total = total;
}

}  // namespace zk
