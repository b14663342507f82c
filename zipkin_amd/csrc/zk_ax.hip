// zk_ax.hip — the trace-id index by annotation (include/zkannindex.h): segments of entries grouped by
// service in HBM, and the radix select of the newest trace ids of one (service, key[, value]) row.
//
// The design is zk_ix.hip's with another entry: a segment is one allocation of four columns,
// tkey[u64] = ts ^ sign, tid[u64], key[u64], val[u64], each 256-B aligned, with the entries of service s
// at [off[s], off[s + 1]); `off` lives on the host.
//
//   k_ax_count    the batch's entries per service: a per-workgroup LDS histogram of up to 4096 bins,
//                 lanes of a wave that share a bin added once, flushed with atomics; the same pass
//                 counts the entries whose service id is out of range. 4 B per entry.
//   (host)        the counts' exclusive scan = the segment's offsets; they also start the cursors.
//   k_ax_scatter  a workgroup owns a stretch of the batch and walks it twice: an LDS histogram of its
//                 entries, ONE returning atomic per workgroup and service with entries to claim that
//                 many places behind the service's cursor, then every entry again, its rank inside the
//                 workgroup from LDS. 36 B per entry read once and the service (4 B) once more, 32 B
//                 written per entry.
//   k_ax_merge    one old segment's entries into the merged one (zk_ix.hip's k_ix_merge, four columns)
//   k_ax_scan, k_ax_hist, k_ax_collect   zk_ax_trace_ids' passes: those of zk_ix.hip, over a filter
//                 that reads key, then val where the key matched and a value was asked, then tkey and
//                 tid where both matched
//   k_ax_expire_count, k_ax_expire_rewrite   zk_ax_expire's passes (zk_expire.h, as in zk_ix.hip): the
//                 survivors per (segment, service) from the tkey column alone, then the survivors of the
//                 mixed segments into one new segment, the service of an entry from its place
//
// Every store is bounded: the scatter and the merge drop a place at or past the segment's size (it
// cannot arise while the columns stay as they were between the count and the scatter, which the header
// asks of the caller; a caller that breaks it loses entries and corrupts nothing), the collect drops
// entries past its lists' capacities, the expiry's rewrite a place at or past the new segment's size.
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>
#include <vector>

#include "zk_expire.h"
#include "zk_guard.h"
#include "zk_hist.h"
#include "zk_ix_select.h"
#include "zk_launch.h"
#include "zkannindex.h"

namespace zk {
namespace {

constexpr int kAxWG = 256;
constexpr uint32_t kAxSvcBins = ZK_AX_MAX_SERVICES;
constexpr uint32_t kAxMaxGrid = 4096;
constexpr uint32_t kAxHistGrid = 1024;         // k_ax_count, k_ax_hist: every workgroup flushes up to 4096 bins
constexpr uint32_t kAxScatterPerWG = 16384;    // k_ax_scatter: entries per workgroup at least (S atomics each)
constexpr uint32_t kAxCap = ZK_AX_MAX_LIMIT;   // the most entries the select brings to the host
constexpr uint64_t kAxMaxEntries = 0xFFFFFFFFull;
constexpr int kCntItems = 4;                   // the counting loops: entries per thread and step
constexpr uint32_t kCntTile = kAxWG * kCntItems;
// the select's counters (those of zk_ix.hip)
enum { kSelMatched = 0, kSelCertain = 1, kSelOrHi = 2, kSelNorHi = 3, kSelOrLo = 4, kSelNorLo = 5, kSelCand = 6, kSelWords = 8 };

// a service's entries in one segment, or (key == nullptr) a list of 16-B entries {tkey, traceId} at tkey
struct AxSlice {
    const unsigned long long* tkey;
    const unsigned long long* tid;
    const unsigned long long* key;
    const unsigned long long* val;
    unsigned long long count;
};
// what a query takes of a slice (a list: everything)
struct AxFilter {
    unsigned long long max_key;  // end_ts ^ sign
    unsigned long long key;
    unsigned long long val;      // ZK_AX_ANY_VALUE or a value hash
};

// byte offsets in the select's scratch block
constexpr size_t kSelHistAt = 256;
constexpr size_t kSelCertainAt = kSelHistAt + kTdBins * 4;
constexpr size_t kSelSlicesAt = kSelCertainAt + (size_t)kAxCap * sizeof(IxEntry);
constexpr size_t kSelBytes = kSelSlicesAt + ZK_AX_MAX_SEGMENTS * sizeof(AxSlice);
// the observe's block: the counts, the cursors, then the range violations
constexpr size_t kObsCursorAt = kAxSvcBins * 4;
constexpr size_t kObsStatAt = 2 * kAxSvcBins * 4;
constexpr size_t kObsBytes = kObsStatAt + 64;

static_assert(sizeof(IxEntry) == 16 && sizeof(AxSlice) == 40, "entry and slice layouts");
static_assert(kSelWords * 8 <= kSelHistAt && kSelCertainAt % 16 == 0 && kSelSlicesAt % 8 == 0, "the scratch block's layout");

uint32_t ax_grid(uint64_t items, uint32_t cap = kAxMaxGrid) {
    const uint64_t g = (items + kAxWG - 1) / kAxWG;
    return (uint32_t)(g < 1 ? 1 : g > cap ? cap : g);
}

// ---- observe -------------------------------------------------------------------------------------------
// counts[s] += the entries of service s (s < S); stat[0] += the entries with s >= S. The loop's bounds
// are the same for all threads of a workgroup, so every lane reaches the ballots.
__global__ __launch_bounds__(kAxWG) void k_ax_count(const uint32_t* __restrict__ svc, unsigned long long n, uint32_t S,
                                                    uint32_t* __restrict__ counts, unsigned long long* __restrict__ stat) {
    __shared__ uint32_t s_hist[kAxSvcBins];
    __shared__ uint32_t s_bad;
    for (uint32_t b = threadIdx.x; b < kAxSvcBins; b += kAxWG) s_hist[b] = 0u;
    if (threadIdx.x == 0) s_bad = 0u;
    __syncthreads();
    const unsigned long long stride = (unsigned long long)gridDim.x * kCntTile;
    for (unsigned long long base = (unsigned long long)blockIdx.x * kCntTile; base < n; base += stride) {
        uint32_t s[kCntItems];  // (the tile's loads first, then the ballots)
#pragma unroll
        for (int j = 0; j < kCntItems; ++j) {
            const unsigned long long i = base + (unsigned long long)j * kAxWG + threadIdx.x;
            s[j] = i < n ? svc[i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kCntItems; ++j) {
            const bool valid = base + (unsigned long long)j * kAxWG + threadIdx.x < n;
            if (valid && s[j] >= S) atomicAdd(&s_bad, 1u);
            hist_add(s_hist, valid && s[j] < S, s[j]);
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kAxSvcBins; b += kAxWG) {
        const uint32_t c = s_hist[b];
        if (c && b < S) atomicAdd(&counts[b], c);
    }
    if (threadIdx.x == 0 && s_bad) atomicAdd(&stat[0], (unsigned long long)s_bad);
}

// Workgroup b owns entries [b * chunk, (b + 1) * chunk) (chunk a multiple of the workgroup). cursor[s]
// starts at the segment's off[s]; `total` is the segment's size. hist_add and hist_rank index LDS with
// the service only under s < S <= kAxSvcBins.
__global__ __launch_bounds__(kAxWG) void k_ax_scatter(const uint32_t* __restrict__ svc, const unsigned long long* __restrict__ key,
                                                      const unsigned long long* __restrict__ val, const long long* __restrict__ ts,
                                                      const unsigned long long* __restrict__ tid, unsigned long long n,
                                                      unsigned long long chunk, uint32_t S, uint32_t* __restrict__ cursor,
                                                      unsigned long long total, unsigned long long* __restrict__ out_tkey,
                                                      unsigned long long* __restrict__ out_tid, unsigned long long* __restrict__ out_key,
                                                      unsigned long long* __restrict__ out_val) {
    __shared__ uint32_t s_cnt[kAxSvcBins];   // the stretch's entries per service, then the ranks given out
    __shared__ uint32_t s_base[kAxSvcBins];  // where the workgroup's places of a service begin
    const unsigned long long lo = (unsigned long long)blockIdx.x * chunk;
    const unsigned long long hi = lo + chunk < n ? lo + chunk : n;
    for (uint32_t b = threadIdx.x; b < kAxSvcBins; b += kAxWG) s_cnt[b] = 0u;
    __syncthreads();
    for (unsigned long long base = lo; base < hi; base += kCntTile) {
        uint32_t s[kCntItems];
#pragma unroll
        for (int j = 0; j < kCntItems; ++j) {
            const unsigned long long i = base + (unsigned long long)j * kAxWG + threadIdx.x;
            s[j] = i < hi ? svc[i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kCntItems; ++j)
            hist_add(s_cnt, base + (unsigned long long)j * kAxWG + threadIdx.x < hi && s[j] < S, s[j]);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kAxSvcBins; b += kAxWG) {
        const uint32_t c = s_cnt[b];
        if (c && b < S) s_base[b] = atomicAdd(&cursor[b], c);
        s_cnt[b] = 0u;
    }
    __syncthreads();
    for (unsigned long long base = lo; base < hi; base += kAxWG) {
        const unsigned long long i = base + threadIdx.x;
        const bool valid = i < hi;
        const uint32_t s = valid ? svc[i] : 0u;
        const bool take = valid && s < S;
        const uint32_t rank = hist_rank(s_cnt, take, s);
        if (take) {
            const unsigned long long at = (unsigned long long)s_base[s] + rank;
            if (at < total) {
                out_tkey[at] = (unsigned long long)ts[i] ^ kTdSign;
                out_tid[at] = tid[i];
                out_key[at] = key[i];
                out_val[at] = val[i];
            }
        }
    }
}

// one column of a segment: src / dst + c * stride (in words)
struct AxCols {
    unsigned long long* p;
    unsigned long long stride;
};

// src_off[S + 1]: the old segment's offsets; dst_base[S]: where its slice of each service begins in
// the merged segment
__global__ __launch_bounds__(kAxWG) void k_ax_merge(AxCols src, unsigned long long n_src, const unsigned long long* __restrict__ src_off,
                                                    const unsigned long long* __restrict__ dst_base, uint32_t S, AxCols dst,
                                                    unsigned long long dst_total) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kAxWG;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kAxWG + threadIdx.x; i < n_src; i += stride) {
        // the last service whose offset is <= i (src_off[0] = 0 <= i < n_src = src_off[S]): the ones
        // behind it that share the offset are empty
        uint32_t a = 0, b = S;
        while (b - a > 1) {
            const uint32_t mid = (a + b) >> 1;
            if (src_off[mid] <= i) a = mid; else b = mid;
        }
        const unsigned long long at = dst_base[a] + (i - src_off[a]);
        if (at < dst_total) {
#pragma unroll
            for (int c = 0; c < 4; ++c) dst.p[c * dst.stride + at] = src.p[c * src.stride + i];
        }
    }
}

// ---- the select (zk_ix.hip's passes and termination argument; only the filter differs) ------------------
__device__ inline bool ax_load(const AxSlice& s, unsigned long long i, const AxFilter& f, IxEntry* e) {
    if (i >= s.count) return false;
    if (!s.key) {
        e->tkey = s.tkey[2 * i];
        e->id = s.tkey[2 * i + 1];
        return true;
    }
    if (s.key[i] != f.key) return false;
    if (f.val != ZK_AX_ANY_VALUE && s.val[i] != f.val) return false;
    e->tkey = s.tkey[i];
    if (e->tkey > f.max_key) return false;
    e->id = s.tid[i];
    return true;
}

__device__ inline unsigned long long wave_or(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off);
    return v;
}

__device__ inline void flush_bits(unsigned long long or_hi, unsigned long long nor_hi, unsigned long long or_lo,
                                  unsigned long long nor_lo, unsigned long long* __restrict__ sel) {
    or_hi = wave_or(or_hi);
    nor_hi = wave_or(nor_hi);
    or_lo = wave_or(or_lo);
    nor_lo = wave_or(nor_lo);
    if (lane_id() == 0 && (or_hi | nor_hi | or_lo | nor_lo)) {
        atomicOr(&sel[kSelOrHi], or_hi);
        atomicOr(&sel[kSelNorHi], nor_hi);
        atomicOr(&sel[kSelOrLo], or_lo);
        atomicOr(&sel[kSelNorLo], nor_lo);
    }
}

// A grid's y index picks the slice; a list is the one slice passed by value.
__global__ __launch_bounds__(kAxWG) void k_ax_scan(const AxSlice* __restrict__ slices, AxSlice one, AxFilter flt,
                                                   unsigned long long* __restrict__ sel) {
    const AxSlice sl = slices ? slices[blockIdx.y] : one;
    const unsigned long long stride = (unsigned long long)gridDim.x * kAxWG;
    unsigned long long or_hi = 0, nor_hi = 0, or_lo = 0, nor_lo = 0, cnt = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kAxWG + threadIdx.x; i < sl.count; i += stride) {
        IxEntry e;
        if (!ax_load(sl, i, flt, &e)) continue;
        or_hi |= ~e.tkey;
        nor_hi |= e.tkey;
        or_lo |= e.id;
        nor_lo |= ~e.id;
        ++cnt;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if (lane_id() == 0 && cnt) atomicAdd(&sel[kSelMatched], cnt);
    flush_bits(or_hi, nor_hi, or_lo, nor_lo, sel);
}

// td_digit is below kTdBins for any key and shift: it indexes s_hist
__global__ __launch_bounds__(kAxWG) void k_ax_hist(const AxSlice* __restrict__ slices, AxSlice one, AxFilter flt, uint32_t shift,
                                                   uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[kTdBins];
    const AxSlice sl = slices ? slices[blockIdx.y] : one;
    for (uint32_t b = threadIdx.x; b < kTdBins; b += kAxWG) s_hist[b] = 0u;
    __syncthreads();
    const unsigned long long stride = (unsigned long long)gridDim.x * kAxWG;
    for (unsigned long long base = (unsigned long long)blockIdx.x * kAxWG; base < sl.count; base += stride) {
        IxEntry e{0, 0};
        const bool ok = ax_load(sl, base + threadIdx.x, flt, &e);
        hist_add(s_hist, ok, td_digit(~e.tkey, e.id, shift));
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kTdBins; b += kAxWG) {
        const uint32_t c = s_hist[b];
        if (c) atomicAdd(&hist[b], c);
    }
}

// digit < bin: certain; digit == bin: a candidate (bin = kTdBins: every matching entry is certain).
// zk_ix.hip's k_ix_collect: a workgroup walks tiles of kColTile entries, each wave ranks its takers of
// both kinds with ballots, one thread per list draws the tile's stretch with a returning atomicAdd.
constexpr int kColItems = 4;
constexpr uint32_t kColTile = kAxWG * kColItems;
constexpr int kColWaves = kAxWG / 64;

__device__ inline void put_entry(unsigned long long* __restrict__ out, unsigned long long cap, unsigned long long at,
                                 const IxEntry& e) {
    if (at < cap) {
        out[2 * at] = e.tkey;
        out[2 * at + 1] = e.id;
    }
}

__global__ __launch_bounds__(kAxWG) void k_ax_collect(const AxSlice* __restrict__ slices, AxSlice one, AxFilter flt, uint32_t shift,
                                                      uint32_t bin, unsigned long long* __restrict__ sel,
                                                      unsigned long long* __restrict__ certain, unsigned long long certain_cap,
                                                      unsigned long long* __restrict__ cand, unsigned long long cand_cap) {
    __shared__ uint32_t s_cnt[2][kColWaves];
    __shared__ unsigned long long s_base[2];
    const AxSlice sl = slices ? slices[blockIdx.y] : one;
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const unsigned long long stride = (unsigned long long)gridDim.x * kColTile;
    unsigned long long or_hi = 0, nor_hi = 0, or_lo = 0, nor_lo = 0;
    for (unsigned long long tile = (unsigned long long)blockIdx.x * kColTile; tile < sl.count; tile += stride) {
        IxEntry e[kColItems];
        uint32_t kind[kColItems], rank[kColItems];  // kind: 0 dropped, 1 certain, 2 candidate; rank in the wave's takers
        uint32_t wc = 0, ws = 0;                    // the wave's takers so far (wave-uniform)
#pragma unroll
        for (int j = 0; j < kColItems; ++j) {
            e[j] = IxEntry{0, 0};
            const bool ok = ax_load(sl, tile + (unsigned long long)j * kAxWG + threadIdx.x, flt, &e[j]);
            const uint32_t d = td_digit(~e[j].tkey, e[j].id, shift);
            const bool below = ok && d < bin, stays = ok && d == bin;
            const unsigned long long mb = __ballot(below), ms = __ballot(stays);
            kind[j] = below ? 1u : stays ? 2u : 0u;
            rank[j] = (below ? wc : ws) + rank_in(below ? mb : ms);
            wc += (uint32_t)__popcll(mb);
            ws += (uint32_t)__popcll(ms);
            if (stays) {
                or_hi |= ~e[j].tkey;
                nor_hi |= e[j].tkey;
                or_lo |= e[j].id;
                nor_lo |= ~e[j].id;
            }
        }
        if (lane == 0) {
            s_cnt[0][wave] = wc;
            s_cnt[1][wave] = ws;
        }
        __syncthreads();
        if (lane == 0 && wave < 2) {  // wave 0 draws the certain stretch, wave 1 the candidates'
            uint32_t total = 0;
            for (int w = 0; w < kColWaves; ++w) total += s_cnt[wave][w];
            s_base[wave] = total ? atomicAdd(&sel[wave == 0 ? kSelCertain : kSelCand], (unsigned long long)total) : 0ull;
        }
        __syncthreads();
        unsigned long long at_c = s_base[0], at_s = s_base[1];
        for (uint32_t w = 0; w < wave; ++w) {
            at_c += s_cnt[0][w];
            at_s += s_cnt[1][w];
        }
#pragma unroll
        for (int j = 0; j < kColItems; ++j) {
            if (kind[j] == 1u) put_entry(certain, certain_cap, at_c + rank[j], e[j]);
            if (kind[j] == 2u) put_entry(cand, cand_cap, at_s + rank[j], e[j]);
        }
        __syncthreads();  // (the next tile overwrites s_cnt and s_base)
    }
    flush_bits(or_hi, nor_hi, or_lo, nor_lo, sel);
}

// ---- expiry (zk_expire.h) -----------------------------------------------------------------------------
static_assert(kExpBins == kAxSvcBins && kExpWG == kAxWG, "zk_expire.h's bins and workgroup are this file's");

__global__ __launch_bounds__(kExpWG) void k_ax_expire_count(const ExpSeg* __restrict__ segs, const ExpItem* __restrict__ items,
                                                            unsigned long long chunk, uint32_t S, unsigned long long cut,
                                                            uint32_t* __restrict__ surv) {
    __shared__ ExpLds lds;
    exp_count(segs, items, chunk, S, cut, surv, &lds);
}

// an old segment's entry into the new one: tid, key and val lie behind tkey (Segment's layout); 32 B written
struct AxPut {
    AxCols dst;
    __device__ void operator()(const ExpSeg& sg, unsigned long long i, unsigned long long k, unsigned long long at) const {
        const unsigned long long col = (sg.n * 8ull + 255ull) / 256ull * 32ull;  // a column, in words
        dst.p[at] = k;
#pragma unroll
        for (int c = 1; c < 4; ++c) dst.p[c * dst.stride + at] = sg.tkey[c * col + i];
    }
};

__global__ __launch_bounds__(kExpWG) void k_ax_expire_rewrite(const ExpSeg* __restrict__ segs, const ExpItem* __restrict__ items,
                                                              unsigned long long chunk, uint32_t S, unsigned long long cut,
                                                              uint32_t* __restrict__ cursor, unsigned long long total, AxPut put) {
    __shared__ ExpLds lds;
    __shared__ uint32_t s_base[kExpBins];
    exp_rewrite(segs, items, chunk, S, cut, cursor, total, put, &lds, s_base);
}

struct Segment {
    void* block = nullptr;
    size_t bytes = 0;
    uint64_t n = 0;
    std::vector<uint64_t> off;  // num_services + 1

    static size_t col8(uint64_t n) { return (size_t)((n * 8 + 255) / 256 * 256); }
    static size_t bytes_for(uint64_t n) { return 4 * col8(n); }
    unsigned long long* col(int c) const { return (unsigned long long*)((uint8_t*)block + (size_t)c * col8(n)); }
    unsigned long long* tkey() const { return col(0); }
    unsigned long long* tid() const { return col(1); }
    unsigned long long* key() const { return col(2); }
    unsigned long long* val() const { return col(3); }
    AxCols cols() const { return AxCols{col(0), (unsigned long long)(col8(n) / 8)}; }
};

}  // namespace
}  // namespace zk

using namespace zk;

struct zk_ax {
    int device = 0;
    uint32_t S = 0;
    hipStream_t stream = nullptr, own = nullptr;
    bool timing = false;
    std::vector<Segment> segs;
    std::vector<uint64_t> svc_count;    // entries per service
    uint64_t entries = 0;
    void* obs = nullptr;                // the observe's counts, cursors and range violations (kObsBytes)
    void* stage = nullptr;              // the five columns of a host batch
    void* mplan = nullptr;              // a merge's offsets and bases, per old segment
    void* xplan = nullptr;              // an expiry's segments, offsets, work items, survivor counts and cursors
    void* sel = nullptr;                // the select's counters, histogram, certain list, slices (kSelBytes)
    void* list[2] = {nullptr, nullptr}; // the candidate lists, written in turn
    size_t stage_bytes = 0, mplan_bytes = 0, xplan_bytes = 0, sel_bytes = 0, list_bytes[2] = {0, 0};
    std::vector<uint32_t> counts_host, cursor_host;  // (a queued copy reads cursor_host: it changes only behind a synchronisation)
    std::vector<uint64_t> mplan_host;
    std::vector<uint8_t> xplan_host;                 // (an expiry's queued copies read these three: likewise)
    std::vector<uint32_t> xsurv_host, xcursor_host;
    std::vector<ExpItem> xitems_host;
    std::vector<AxSlice> slices_host;
    std::vector<IxSpan> spans;
    hipEvent_t oev[4] = {};  // around the passes of the last observe (zk_ax_observe_ms)
    hipEvent_t qev[2] = {};  // around the last query (zk_ax_query_ms)
    hipEvent_t xev[4] = {};  // around the passes of the last expiry (zk_ax_expire_ms)
    bool otimed = false, qtimed = false, xtimed = false;
    std::string err;
};

namespace {

zk_status xfail(zk_ax* h, zk_status s, const std::string& m) {
    if (h) h->err = m;
    return s;
}

#define AX_HIP(h, call)                                                                            \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess) return xfail(h, is_refusal(_e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP,       \
                                           std::string(#call) + ": " + launch_error_str(_e));      \
    } while (0)

// a fresh block of `need` bytes; a refused allocation is ZK_ERR_CAPACITY
zk_status alloc(zk_ax* h, void** p, size_t need, const char* what) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, need ? need : 8);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (e != hipErrorOutOfMemory) return xfail(h, ZK_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        return xfail(h, ZK_ERR_CAPACITY, std::string("no device memory for ") + what);
    }
    *p = q;
    return ZK_OK;
}

// at least `need` bytes behind *p: a larger block first, then the old one freed (its content is not
// kept); a refused allocation leaves *p as it was
zk_status grow(zk_ax* h, void** p, size_t* have, size_t need, const char* what) {
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

void free_segments(zk_ax* h) {
    if (!h->segs.empty()) (void)hipStreamSynchronize(h->stream);
    for (Segment& g : h->segs)
        if (g.block) (void)hipFree(g.block);
    h->segs.clear();
}

// All segments into one: each service's slices concatenated in segment order. Anything refused leaves
// the index as it was. Synchronises.
zk_status merge_all(zk_ax* h) {
    const uint32_t S = h->S, G = (uint32_t)h->segs.size();
    if (G < 2) return ZK_OK;
    Segment m;
    m.n = h->entries;
    m.off.assign(S + 1, 0);
    for (uint32_t s = 0; s < S; ++s) m.off[s + 1] = m.off[s] + h->svc_count[s];
    if (m.off[S] != m.n) return xfail(h, ZK_ERR_HIP, "the segments' offsets do not add up");
    // per old segment: its offsets [S + 1], then the bases of its slices in the merged segment [S]
    const size_t per = 2 * (size_t)S + 1;
    h->mplan_host.assign(per * G, 0);
    std::vector<uint64_t> next(m.off.begin(), m.off.begin() + S);
    for (uint32_t g = 0; g < G; ++g) {
        uint64_t* p = h->mplan_host.data() + per * g;
        const Segment& sg = h->segs[g];
        for (uint32_t s = 0; s <= S; ++s) p[s] = sg.off[s];
        for (uint32_t s = 0; s < S; ++s) {
            p[S + 1 + s] = next[s];
            next[s] += sg.off[s + 1] - sg.off[s];
        }
    }
    zk_status st = grow(h, &h->mplan, &h->mplan_bytes, per * G * 8, "a merge's offsets");
    if (st != ZK_OK) return st;
    m.bytes = Segment::bytes_for(m.n);
    if ((st = alloc(h, &m.block, m.bytes, "the merged segment (32 B per entry)")) != ZK_OK) return st;
    hipError_t e = hipMemcpyAsync(h->mplan, h->mplan_host.data(), per * G * 8, hipMemcpyHostToDevice, h->stream);
    for (uint32_t g = 0; g < G && e == hipSuccess; ++g) {
        const Segment& sg = h->segs[g];
        const unsigned long long* p = (const unsigned long long*)h->mplan + per * g;
        e = launch_checked("k_ax_merge", k_ax_merge, dim3(ax_grid(sg.n)), dim3(kAxWG), 0, h->stream, sg.cols(),
                           (unsigned long long)sg.n, p, p + S + 1, S, m.cols(), (unsigned long long)m.n);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(m.block);
        return xfail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("merging the segments: ") + launch_error_str(e));
    }
    free_segments(h);
    h->segs.push_back(std::move(m));
    return ZK_OK;
}

// The asked service's slices into the scratch block (and h->spans); *total = the entries they hold,
// *longest = those of the longest.
zk_status plan_slices(zk_ax* h, uint32_t service, uint64_t* total, uint64_t* longest) {
    std::vector<const uint64_t*> offs(h->segs.size());
    for (size_t g = 0; g < h->segs.size(); ++g) offs[g] = h->segs[g].off.data();
    *total = ix_plan(offs.data(), (uint32_t)offs.size(), service, &h->spans);
    *longest = 0;
    if (!*total) return ZK_OK;
    zk_status st = grow(h, &h->sel, &h->sel_bytes, kSelBytes, "the select's counters and lists");
    if (st != ZK_OK) return st;
    h->slices_host.clear();
    for (const IxSpan& sp : h->spans) {
        const Segment& g = h->segs[sp.segment];
        h->slices_host.push_back(AxSlice{g.tkey() + sp.start, g.tid() + sp.start, g.key() + sp.start, g.val() + sp.start, sp.count});
        if (sp.count > *longest) *longest = sp.count;
    }
    AX_HIP(h, hipMemcpyAsync((uint8_t*)h->sel + kSelSlicesAt, h->slices_host.data(), h->slices_host.size() * sizeof(AxSlice),
                             hipMemcpyHostToDevice, h->stream));
    return ZK_OK;
}

// zk_ax_expire behind its argument checks: every entry with tkey < cut goes. The count pass over all
// segments, the one synchronisation that sizes the rest, then the segments sorted into untouched (no
// entry goes: not read again), gone (every entry goes: freed) and mixed (their survivors rewritten into
// ONE new segment, which takes the place of the first of them). Nothing is freed and no bookkeeping
// changes before the new segment is complete; anything refused leaves the index as it was.
zk_status expire(zk_ax* h, unsigned long long cut, uint64_t* removed_out) {
    const uint32_t S = h->S, G = (uint32_t)h->segs.size();
    const auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const auto items_at = [&](uint64_t c) {
        uint64_t w = 0;
        for (const Segment& g : h->segs) w += (g.n + c - 1) / c;
        return w;
    };
    uint64_t chunk = kExpPerWG;
    while (items_at(chunk) > kExpMaxItems + G) chunk *= 2;
    const uint32_t W = (uint32_t)items_at(chunk);
    // the plan: the segments, their offsets [G][S + 1], the work items, then what the device writes:
    // the survivors [G][S] and the new segment's cursors [S]
    const size_t off_at = al(G * sizeof(ExpSeg)), item_at = off_at + al((size_t)G * (S + 1) * 4);
    const size_t surv_at = item_at + al((size_t)W * sizeof(ExpItem)), cur_at = surv_at + al((size_t)G * S * 4);
    zk_status st = grow(h, &h->xplan, &h->xplan_bytes, cur_at + al((size_t)S * 4), "an expiry's plan");
    if (st != ZK_OK) return st;
    uint8_t* xp = (uint8_t*)h->xplan;
    h->xplan_host.assign(surv_at, 0);
    ExpSeg* hs = (ExpSeg*)h->xplan_host.data();
    uint32_t* ho = (uint32_t*)(h->xplan_host.data() + off_at);
    ExpItem* hi = (ExpItem*)(h->xplan_host.data() + item_at);
    uint32_t w = 0;
    for (uint32_t g = 0; g < G; ++g) {
        const Segment& sg = h->segs[g];
        hs[g] = ExpSeg{sg.tkey(), (unsigned long long)sg.n, (const uint32_t*)(xp + off_at) + (size_t)g * (S + 1)};
        for (uint32_t s = 0; s <= S; ++s) ho[(size_t)g * (S + 1) + s] = (uint32_t)sg.off[s];
        for (uint64_t c = 0; c * chunk < sg.n; ++c) hi[w++] = ExpItem{g, (uint32_t)c};
    }
    const ExpSeg* segs = (const ExpSeg*)xp;
    const ExpItem* items = (const ExpItem*)(xp + item_at);
    uint32_t* surv = (uint32_t*)(xp + surv_at);
    uint32_t* cursor = (uint32_t*)(xp + cur_at);
    const bool timing = h->timing;
    for (hipEvent_t& e : h->xev)
        if (timing && !e) AX_HIP(h, hipEventCreate(&e));
    AX_HIP(h, hipMemcpyAsync(xp, h->xplan_host.data(), surv_at, hipMemcpyHostToDevice, h->stream));
    AX_HIP(h, hipMemsetAsync(surv, 0, (size_t)G * S * 4, h->stream));
    if (timing) AX_HIP(h, hipEventRecord(h->xev[0], h->stream));
    AX_HIP(h, launch_checked("k_ax_expire_count", k_ax_expire_count, dim3(W), dim3(kExpWG), 0, h->stream, segs, items,
                             (unsigned long long)chunk, S, cut, surv));
    if (timing) AX_HIP(h, hipEventRecord(h->xev[1], h->stream));
    h->xsurv_host.resize((size_t)G * S);
    AX_HIP(h, hipMemcpyAsync(h->xsurv_host.data(), surv, (size_t)G * S * 4, hipMemcpyDeviceToHost, h->stream));
    AX_HIP(h, hipStreamSynchronize(h->stream));  // the sizing synchronisation
    std::vector<uint64_t> keep(G, 0), gone(S, 0);
    std::vector<uint32_t> mixed;
    uint64_t removed = 0;
    for (uint32_t g = 0; g < G; ++g) {
        const Segment& sg = h->segs[g];
        for (uint32_t s = 0; s < S; ++s) {
            const uint64_t len = sg.off[s + 1] - sg.off[s], c = h->xsurv_host[(size_t)g * S + s];
            if (c > len) return xfail(h, ZK_ERR_HIP, "the expiry counted more survivors than a slice holds");
            keep[g] += c;
            gone[s] += len - c;
        }
        removed += sg.n - keep[g];
        if (keep[g] != 0 && keep[g] != sg.n) mixed.push_back(g);
    }
    if (removed == 0) {  // nothing goes: nothing is rewritten, reallocated or freed
        if (timing) AX_HIP(h, hipEventRecord(h->xev[2], h->stream));
        if (timing) AX_HIP(h, hipEventRecord(h->xev[3], h->stream));
        h->xtimed = timing;
        return ZK_OK;
    }
    Segment m;
    if (!mixed.empty()) {
        m.off.assign(S + 1, 0);
        for (uint32_t s = 0; s < S; ++s) {
            uint64_t c = 0;
            for (uint32_t g : mixed) c += h->xsurv_host[(size_t)g * S + s];
            m.off[s + 1] = m.off[s] + c;
        }
        m.n = m.off[S];
        m.bytes = Segment::bytes_for(m.n);
        if ((st = alloc(h, &m.block, m.bytes, "the survivors' segment (32 B per entry)")) != ZK_OK) return st;
        h->xcursor_host.resize(S);
        for (uint32_t s = 0; s < S; ++s) h->xcursor_host[s] = (uint32_t)m.off[s];
        h->xitems_host.clear();
        for (uint32_t g : mixed)
            for (uint64_t c = 0; c * chunk < h->segs[g].n; ++c) h->xitems_host.push_back(ExpItem{g, (uint32_t)c});
    }
    hipError_t e = hipSuccess;
    if (!mixed.empty()) {
        e = hipMemcpyAsync(xp + item_at, h->xitems_host.data(), h->xitems_host.size() * sizeof(ExpItem), hipMemcpyHostToDevice,
                           h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cursor, h->xcursor_host.data(), (size_t)S * 4, hipMemcpyHostToDevice, h->stream);
    }
    if (e == hipSuccess && timing) e = hipEventRecord(h->xev[2], h->stream);
    if (e == hipSuccess && !mixed.empty())
        e = launch_checked("k_ax_expire_rewrite", k_ax_expire_rewrite, dim3((uint32_t)h->xitems_host.size()), dim3(kExpWG), 0,
                           h->stream, segs, items, (unsigned long long)chunk, S, cut, cursor, (unsigned long long)m.n,
                           AxPut{m.cols()});
    if (e == hipSuccess && timing) e = hipEventRecord(h->xev[3], h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        if (m.block) (void)hipFree(m.block);
        return xfail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("rewriting the survivors: ") + launch_error_str(e));
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
    for (uint32_t s = 0; s < S; ++s) h->svc_count[s] -= gone[s];
    h->entries -= removed;
    h->xtimed = timing;
    if (removed_out) *removed_out = removed;
    return ZK_OK;
}

}  // namespace

extern "C" {

zk_status zk_ax_create(const zk_ax_config* cfg, zk_ax** out) {
    ZK_GUARD_BEGIN
    if (!cfg || !out) return ZK_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->num_services < 1 || cfg->num_services > ZK_AX_MAX_SERVICES) return ZK_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || cfg->device < 0 || cfg->device >= ndev) return ZK_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return ZK_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return ZK_ERR_NO_DEVICE;
    if (hipSetDevice(cfg->device) != hipSuccess) return ZK_ERR_HIP;
    zk_ax* h = new zk_ax();
    h->device = cfg->device;
    h->S = cfg->num_services;
    h->timing = cfg->timing != 0;
    h->svc_count.assign(h->S, 0);
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

zk_status zk_ax_destroy(zk_ax* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_segments(h);
    for (void* p : {h->obs, h->stage, h->mplan, h->xplan, h->sel, h->list[0], h->list[1]})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : h->oev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->xev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->qev)
        if (e) (void)hipEventDestroy(e);
    if (h->own) (void)hipStreamDestroy(h->own);
    delete h;
    return ZK_OK;
    ZK_GUARD_END
}

const char* zk_ax_last_error(const zk_ax* h) { return h ? h->err.c_str() : "null handle"; }

zk_status zk_ax_observe(zk_ax* h, const zk_ingest_index_items* in, uint32_t flags) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!in) return xfail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (flags & ~ZK_BATCH_DEVICE_PTRS) return xfail(h, ZK_ERR_INVALID_ARG, "unknown batch flag");
    const uint64_t n = in->n;
    if (n >= (1ull << 32)) return xfail(h, ZK_ERR_UNSUPPORTED, "2^32 entries or more in one batch");
    if (n == 0) return ZK_OK;
    if (!in->service || !in->key || !in->val || !in->ts || !in->trace_id) return xfail(h, ZK_ERR_INVALID_ARG, "null column");
    AX_HIP(h, hipSetDevice(h->device));
    const uint32_t S = h->S;
    zk_status st;
    if (!h->obs && (st = alloc(h, &h->obs, kObsBytes, "the observe's counters")) != ZK_OK) return st;
    const uint32_t* svc = in->service;
    const unsigned long long* key = (const unsigned long long*)in->key;
    const unsigned long long* val = (const unsigned long long*)in->val;
    const long long* ts = (const long long*)in->ts;
    const unsigned long long* tid = (const unsigned long long*)in->trace_id;
    if (!(flags & ZK_BATCH_DEVICE_PTRS)) {
        // a host batch: its five columns, staged (each 256-B aligned)
        const size_t a8 = (n * 8 + 255) / 256 * 256, a4 = (n * 4 + 255) / 256 * 256;
        if ((st = grow(h, &h->stage, &h->stage_bytes, 4 * a8 + a4, "staging a host batch (36 B per entry)")) != ZK_OK) return st;
        uint8_t* s = (uint8_t*)h->stage;
        AX_HIP(h, hipMemcpyAsync(s, in->key, n * 8, hipMemcpyHostToDevice, h->stream));
        AX_HIP(h, hipMemcpyAsync(s + a8, in->val, n * 8, hipMemcpyHostToDevice, h->stream));
        AX_HIP(h, hipMemcpyAsync(s + 2 * a8, in->ts, n * 8, hipMemcpyHostToDevice, h->stream));
        AX_HIP(h, hipMemcpyAsync(s + 3 * a8, in->trace_id, n * 8, hipMemcpyHostToDevice, h->stream));
        AX_HIP(h, hipMemcpyAsync(s + 4 * a8, in->service, n * 4, hipMemcpyHostToDevice, h->stream));
        key = (const unsigned long long*)s;
        val = (const unsigned long long*)(s + a8);
        ts = (const long long*)(s + 2 * a8);
        tid = (const unsigned long long*)(s + 3 * a8);
        svc = (const uint32_t*)(s + 4 * a8);
    }
    uint8_t* ob = (uint8_t*)h->obs;
    uint32_t* counts = (uint32_t*)ob;
    uint32_t* cursor = (uint32_t*)(ob + kObsCursorAt);
    unsigned long long* stat = (unsigned long long*)(ob + kObsStatAt);
    const bool timing = h->timing;
    for (hipEvent_t& e : h->oev)
        if (timing && !e) AX_HIP(h, hipEventCreate(&e));
    h->otimed = false;
    AX_HIP(h, hipMemsetAsync(counts, 0, (size_t)S * 4, h->stream));
    AX_HIP(h, hipMemsetAsync(stat, 0, 8, h->stream));
    if (timing) AX_HIP(h, hipEventRecord(h->oev[0], h->stream));
    AX_HIP(h, launch_checked("k_ax_count", k_ax_count, dim3(ax_grid((n + kCntItems - 1) / kCntItems, kAxHistGrid)), dim3(kAxWG), 0,
                             h->stream, svc, (unsigned long long)n, S, counts, stat));
    if (timing) AX_HIP(h, hipEventRecord(h->oev[1], h->stream));
    h->counts_host.resize(S);
    unsigned long long bad = 0;
    AX_HIP(h, hipMemcpyAsync(h->counts_host.data(), counts, (size_t)S * 4, hipMemcpyDeviceToHost, h->stream));
    AX_HIP(h, hipMemcpyAsync(&bad, stat, 8, hipMemcpyDeviceToHost, h->stream));
    AX_HIP(h, hipStreamSynchronize(h->stream));  // the call's one synchronisation (also: the staging copies are done)
    if (bad) return xfail(h, ZK_ERR_SERVICE_RANGE, std::to_string(bad) + " entr(ies) with service >= num_services");
    Segment g;
    g.off.assign(S + 1, 0);
    for (uint32_t s = 0; s < S; ++s) g.off[s + 1] = g.off[s] + h->counts_host[s];
    g.n = g.off[S];
    if (g.n != n) return xfail(h, ZK_ERR_HIP, "entry count out of range");
    if (h->entries + g.n > kAxMaxEntries) return xfail(h, ZK_ERR_CAPACITY, "more than 2^32 - 1 entries in one index");
    if (h->segs.size() >= ZK_AX_MAX_SEGMENTS && (st = merge_all(h)) != ZK_OK) return st;
    g.bytes = Segment::bytes_for(g.n);
    if ((st = alloc(h, &g.block, g.bytes, "a segment (32 B per entry)")) != ZK_OK) return st;
    h->cursor_host.resize(S);
    for (uint32_t s = 0; s < S; ++s) h->cursor_host[s] = (uint32_t)g.off[s];
    uint32_t grid = (uint32_t)((n + kAxScatterPerWG - 1) / kAxScatterPerWG);
    grid = grid < 1 ? 1 : grid > kAxMaxGrid ? kAxMaxGrid : grid;
    const uint64_t chunk = ((n + grid - 1) / grid + kAxWG - 1) / kAxWG * kAxWG;
    hipError_t e = hipMemcpyAsync(cursor, h->cursor_host.data(), (size_t)S * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && timing) e = hipEventRecord(h->oev[2], h->stream);
    if (e == hipSuccess)
        e = launch_checked("k_ax_scatter", k_ax_scatter, dim3(grid), dim3(kAxWG), 0, h->stream, svc, key, val, ts, tid,
                           (unsigned long long)n, (unsigned long long)chunk, S, cursor, (unsigned long long)g.n, g.tkey(), g.tid(),
                           g.key(), g.val());
    if (e == hipSuccess && timing) e = hipEventRecord(h->oev[3], h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(g.block);
        return xfail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("k_ax_scatter: ") + launch_error_str(e));
    }
    for (uint32_t s = 0; s < S; ++s) h->svc_count[s] += h->counts_host[s];
    h->entries += g.n;
    h->segs.push_back(std::move(g));
    h->otimed = timing;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_ax_observe_ms(zk_ax* h, double out[3]) {
    ZK_GUARD_BEGIN
    if (!h || !out) return ZK_ERR_INVALID_ARG;
    if (!h->otimed) return xfail(h, ZK_ERR_INVALID_ARG, "no timed observe has added a segment (zk_ax_config.timing)");
    AX_HIP(h, hipSetDevice(h->device));
    AX_HIP(h, hipEventSynchronize(h->oev[3]));
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        AX_HIP(h, hipEventElapsedTime(&ms, h->oev[k], h->oev[k + 1]));
        out[k] = ms;
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_ax_reset(zk_ax* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (h->segs.empty()) return ZK_OK;
    AX_HIP(h, hipSetDevice(h->device));
    free_segments(h);
    h->svc_count.assign(h->S, 0);
    h->entries = 0;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_ax_compact(zk_ax* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (h->segs.size() < 2) return ZK_OK;
    AX_HIP(h, hipSetDevice(h->device));
    return merge_all(h);
    ZK_GUARD_END
}

zk_status zk_ax_expire(zk_ax* h, int64_t min_ts, uint64_t* removed) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (removed) *removed = 0;
    h->xtimed = false;
    if (h->segs.empty()) return ZK_OK;
    AX_HIP(h, hipSetDevice(h->device));
    return expire(h, (unsigned long long)min_ts ^ kTdSign, removed);
    ZK_GUARD_END
}

zk_status zk_ax_expire_ms(zk_ax* h, double out[3]) {
    ZK_GUARD_BEGIN
    if (!h || !out) return ZK_ERR_INVALID_ARG;
    if (!h->xtimed) return xfail(h, ZK_ERR_INVALID_ARG, "no timed expiry has run a pass (zk_ax_config.timing)");
    AX_HIP(h, hipSetDevice(h->device));
    AX_HIP(h, hipEventSynchronize(h->xev[3]));
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        AX_HIP(h, hipEventElapsedTime(&ms, h->xev[k], h->xev[k + 1]));
        out[k] = ms;
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_ax_info(zk_ax* h, uint64_t* entries, uint64_t* segments, uint64_t* bytes) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!h->segs.empty()) {
        AX_HIP(h, hipSetDevice(h->device));
        AX_HIP(h, hipStreamSynchronize(h->stream));
    }
    uint64_t b = 0;
    for (const Segment& g : h->segs) b += g.bytes;
    if (entries) *entries = h->entries;
    if (segments) *segments = h->segs.size();
    if (bytes) *bytes = b;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_ax_service_counts(zk_ax* h, uint64_t* counts) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!counts) return xfail(h, ZK_ERR_INVALID_ARG, "null argument");
    memcpy(counts, h->svc_count.data(), (size_t)h->S * 8);
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_ax_trace_ids(zk_ax* h, uint32_t service, uint64_t key, uint64_t val, int64_t end_ts, uint32_t limit,
                          uint64_t* trace_id, int64_t* ts, uint32_t* n_out, uint64_t* matched_out) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!trace_id || !ts || !n_out) return xfail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (service >= h->S) return xfail(h, ZK_ERR_INVALID_ARG, "service >= num_services");
    if (limit < 1 || limit > ZK_AX_MAX_LIMIT) return xfail(h, ZK_ERR_INVALID_ARG, "limit outside 1..ZK_AX_MAX_LIMIT");
    *n_out = 0;
    if (matched_out) *matched_out = 0;
    if (h->svc_count[service] == 0) return ZK_OK;
    AX_HIP(h, hipSetDevice(h->device));
    uint64_t total = 0, longest = 0;
    zk_status st = plan_slices(h, service, &total, &longest);
    if (st != ZK_OK) return st;
    if (!total) return ZK_OK;
    uint8_t* sb = (uint8_t*)h->sel;
    unsigned long long* sel = (unsigned long long*)sb;
    uint32_t* hist = (uint32_t*)(sb + kSelHistAt);
    unsigned long long* certain_list = (unsigned long long*)(sb + kSelCertainAt);
    const AxSlice* slices = (const AxSlice*)(sb + kSelSlicesAt);
    const uint32_t ns = (uint32_t)h->spans.size();
    const bool timing = h->timing;
    for (hipEvent_t& e : h->qev)
        if (timing && !e) AX_HIP(h, hipEventCreate(&e));
    h->qtimed = false;

    const AxFilter flt{(unsigned long long)end_ts ^ kTdSign, (unsigned long long)key, (unsigned long long)val};
    AxSlice one{nullptr, nullptr, nullptr, nullptr, 0};  // the candidate list, once there is one
    // the passes' grids: y picks the slice, x covers the longest
    dim3 g_scan(ax_grid(longest), ns), g_hist(ax_grid(longest, std::max(1u, kAxHistGrid / ns)), ns),
        g_col(ax_grid((longest + kColItems - 1) / kColItems), ns);
    unsigned long long host[kSelWords];
    // pass 1 over the slices: how many match, and the bits in which their keys differ
    AX_HIP(h, hipMemsetAsync(sel, 0, kSelWords * 8, h->stream));
    if (timing) AX_HIP(h, hipEventRecord(h->qev[0], h->stream));
    AX_HIP(h, launch_checked("k_ax_scan", k_ax_scan, g_scan, dim3(kAxWG), 0, h->stream, slices, one, flt, sel));
    AX_HIP(h, hipMemcpyAsync(host, sel, sizeof host, hipMemcpyDeviceToHost, h->stream));
    AX_HIP(h, hipStreamSynchronize(h->stream));
    const uint64_t matched = host[kSelMatched];
    if (matched > total) return xfail(h, ZK_ERR_HIP, "the select counted more entries than the slices hold");
    uint64_t certain = 0, cand = matched, want = limit, copies = 0;
    IxEntry same{0, 0};
    int cur = -1;  // the list that holds the candidates; -1: they are still the slices'
    static thread_local std::vector<uint32_t> hh;
    hh.resize(kTdBins);
    while (matched && certain + cand > kAxCap) {
        const uint64_t diff_hi = host[kSelOrHi] & host[kSelNorHi], diff_lo = host[kSelOrLo] & host[kSelNorLo];
        if (!(diff_hi | diff_lo)) {
            // the candidates differ in no bit: they are all the pair their OR spells; `want` of them
            // end the answer (want <= limit - certain, and there are more than that many)
            same = IxEntry{~host[kSelOrHi], host[kSelOrLo]};
            copies = want;
            cand = 0;
            break;
        }
        const uint32_t shift = td_shift_of(diff_hi, diff_lo);
        AX_HIP(h, hipMemsetAsync(hist, 0, kTdBins * 4, h->stream));
        AX_HIP(h, launch_checked("k_ax_hist", k_ax_hist, g_hist, dim3(kAxWG), 0, h->stream, cur < 0 ? slices : nullptr, one, flt,
                                 shift, hist));
        AX_HIP(h, hipMemcpyAsync(hh.data(), hist, kTdBins * 4, hipMemcpyDeviceToHost, h->stream));
        AX_HIP(h, hipStreamSynchronize(h->stream));
        uint64_t below = 0;
        const uint32_t bin = td_pick_bin(hh.data(), want, &below);
        if (bin >= kTdBins || hh[bin] >= cand || below >= want)
            return xfail(h, ZK_ERR_HIP, "the select's histogram does not split its candidates");
        const uint64_t stay = hh[bin];
        const int dst = cur == 0 ? 1 : 0;
        if ((st = grow(h, &h->list[dst], &h->list_bytes[dst], (size_t)stay * sizeof(IxEntry),
                       "the select's candidate list (16 B per entry)")) != ZK_OK)
            return st;
        AX_HIP(h, hipMemsetAsync(sel + kSelOrHi, 0, (kSelCand + 1 - kSelOrHi) * 8, h->stream));
        AX_HIP(h, launch_checked("k_ax_collect", k_ax_collect, g_col, dim3(kAxWG), 0, h->stream, cur < 0 ? slices : nullptr, one, flt,
                                 shift, bin, sel, certain_list, (unsigned long long)kAxCap, (unsigned long long*)h->list[dst],
                                 (unsigned long long)stay));
        certain += below;
        want -= below;
        cand = stay;
        cur = dst;
        one = AxSlice{(const unsigned long long*)h->list[dst], nullptr, nullptr, nullptr, stay};
        g_hist = dim3(ax_grid(stay, kAxHistGrid), 1);
        g_col = dim3(ax_grid((stay + kColItems - 1) / kColItems), 1);
        if (certain + cand > kAxCap) {
            AX_HIP(h, hipMemcpyAsync(host, sel, sizeof host, hipMemcpyDeviceToHost, h->stream));
            AX_HIP(h, hipStreamSynchronize(h->stream));
        }
    }
    if (matched && cur < 0 && !copies) {
        // everything that matches fits the cap: one pass appends it all to the certain list
        AX_HIP(h, launch_checked("k_ax_collect", k_ax_collect, g_col, dim3(kAxWG), 0, h->stream, slices, one, flt, 0u, kTdBins, sel,
                                 certain_list, (unsigned long long)kAxCap, (unsigned long long*)nullptr, 0ull));
        certain = matched;
        cand = 0;
    }
    static thread_local std::vector<IxEntry> ent;
    ent.resize(certain + cand);
    if (certain) AX_HIP(h, hipMemcpyAsync(ent.data(), certain_list, certain * sizeof(IxEntry), hipMemcpyDeviceToHost, h->stream));
    if (cand)
        AX_HIP(h, hipMemcpyAsync(ent.data() + certain, h->list[cur], cand * sizeof(IxEntry), hipMemcpyDeviceToHost, h->stream));
    if (timing) AX_HIP(h, hipEventRecord(h->qev[1], h->stream));
    AX_HIP(h, hipStreamSynchronize(h->stream));
    h->qtimed = timing;
    *n_out = ix_emit(ent.data(), ent.size(), same, copies, limit, trace_id, ts);
    if (matched_out) *matched_out = matched;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_ax_query_ms(zk_ax* h, double* ms) {
    ZK_GUARD_BEGIN
    if (!h || !ms) return ZK_ERR_INVALID_ARG;
    if (!h->qtimed) return xfail(h, ZK_ERR_INVALID_ARG, "no timed query has run a pass (zk_ax_config.timing)");
    AX_HIP(h, hipSetDevice(h->device));
    float f = 0.f;
    AX_HIP(h, hipEventElapsedTime(&f, h->qev[0], h->qev[1]));
    *ms = f;
    return ZK_OK;
    ZK_GUARD_END
}

}  // extern "C"
