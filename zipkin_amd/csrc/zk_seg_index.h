// zk_seg_index.h — what the two segment indices share (zk_ix.hip: trace ids by service and span name,
// zk_ax.hip: trace ids by annotation), written once over a traits type T per index.
//
// A segment index holds entries grouped by service in HBM. One observe makes one SEGMENT: one allocation
// of columns, each 256-B aligned, the first tkey[u64] = ts ^ sign, the second tid[u64], with the entries of
// service s at [off[s], off[s + 1]); `off` lives on the host. At most T::MAX_SEGMENTS segments (the
// observe that would make one more first merges all into one) and 2^32 - 1 entries.
//
// Device side: the bodies of the merge and of the select's hist and collect passes (the expiry's are
// zk_expire.h's); the __global__ kernels, with their names, launch bounds and LDS, are the two files'. Host
// side: SegIndex<T>, the handle, and the seg_* procedures over it. T says only what differs: Slice, Filter,
// load (a service's entries in one segment, what a query takes of them), list and slice (the Slice of a 16-B
// entry list, of a segment's part), bytes_for, put (the expiry's copy of an entry), merge (the merge kernel's
// launch), the kernels scan, hist, collect, expire_count, expire_rewrite, MAX_SEGMENTS, MAX_LIMIT, EXTRA_SCRATCH
// (bytes behind the slices in the select's scratch) and the messages' wording MERGED, SURVIVORS, CONFIG.
//
// Every store is bounded: the scatter and the merge drop a place at or past the segment's size (it
// cannot arise while the columns stay as they were between the count and the scatter, which the headers
// ask of the caller; a caller that breaks it loses entries and corrupts nothing), the collect drops
// entries past its lists' capacities, the expiry's rewrite a place at or past the new segment's size.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "zk_expire.h"
#include "zk_hist.h"
#include "zk_ix_select.h"
#include "zk_launch.h"
#include "zkagg.h"

namespace zk {

constexpr int kSegWG = 256;
constexpr uint32_t kSegSvcBins = 4096;           // ZK_IX_MAX_SERVICES = ZK_AX_MAX_SERVICES
constexpr uint32_t kSegMaxGrid = 4096;
constexpr uint32_t kSegHistGrid = 1024;          // the count and hist kernels: every workgroup flushes up to 4096 bins
constexpr uint32_t kSegScatterPerWG = 16384;     // the scatter kernels: records per workgroup at least (S atomics each)
constexpr uint64_t kSegMaxEntries = 0xFFFFFFFFull;
constexpr int kCntItems = 4;                     // the counting loops: records per thread and step
constexpr uint32_t kCntTile = kSegWG * kCntItems;
static_assert(kExpBins == kSegSvcBins && kExpWG == kSegWG, "zk_expire.h's bins and workgroup are the indices'");

// the select's counters (those of zk_td.hip): matched, certain entries appended, then what a round
// zeroes: the OR of the keys and of their complements (hi, lo) over the entries that stay candidates,
// and their number
enum { kSelMatched = 0, kSelCertain = 1, kSelOrHi = 2, kSelNorHi = 3, kSelOrLo = 4, kSelNorLo = 5, kSelCand = 6, kSelWords = 8 };

// the observe's block: the counts, the cursors, then the range violations
constexpr size_t kObsCursorAt = kSegSvcBins * 4;
constexpr size_t kObsStatAt = 2 * kSegSvcBins * 4;
constexpr size_t kObsBytes = kObsStatAt + 64;

inline uint32_t seg_grid(uint64_t items, uint32_t cap = kSegMaxGrid) {
    const uint64_t g = (items + kSegWG - 1) / kSegWG;
    return (uint32_t)(g < 1 ? 1 : g > cap ? cap : g);
}

// ---- the merge -----------------------------------------------------------------------------------------
// One old segment's n_src entries into the merged one. src_off[S + 1]: the old segment's offsets;
// dst_base[S]: where its slice of each service begins in the merged segment; copy(i, at) copies entry i
// to place `at` (at < dst_total).
template <class Copy>
__device__ __forceinline__ void seg_merge(unsigned long long n_src, const unsigned long long* __restrict__ src_off,
                                          const unsigned long long* __restrict__ dst_base, uint32_t S,
                                          unsigned long long dst_total, const Copy& copy) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kSegWG;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kSegWG + threadIdx.x; i < n_src; i += stride) {
        // the last service whose offset is <= i (src_off[0] = 0 <= i < n_src = src_off[S]): the ones
        // behind it that share the offset are empty
        uint32_t a = 0, b = S;
        while (b - a > 1) {
            const uint32_t mid = (a + b) >> 1;
            if (src_off[mid] <= i) a = mid; else b = mid;
        }
        const unsigned long long at = dst_base[a] + (i - src_off[a]);
        if (at < dst_total) copy(i, at);
    }
}

// ---- the select ----------------------------------------------------------------------------------------
// trace_ids finds the first `limit` entries by the 128-bit key (hi = ~tkey, lo = traceId) without
// sorting, with the passes of zk_td.hip:
//   scan     over the service's slices: the filter (T::load reads the narrow columns first, the 16 B of tkey
//            and traceId only where they match), the number of matching entries and the OR of their keys and
//            of the keys' complements, whose AND is the set of bits in which the matching keys differ;
//   hist     a 4096-bin histogram of the 12-bit digit that starts at the highest differing bit (so the
//            bins always split the entries), per workgroup in LDS, flushed with atomics; td_digit is
//            below kTdBins for any key and shift: it indexes s_hist;
//   (host)   the bin in which the running count crosses the number still wanted;
//   collect  appends the entries below that bin to the CERTAIN list (they are in the answer) and the
//            entries in it to a CANDIDATE list of 16-B entries, and gathers the differing bits of the
//            candidates for the next round.
// The slices are so read three times at most (twice when everything that matches fits the host's cap).
// While certain + candidates exceed the cap the hist / collect pair repeats over the candidate list alone.
//
// TERMINATION. Entries here may be equal in all 128 bits, so "the candidates differ in some bit" is not
// given. Every round either SPLITS the list or ENDS the select: when the candidates differ in some bit,
// the digit's top bit is the highest such bit, both of its values occur, so at least two bins are
// occupied and the chosen bin holds fewer entries than the list did (the list strictly shrinks, and the
// next round's differing bits lie below this round's digit: at most 11 rounds consume the 128 bits);
// when they differ in no bit they are all one pair (it is the OR of their keys), the call takes as
// many copies of it as are still wanted and stops.
//
// A grid's y index picks the slice; a list is the one slice passed by value: the kernels choose, the
// bodies get the slice `sl`. The scan's short loop is spelled in k_ix_scan and k_ax_scan, and the bodies here
// are __forceinline__: so every kernel keeps the registers it had (profiles/seg_index/kernel_resources.txt).
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

// s_hist: kTdBins words of LDS
template <class T>
__device__ __forceinline__ void seg_hist(const typename T::Slice& sl, const typename T::Filter& flt, uint32_t shift,
                                         uint32_t* __restrict__ hist, uint32_t* s_hist) {
    for (uint32_t b = threadIdx.x; b < kTdBins; b += kSegWG) s_hist[b] = 0u;
    __syncthreads();
    const unsigned long long stride = (unsigned long long)gridDim.x * kSegWG;
    for (unsigned long long base = (unsigned long long)blockIdx.x * kSegWG; base < sl.count; base += stride) {
        IxEntry e{0, 0};
        const bool ok = T::load(sl, base + threadIdx.x, flt, &e);
        hist_add(s_hist, ok, td_digit(~e.tkey, e.id, shift));
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kTdBins; b += kSegWG) {
        const uint32_t c = s_hist[b];
        if (c) atomicAdd(&hist[b], c);
    }
}

// digit < bin: certain; digit == bin: a candidate (bin = kTdBins: every matching entry is certain).
// A workgroup walks tiles of kColTile entries of its slice, kColItems per thread; each wave ranks its
// takers of both kinds with ballots, the workgroup sums its waves' counts in LDS and one thread per
// list draws the tile's stretch with a returning atomicAdd (zk_td.hip's k_td_collect). The loop's bounds
// are the same for all threads of a workgroup, so every lane reaches the ballots and the barriers.
constexpr int kColItems = 4;
constexpr uint32_t kColTile = kSegWG * kColItems;
constexpr int kColWaves = kSegWG / 64;

__device__ inline void put_entry(unsigned long long* __restrict__ out, unsigned long long cap, unsigned long long at,
                                 const IxEntry& e) {
    if (at < cap) {
        out[2 * at] = e.tkey;
        out[2 * at + 1] = e.id;
    }
}

// s_cnt, s_base: the workgroup's LDS, the waves' takers of each kind and where the tile's stretches begin
template <class T>
__device__ __forceinline__ void seg_collect(const typename T::Slice& sl, const typename T::Filter& flt, uint32_t shift,
                                            uint32_t bin, unsigned long long* __restrict__ sel, unsigned long long* __restrict__ certain,
                                            unsigned long long certain_cap, unsigned long long* __restrict__ cand,
                                            unsigned long long cand_cap, uint32_t (*s_cnt)[kColWaves], unsigned long long* s_base) {
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
            const bool ok = T::load(sl, tile + (unsigned long long)j * kSegWG + threadIdx.x, flt, &e[j]);
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

// ---- the handle ----------------------------------------------------------------------------------------
// one segment: its columns lie one behind the other in `block`, each col8(n) bytes apart
struct Segment {
    void* block = nullptr;
    size_t bytes = 0;
    uint64_t n = 0;
    std::vector<uint64_t> off;  // num_services + 1

    static size_t col8(uint64_t n) { return (size_t)((n * 8 + 255) / 256 * 256); }
    unsigned long long* col(int c) const { return (unsigned long long*)((uint8_t*)block + (size_t)c * col8(n)); }
    unsigned long long* tkey() const { return col(0); }
    unsigned long long* tid() const { return col(1); }
};

template <class F>
struct SegKernel {  // a kernel and the name launch_checked reports it under
    const char* name;
    F* fn;
};

template <class T>
struct SegIndex {
    // byte offsets in the select's scratch block
    static constexpr uint32_t kCap = T::MAX_LIMIT;  // the most entries the select brings to the host
    static constexpr size_t kSelHistAt = 256;
    static constexpr size_t kSelCertainAt = kSelHistAt + kTdBins * 4;
    static constexpr size_t kSelSlicesAt = kSelCertainAt + (size_t)kCap * sizeof(IxEntry);
    static constexpr size_t kSelExtraAt = kSelSlicesAt + T::MAX_SEGMENTS * sizeof(typename T::Slice);
    static constexpr size_t kSelBytes = kSelExtraAt + T::EXTRA_SCRATCH;
    static_assert(sizeof(IxEntry) == 16 && sizeof(typename T::Slice) % 8 == 0, "entry and slice layouts");
    static_assert(kSelWords * 8 <= kSelHistAt && kSelCertainAt % 16 == 0 && kSelSlicesAt % 8 == 0 && kSelExtraAt % 4 == 0,
                  "the scratch block's layout");

    int device = 0;
    uint32_t S = 0;
    hipStream_t stream = nullptr, own = nullptr;
    bool timing = false;
    std::vector<Segment> segs;
    std::vector<uint64_t> svc_count;    // entries per service
    uint64_t entries = 0;
    void* obs = nullptr;                // the observe's counts, cursors and range violations (kObsBytes)
    void* stage = nullptr;              // the columns of a host batch
    void* mplan = nullptr;              // a merge's offsets and bases, per old segment
    void* xplan = nullptr;              // an expiry's segments, offsets, work items, survivor counts and cursors
    void* sel = nullptr;                // the select's counters, histogram, certain list, slices, T's extra (kSelBytes)
    void* list[2] = {nullptr, nullptr}; // the candidate lists, written in turn
    size_t stage_bytes = 0, mplan_bytes = 0, xplan_bytes = 0, sel_bytes = 0, list_bytes[2] = {0, 0};
    std::vector<uint32_t> counts_host, cursor_host;  // (a queued copy reads cursor_host: it changes only behind a synchronisation)
    std::vector<uint64_t> mplan_host;
    std::vector<uint8_t> xplan_host;                 // (an expiry's queued copies read these three: likewise)
    std::vector<uint32_t> xsurv_host, xcursor_host;
    std::vector<ExpItem> xitems_host;
    std::vector<typename T::Slice> slices_host;
    std::vector<IxSpan> spans;
    hipEvent_t oev[4] = {};  // around the passes of the last observe (observe_ms)
    hipEvent_t qev[2] = {};  // around the last query (query_ms)
    hipEvent_t xev[4] = {};  // around the passes of the last expiry (expire_ms)
    bool otimed = false, qtimed = false, xtimed = false;
    std::string err;
};

template <class T>
zk_status seg_fail(SegIndex<T>* h, zk_status s, const std::string& m) {
    if (h) h->err = m;
    return s;
}

// a failed HIP call: ZK_ERR_HIP or ZK_ERR_CAPACITY, the message the call as written (a launch: the kernel's name)
#define ZK_SEG_TRY(h, call, what)                                                                  \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess) return seg_fail(h, is_refusal(_e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP,    \
                                              std::string(what) + ": " + launch_error_str(_e));    \
    } while (0)
#define ZK_SEG_HIP(h, call) ZK_SEG_TRY(h, call, #call)
#define ZK_SEG_LAUNCH(h, k, ...) ZK_SEG_TRY(h, launch_checked((k).name, (k).fn, __VA_ARGS__), (k).name)

// a fresh block of `need` bytes; a refused allocation is ZK_ERR_CAPACITY
template <class T>
zk_status seg_alloc(SegIndex<T>* h, void** p, size_t need, const char* what) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, need ? need : 8);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (e != hipErrorOutOfMemory) return seg_fail(h, ZK_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        return seg_fail(h, ZK_ERR_CAPACITY, std::string("no device memory for ") + what);
    }
    *p = q;
    return ZK_OK;
}

// at least `need` bytes behind *p: a larger block first, then the old one freed (its content is not
// kept); a refused allocation leaves *p as it was
template <class T>
zk_status seg_grow(SegIndex<T>* h, void** p, size_t* have, size_t need, const char* what) {
    if (need <= *have && *p) return ZK_OK;
    void* q = nullptr;
    const zk_status st = seg_alloc(h, &q, need, what);
    if (st != ZK_OK) return st;
    if (*p) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(*p);
    }
    *p = q;
    *have = need;
    return ZK_OK;
}

template <class T>
void seg_free(SegIndex<T>* h) {
    if (!h->segs.empty()) (void)hipStreamSynchronize(h->stream);
    for (Segment& g : h->segs)
        if (g.block) (void)hipFree(g.block);
    h->segs.clear();
}

// All segments into one: each service's slices concatenated in segment order. Anything refused leaves
// the index as it was. Synchronises.
template <class T>
zk_status seg_merge_all(SegIndex<T>* h) {
    const uint32_t S = h->S, G = (uint32_t)h->segs.size();
    if (G < 2) return ZK_OK;
    Segment m;
    m.n = h->entries;
    m.off.assign(S + 1, 0);
    for (uint32_t s = 0; s < S; ++s) m.off[s + 1] = m.off[s] + h->svc_count[s];
    if (m.off[S] != m.n) return seg_fail(h, ZK_ERR_HIP, "the segments' offsets do not add up");
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
    zk_status st = seg_grow(h, &h->mplan, &h->mplan_bytes, per * G * 8, "a merge's offsets");
    if (st != ZK_OK) return st;
    m.bytes = T::bytes_for(m.n);
    if ((st = seg_alloc(h, &m.block, m.bytes, T::MERGED)) != ZK_OK) return st;
    hipError_t e = hipMemcpyAsync(h->mplan, h->mplan_host.data(), per * G * 8, hipMemcpyHostToDevice, h->stream);
    for (uint32_t g = 0; g < G && e == hipSuccess; ++g)
        e = T::merge(h->stream, h->segs[g], (const unsigned long long*)h->mplan + per * g, S, m);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(m.block);
        return seg_fail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("merging the segments: ") + launch_error_str(e));
    }
    seg_free(h);
    h->segs.push_back(std::move(m));
    return ZK_OK;
}

// The asked service's slices into the scratch block (and h->spans); *total = the entries they hold,
// *longest = those of the longest.
template <class T>
zk_status seg_plan(SegIndex<T>* h, uint32_t service, uint64_t* total, uint64_t* longest) {
    std::vector<const uint64_t*> offs(h->segs.size());
    for (size_t g = 0; g < h->segs.size(); ++g) offs[g] = h->segs[g].off.data();
    *total = ix_plan(offs.data(), (uint32_t)offs.size(), service, &h->spans);
    *longest = 0;
    if (!*total) return ZK_OK;
    zk_status st = seg_grow(h, &h->sel, &h->sel_bytes, SegIndex<T>::kSelBytes, "the select's counters and lists");
    if (st != ZK_OK) return st;
    h->slices_host.clear();
    for (const IxSpan& sp : h->spans) {
        h->slices_host.push_back(T::slice(h->segs[sp.segment], sp.start, sp.count));
        if (sp.count > *longest) *longest = sp.count;
    }
    ZK_SEG_HIP(h, hipMemcpyAsync((uint8_t*)h->sel + SegIndex<T>::kSelSlicesAt, h->slices_host.data(),
                                 h->slices_host.size() * sizeof(typename T::Slice), hipMemcpyHostToDevice, h->stream));
    return ZK_OK;
}

// The expiry behind its argument checks: every entry with tkey < cut goes. The count pass over all
// segments, the one synchronisation that sizes the rest, then the segments sorted into untouched (no
// entry goes: not read again), gone (every entry goes: freed) and mixed (their survivors rewritten into
// ONE new segment, which takes the place of the first of them). An entry's service comes from its place
// in its segment, resolved once per workgroup (zk_expire.h), not searched per entry as in the merge.
// Nothing is freed and no bookkeeping changes before the new segment is complete; anything refused
// leaves the index as it was.
template <class T>
zk_status seg_expire(SegIndex<T>* h, int64_t min_ts, uint64_t* removed_out) {
    if (removed_out) *removed_out = 0;
    h->xtimed = false;
    if (h->segs.empty()) return ZK_OK;
    ZK_SEG_HIP(h, hipSetDevice(h->device));
    const unsigned long long cut = (unsigned long long)min_ts ^ kTdSign;
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
    zk_status st = seg_grow(h, &h->xplan, &h->xplan_bytes, cur_at + al((size_t)S * 4), "an expiry's plan");
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
        if (timing && !e) ZK_SEG_HIP(h, hipEventCreate(&e));
    ZK_SEG_HIP(h, hipMemcpyAsync(xp, h->xplan_host.data(), surv_at, hipMemcpyHostToDevice, h->stream));
    ZK_SEG_HIP(h, hipMemsetAsync(surv, 0, (size_t)G * S * 4, h->stream));
    if (timing) ZK_SEG_HIP(h, hipEventRecord(h->xev[0], h->stream));
    ZK_SEG_LAUNCH(h, T::expire_count, dim3(W), dim3(kExpWG), 0, h->stream, segs, items, (unsigned long long)chunk, S, cut, surv);
    if (timing) ZK_SEG_HIP(h, hipEventRecord(h->xev[1], h->stream));
    h->xsurv_host.resize((size_t)G * S);
    ZK_SEG_HIP(h, hipMemcpyAsync(h->xsurv_host.data(), surv, (size_t)G * S * 4, hipMemcpyDeviceToHost, h->stream));
    ZK_SEG_HIP(h, hipStreamSynchronize(h->stream));  // the sizing synchronisation
    std::vector<uint64_t> keep(G, 0), gone(S, 0);
    std::vector<uint32_t> mixed;
    uint64_t removed = 0;
    for (uint32_t g = 0; g < G; ++g) {
        const Segment& sg = h->segs[g];
        for (uint32_t s = 0; s < S; ++s) {
            const uint64_t len = sg.off[s + 1] - sg.off[s], c = h->xsurv_host[(size_t)g * S + s];
            if (c > len) return seg_fail(h, ZK_ERR_HIP, "the expiry counted more survivors than a slice holds");
            keep[g] += c;
            gone[s] += len - c;
        }
        removed += sg.n - keep[g];
        if (keep[g] != 0 && keep[g] != sg.n) mixed.push_back(g);
    }
    if (removed == 0) {  // nothing goes: nothing is rewritten, reallocated or freed
        if (timing) ZK_SEG_HIP(h, hipEventRecord(h->xev[2], h->stream));
        if (timing) ZK_SEG_HIP(h, hipEventRecord(h->xev[3], h->stream));
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
        m.bytes = T::bytes_for(m.n);
        if ((st = seg_alloc(h, &m.block, m.bytes, T::SURVIVORS)) != ZK_OK) return st;
        h->xcursor_host.resize(S);
        for (uint32_t s = 0; s < S; ++s) h->xcursor_host[s] = (uint32_t)m.off[s];
        h->xitems_host.resize(W);  // (filled by index, not one push_back call per item; W bounds their number)
        uint32_t nx = 0;
        for (uint32_t g : mixed)
            for (uint64_t c = 0; c * chunk < h->segs[g].n; ++c) h->xitems_host[nx++] = ExpItem{g, (uint32_t)c};
        h->xitems_host.resize(nx);
    }
    hipError_t e = hipSuccess;
    if (!mixed.empty()) {
        e = hipMemcpyAsync(xp + item_at, h->xitems_host.data(), h->xitems_host.size() * sizeof(ExpItem), hipMemcpyHostToDevice,
                           h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cursor, h->xcursor_host.data(), (size_t)S * 4, hipMemcpyHostToDevice, h->stream);
    }
    if (e == hipSuccess && timing) e = hipEventRecord(h->xev[2], h->stream);
    if (e == hipSuccess && !mixed.empty())
        e = launch_checked(T::expire_rewrite.name, T::expire_rewrite.fn, dim3((uint32_t)h->xitems_host.size()), dim3(kExpWG), 0,
                           h->stream, segs, items, (unsigned long long)chunk, S, cut, cursor, (unsigned long long)m.n, T::put(m));
    if (e == hipSuccess && timing) e = hipEventRecord(h->xev[3], h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        if (m.block) (void)hipFree(m.block);
        return seg_fail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("rewriting the survivors: ") + launch_error_str(e));
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

// The select's driver, behind the query's argument checks (service < S, 1 <= limit <= T::MAX_LIMIT, the
// outputs not null): the first `limit` of the service's entries that flt takes, by the 128-bit key.
template <class T>
zk_status seg_trace_ids(SegIndex<T>* h, uint32_t service, const typename T::Filter& flt, uint32_t limit, uint64_t* trace_id,
                    int64_t* ts, uint32_t* n_out, uint64_t* matched_out) {
    using Slice = typename T::Slice;
    using H = SegIndex<T>;
    constexpr uint32_t kCap = H::kCap;
    *n_out = 0;
    if (matched_out) *matched_out = 0;
    if (h->svc_count[service] == 0) return ZK_OK;
    ZK_SEG_HIP(h, hipSetDevice(h->device));
    uint64_t total = 0, longest = 0;
    zk_status st = seg_plan(h, service, &total, &longest);
    if (st != ZK_OK) return st;
    if (!total) return ZK_OK;
    uint8_t* sb = (uint8_t*)h->sel;
    unsigned long long* sel = (unsigned long long*)sb;
    uint32_t* hist = (uint32_t*)(sb + H::kSelHistAt);
    unsigned long long* certain_list = (unsigned long long*)(sb + H::kSelCertainAt);
    const Slice* slices = (const Slice*)(sb + H::kSelSlicesAt);
    const uint32_t ns = (uint32_t)h->spans.size();
    const bool timing = h->timing;
    for (hipEvent_t& e : h->qev)
        if (timing && !e) ZK_SEG_HIP(h, hipEventCreate(&e));
    h->qtimed = false;

    Slice one = T::list(nullptr, 0);  // the candidate list, once there is one
    // the passes' grids: y picks the slice, x covers the longest
    dim3 g_scan(seg_grid(longest), ns), g_hist(seg_grid(longest, std::max(1u, kSegHistGrid / ns)), ns),
        g_col(seg_grid((longest + kColItems - 1) / kColItems), ns);
    unsigned long long host[kSelWords];
    // pass 1 over the slices: how many match, and the bits in which their keys differ
    ZK_SEG_HIP(h, hipMemsetAsync(sel, 0, kSelWords * 8, h->stream));
    if (timing) ZK_SEG_HIP(h, hipEventRecord(h->qev[0], h->stream));
    ZK_SEG_LAUNCH(h, T::scan, g_scan, dim3(kSegWG), 0, h->stream, slices, one, flt, sel);
    ZK_SEG_HIP(h, hipMemcpyAsync(host, sel, sizeof host, hipMemcpyDeviceToHost, h->stream));
    ZK_SEG_HIP(h, hipStreamSynchronize(h->stream));
    const uint64_t matched = host[kSelMatched];
    if (matched > total) return seg_fail(h, ZK_ERR_HIP, "the select counted more entries than the slices hold");
    uint64_t certain = 0, cand = matched, want = limit, copies = 0;
    IxEntry same{0, 0};
    int cur = -1;  // the list that holds the candidates; -1: they are still the slices'
    static thread_local std::vector<uint32_t> hh;
    hh.resize(kTdBins);
    while (matched && certain + cand > kCap) {
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
        ZK_SEG_HIP(h, hipMemsetAsync(hist, 0, kTdBins * 4, h->stream));
        ZK_SEG_LAUNCH(h, T::hist, g_hist, dim3(kSegWG), 0, h->stream, cur < 0 ? slices : nullptr, one, flt, shift, hist);
        ZK_SEG_HIP(h, hipMemcpyAsync(hh.data(), hist, kTdBins * 4, hipMemcpyDeviceToHost, h->stream));
        ZK_SEG_HIP(h, hipStreamSynchronize(h->stream));
        uint64_t below = 0;
        const uint32_t bin = td_pick_bin(hh.data(), want, &below);
        if (bin >= kTdBins || hh[bin] >= cand || below >= want)
            return seg_fail(h, ZK_ERR_HIP, "the select's histogram does not split its candidates");
        const uint64_t stay = hh[bin];
        const int dst = cur == 0 ? 1 : 0;
        if ((st = seg_grow(h, &h->list[dst], &h->list_bytes[dst], (size_t)stay * sizeof(IxEntry),
                       "the select's candidate list (16 B per entry)")) != ZK_OK)
            return st;
        ZK_SEG_HIP(h, hipMemsetAsync(sel + kSelOrHi, 0, (kSelCand + 1 - kSelOrHi) * 8, h->stream));
        ZK_SEG_LAUNCH(h, T::collect, g_col, dim3(kSegWG), 0, h->stream, cur < 0 ? slices : nullptr, one, flt, shift, bin, sel,
                      certain_list, (unsigned long long)kCap, (unsigned long long*)h->list[dst], (unsigned long long)stay);
        certain += below;
        want -= below;
        cand = stay;
        cur = dst;
        one = T::list((const unsigned long long*)h->list[dst], stay);
        g_hist = dim3(seg_grid(stay, kSegHistGrid), 1);
        g_col = dim3(seg_grid((stay + kColItems - 1) / kColItems), 1);
        if (certain + cand > kCap) {
            ZK_SEG_HIP(h, hipMemcpyAsync(host, sel, sizeof host, hipMemcpyDeviceToHost, h->stream));
            ZK_SEG_HIP(h, hipStreamSynchronize(h->stream));
        }
    }
    if (matched && cur < 0 && !copies) {
        // everything that matches fits the cap: one pass appends it all to the certain list
        ZK_SEG_LAUNCH(h, T::collect, g_col, dim3(kSegWG), 0, h->stream, slices, one, flt, 0u, kTdBins, sel, certain_list,
                      (unsigned long long)kCap, (unsigned long long*)nullptr, 0ull);
        certain = matched;
        cand = 0;
    }
    static thread_local std::vector<IxEntry> ent;
    ent.resize(certain + cand);
    if (certain) ZK_SEG_HIP(h, hipMemcpyAsync(ent.data(), certain_list, certain * sizeof(IxEntry), hipMemcpyDeviceToHost, h->stream));
    if (cand)
        ZK_SEG_HIP(h, hipMemcpyAsync(ent.data() + certain, h->list[cur], cand * sizeof(IxEntry), hipMemcpyDeviceToHost, h->stream));
    if (timing) ZK_SEG_HIP(h, hipEventRecord(h->qev[1], h->stream));
    ZK_SEG_HIP(h, hipStreamSynchronize(h->stream));
    h->qtimed = timing;
    *n_out = ix_emit(ent.data(), ent.size(), same, copies, limit, trace_id, ts);
    if (matched_out) *matched_out = matched;
    return ZK_OK;
}

// ---- the small calls -----------------------------------------------------------------------------------
template <class T>
zk_status seg_reset(SegIndex<T>* h) {
    if (h->segs.empty()) return ZK_OK;
    ZK_SEG_HIP(h, hipSetDevice(h->device));
    seg_free(h);
    h->svc_count.assign(h->S, 0);
    h->entries = 0;
    return ZK_OK;
}

template <class T>
zk_status seg_compact(SegIndex<T>* h) {
    if (h->segs.size() < 2) return ZK_OK;
    ZK_SEG_HIP(h, hipSetDevice(h->device));
    return seg_merge_all(h);
}

template <class T>
zk_status seg_info(SegIndex<T>* h, uint64_t* entries, uint64_t* segments, uint64_t* bytes) {
    if (!h->segs.empty()) {
        ZK_SEG_HIP(h, hipSetDevice(h->device));
        ZK_SEG_HIP(h, hipStreamSynchronize(h->stream));
    }
    uint64_t b = 0;
    for (const Segment& g : h->segs) b += g.bytes;
    if (entries) *entries = h->entries;
    if (segments) *segments = h->segs.size();
    if (bytes) *bytes = b;
    return ZK_OK;
}

template <class T>  // the three intervals between the four events of the last timed observe or expiry
zk_status seg_passes_ms(SegIndex<T>* h, bool timed, const hipEvent_t* ev, const char* none, double out[3]) {
    if (!timed) return seg_fail(h, ZK_ERR_INVALID_ARG, std::string(none) + " (" + T::CONFIG + ".timing)");
    ZK_SEG_HIP(h, hipSetDevice(h->device));
    ZK_SEG_HIP(h, hipEventSynchronize(ev[3]));
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        ZK_SEG_HIP(h, hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
        out[k] = ms;
    }
    return ZK_OK;
}

template <class T>
zk_status seg_query_ms(SegIndex<T>* h, double* ms) {
    if (!h->qtimed) return seg_fail(h, ZK_ERR_INVALID_ARG, std::string("no timed query has run a pass (") + T::CONFIG + ".timing)");
    ZK_SEG_HIP(h, hipSetDevice(h->device));
    float f = 0.f;
    ZK_SEG_HIP(h, hipEventElapsedTime(&f, h->qev[0], h->qev[1]));
    *ms = f;
    return ZK_OK;
}

// ---- create and destroy --------------------------------------------------------------------------------
// a handle H (a SegIndex) on `device`, which must be there and a gfx950, over the caller's stream or its own
template <class H>
zk_status seg_create(int device, uint32_t S, bool timing, void* stream, H** out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || device < 0 || device >= ndev) return ZK_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ZK_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return ZK_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return ZK_ERR_HIP;
    H* h = new H();
    h->device = device;
    h->S = S;
    h->timing = timing;
    h->svc_count.assign(h->S, 0);
    if (!stream && hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return ZK_ERR_HIP;
    }
    h->stream = stream ? (hipStream_t)stream : h->own;
    *out = h;
    return ZK_OK;
}

template <class H>
zk_status seg_destroy(H* h) {
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    seg_free(h);
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
}

}  // namespace zk
