// zk_ax.hip — the trace-id index by annotation (include/zkannindex.h): what is this index's own of the
// segment index of zk_seg_index.h, where segments, merge, select, expiry and the handle are. A segment has
// four columns, tkey[u64] = ts ^ sign, tid[u64], key[u64], val[u64]: 32 B per entry. Here: the traits,
// k_ax_count and k_ax_scatter with zk_ax_observe, the kernels that give the shared bodies their names, and
// the C functions' argument checks.
#include "zk_guard.h"
#include "zk_seg_index.h"
#include "zkannindex.h"

namespace zk {
namespace {

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
static_assert(sizeof(AxSlice) == 40, "slice layout");

// the four columns of a segment: p + c * stride (in words)
struct AxCols {
    unsigned long long* p;
    unsigned long long stride;
};
AxCols ax_cols(const Segment& g) { return AxCols{g.col(0), (unsigned long long)(Segment::col8(g.n) / 8)}; }

// an old segment's entry into the expiry's new one: tid, key and val lie behind tkey; 32 B written
struct AxPut {
    AxCols dst;
    __device__ void operator()(const ExpSeg& sg, unsigned long long i, unsigned long long k, unsigned long long at) const {
        const unsigned long long col = (sg.n * 8ull + 255ull) / 256ull * 32ull;  // a column, in words
        dst.p[at] = k;
#pragma unroll
        for (int c = 1; c < 4; ++c) dst.p[c * dst.stride + at] = sg.tkey[c * col + i];
    }
};

// the entry's columns and the filter (the device side of the traits)
struct AxLayout {
    using Slice = AxSlice;
    using Filter = AxFilter;
    __device__ static bool load(const AxSlice& s, unsigned long long i, const AxFilter& f, IxEntry* e) {
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
    static AxSlice list(const unsigned long long* p, unsigned long long n) { return AxSlice{p, nullptr, nullptr, nullptr, n}; }
    static AxSlice slice(const Segment& g, uint64_t start, uint64_t n) {
        return AxSlice{g.col(0) + start, g.col(1) + start, g.col(2) + start, g.col(3) + start, n};
    }
    static size_t bytes_for(uint64_t n) { return 4 * Segment::col8(n); }
    static AxPut put(const Segment& g) { return AxPut{ax_cols(g)}; }
};

// ---- observe -------------------------------------------------------------------------------------------
// counts[s] += the entries of service s (s < S); stat[0] += the entries with s >= S. The loop's bounds
// are the same for all threads of a workgroup, so every lane reaches the ballots.
__global__ __launch_bounds__(kSegWG) void k_ax_count(const uint32_t* __restrict__ svc, unsigned long long n, uint32_t S,
                                                     uint32_t* __restrict__ counts, unsigned long long* __restrict__ stat) {
    __shared__ uint32_t s_hist[kSegSvcBins];
    __shared__ uint32_t s_bad;
    for (uint32_t b = threadIdx.x; b < kSegSvcBins; b += kSegWG) s_hist[b] = 0u;
    if (threadIdx.x == 0) s_bad = 0u;
    __syncthreads();
    const unsigned long long stride = (unsigned long long)gridDim.x * kCntTile;
    for (unsigned long long base = (unsigned long long)blockIdx.x * kCntTile; base < n; base += stride) {
        uint32_t s[kCntItems];  // (the tile's loads first, then the ballots)
#pragma unroll
        for (int j = 0; j < kCntItems; ++j) {
            const unsigned long long i = base + (unsigned long long)j * kSegWG + threadIdx.x;
            s[j] = i < n ? svc[i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kCntItems; ++j) {
            const bool valid = base + (unsigned long long)j * kSegWG + threadIdx.x < n;
            if (valid && s[j] >= S) atomicAdd(&s_bad, 1u);
            hist_add(s_hist, valid && s[j] < S, s[j]);
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kSegSvcBins; b += kSegWG) {
        const uint32_t c = s_hist[b];
        if (c && b < S) atomicAdd(&counts[b], c);
    }
    if (threadIdx.x == 0 && s_bad) atomicAdd(&stat[0], (unsigned long long)s_bad);
}

// Workgroup b owns entries [b * chunk, (b + 1) * chunk) (chunk a multiple of the workgroup). cursor[s]
// starts at the segment's off[s]; `total` is the segment's size. hist_add and hist_rank index LDS with
// the service only under s < S <= kSegSvcBins.
__global__ __launch_bounds__(kSegWG) void k_ax_scatter(const uint32_t* __restrict__ svc, const unsigned long long* __restrict__ key,
                                                       const unsigned long long* __restrict__ val, const long long* __restrict__ ts,
                                                       const unsigned long long* __restrict__ tid, unsigned long long n,
                                                       unsigned long long chunk, uint32_t S, uint32_t* __restrict__ cursor,
                                                       unsigned long long total, unsigned long long* __restrict__ out_tkey,
                                                       unsigned long long* __restrict__ out_tid, unsigned long long* __restrict__ out_key,
                                                       unsigned long long* __restrict__ out_val) {
    __shared__ uint32_t s_cnt[kSegSvcBins];   // the stretch's entries per service, then the ranks given out
    __shared__ uint32_t s_base[kSegSvcBins];  // where the workgroup's places of a service begin
    const unsigned long long lo = (unsigned long long)blockIdx.x * chunk;
    const unsigned long long hi = lo + chunk < n ? lo + chunk : n;
    for (uint32_t b = threadIdx.x; b < kSegSvcBins; b += kSegWG) s_cnt[b] = 0u;
    __syncthreads();
    for (unsigned long long base = lo; base < hi; base += kCntTile) {
        uint32_t s[kCntItems];
#pragma unroll
        for (int j = 0; j < kCntItems; ++j) {
            const unsigned long long i = base + (unsigned long long)j * kSegWG + threadIdx.x;
            s[j] = i < hi ? svc[i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kCntItems; ++j)
            hist_add(s_cnt, base + (unsigned long long)j * kSegWG + threadIdx.x < hi && s[j] < S, s[j]);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kSegSvcBins; b += kSegWG) {
        const uint32_t c = s_cnt[b];
        if (c && b < S) s_base[b] = atomicAdd(&cursor[b], c);
        s_cnt[b] = 0u;
    }
    __syncthreads();
    for (unsigned long long base = lo; base < hi; base += kSegWG) {
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

// ---- the wrappers of zk_seg_index.h's and zk_expire.h's bodies -----------------------------------------
__global__ __launch_bounds__(kSegWG) void k_ax_merge(AxCols src, unsigned long long n_src, const unsigned long long* __restrict__ src_off,
                                                     const unsigned long long* __restrict__ dst_base, uint32_t S, AxCols dst,
                                                     unsigned long long dst_total) {
    seg_merge(n_src, src_off, dst_base, S, dst_total, [&](unsigned long long i, unsigned long long at) {
#pragma unroll
        for (int c = 0; c < 4; ++c) dst.p[c * dst.stride + at] = src.p[c * src.stride + i];
    });
}

__global__ __launch_bounds__(kSegWG) void k_ax_scan(const AxSlice* __restrict__ slices, AxSlice one, AxFilter flt,
                                                    unsigned long long* __restrict__ sel) {
    const AxSlice sl = slices ? slices[blockIdx.y] : one;
    const unsigned long long stride = (unsigned long long)gridDim.x * kSegWG;
    unsigned long long or_hi = 0, nor_hi = 0, or_lo = 0, nor_lo = 0, cnt = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kSegWG + threadIdx.x; i < sl.count; i += stride) {
        IxEntry e;
        if (!AxLayout::load(sl, i, flt, &e)) continue;
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

__global__ __launch_bounds__(kSegWG) void k_ax_hist(const AxSlice* __restrict__ slices, AxSlice one, AxFilter flt, uint32_t shift,
                                                    uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[kTdBins];
    const AxSlice sl = slices ? slices[blockIdx.y] : one;
    seg_hist<AxLayout>(sl, flt, shift, hist, s_hist);
}

__global__ __launch_bounds__(kSegWG) void k_ax_collect(const AxSlice* __restrict__ slices, AxSlice one, AxFilter flt, uint32_t shift,
                                                       uint32_t bin, unsigned long long* __restrict__ sel,
                                                       unsigned long long* __restrict__ certain, unsigned long long certain_cap,
                                                       unsigned long long* __restrict__ cand, unsigned long long cand_cap) {
    __shared__ uint32_t s_cnt[2][kColWaves];
    __shared__ unsigned long long s_base[2];
    const AxSlice sl = slices ? slices[blockIdx.y] : one;
    seg_collect<AxLayout>(sl, flt, shift, bin, sel, certain, certain_cap, cand, cand_cap, s_cnt, s_base);
}

__global__ __launch_bounds__(kExpWG) void k_ax_expire_count(const ExpSeg* __restrict__ segs, const ExpItem* __restrict__ items,
                                                            unsigned long long chunk, uint32_t S, unsigned long long cut,
                                                            uint32_t* __restrict__ surv) {
    __shared__ ExpLds lds;
    exp_count(segs, items, chunk, S, cut, surv, &lds);
}

__global__ __launch_bounds__(kExpWG) void k_ax_expire_rewrite(const ExpSeg* __restrict__ segs, const ExpItem* __restrict__ items,
                                                              unsigned long long chunk, uint32_t S, unsigned long long cut,
                                                              uint32_t* __restrict__ cursor, unsigned long long total, AxPut put) {
    __shared__ ExpLds lds;
    __shared__ uint32_t s_base[kExpBins];
    exp_rewrite(segs, items, chunk, S, cut, cursor, total, put, &lds, s_base);
}

// the host side of the traits: the limits, the kernels, the wording
struct AxTraits : AxLayout {
    static constexpr uint32_t MAX_SEGMENTS = ZK_AX_MAX_SEGMENTS, MAX_LIMIT = ZK_AX_MAX_LIMIT;
    static_assert(ZK_AX_MAX_SERVICES == kSegSvcBins, "the shared kernels' bins");
    static constexpr size_t EXTRA_SCRATCH = 0;
    static constexpr const char* MERGED = "the merged segment (32 B per entry)";
    static constexpr const char* SURVIVORS = "the survivors' segment (32 B per entry)";
    static constexpr const char* CONFIG = "zk_ax_config";
    static constexpr SegKernel<decltype(k_ax_scan)> scan{"k_ax_scan", k_ax_scan};
    static constexpr SegKernel<decltype(k_ax_hist)> hist{"k_ax_hist", k_ax_hist};
    static constexpr SegKernel<decltype(k_ax_collect)> collect{"k_ax_collect", k_ax_collect};
    static constexpr SegKernel<decltype(k_ax_expire_count)> expire_count{"k_ax_expire_count", k_ax_expire_count};
    static constexpr SegKernel<decltype(k_ax_expire_rewrite)> expire_rewrite{"k_ax_expire_rewrite", k_ax_expire_rewrite};

    static hipError_t merge(hipStream_t stream, const Segment& sg, const unsigned long long* plan, uint32_t S, const Segment& m) {
        return launch_checked("k_ax_merge", k_ax_merge, dim3(seg_grid(sg.n)), dim3(kSegWG), 0, stream, ax_cols(sg),
                              (unsigned long long)sg.n, plan, plan + S + 1, S, ax_cols(m), (unsigned long long)m.n);
    }
};

}  // namespace
}  // namespace zk

using namespace zk;

struct zk_ax : SegIndex<AxTraits> {};

extern "C" {

zk_status zk_ax_create(const zk_ax_config* cfg, zk_ax** out) {
    ZK_GUARD_BEGIN
    if (!cfg || !out) return ZK_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->num_services < 1 || cfg->num_services > ZK_AX_MAX_SERVICES) return ZK_ERR_INVALID_ARG;
    return seg_create(cfg->device, cfg->num_services, cfg->timing != 0, cfg->stream, out);
    ZK_GUARD_END
}

zk_status zk_ax_destroy(zk_ax* h) {
    ZK_GUARD_BEGIN
    return h ? seg_destroy(h) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

const char* zk_ax_last_error(const zk_ax* h) { return h ? h->err.c_str() : "null handle"; }

zk_status zk_ax_observe(zk_ax* h, const zk_ingest_index_items* in, uint32_t flags) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!in) return seg_fail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (flags & ~ZK_BATCH_DEVICE_PTRS) return seg_fail(h, ZK_ERR_INVALID_ARG, "unknown batch flag");
    const uint64_t n = in->n;
    if (n >= (1ull << 32)) return seg_fail(h, ZK_ERR_UNSUPPORTED, "2^32 entries or more in one batch");
    if (n == 0) return ZK_OK;
    if (!in->service || !in->key || !in->val || !in->ts || !in->trace_id) return seg_fail(h, ZK_ERR_INVALID_ARG, "null column");
    ZK_SEG_HIP(h, hipSetDevice(h->device));
    const uint32_t S = h->S;
    zk_status st;
    if (!h->obs && (st = seg_alloc(h, &h->obs, kObsBytes, "the observe's counters")) != ZK_OK) return st;
    const uint32_t* svc = in->service;
    const unsigned long long* key = (const unsigned long long*)in->key;
    const unsigned long long* val = (const unsigned long long*)in->val;
    const long long* ts = (const long long*)in->ts;
    const unsigned long long* tid = (const unsigned long long*)in->trace_id;
    if (!(flags & ZK_BATCH_DEVICE_PTRS)) {
        // a host batch: its five columns, staged (each 256-B aligned)
        const size_t a8 = (n * 8 + 255) / 256 * 256, a4 = (n * 4 + 255) / 256 * 256;
        if ((st = seg_grow(h, &h->stage, &h->stage_bytes, 4 * a8 + a4, "staging a host batch (36 B per entry)")) != ZK_OK) return st;
        uint8_t* s = (uint8_t*)h->stage;
        ZK_SEG_HIP(h, hipMemcpyAsync(s, in->key, n * 8, hipMemcpyHostToDevice, h->stream));
        ZK_SEG_HIP(h, hipMemcpyAsync(s + a8, in->val, n * 8, hipMemcpyHostToDevice, h->stream));
        ZK_SEG_HIP(h, hipMemcpyAsync(s + 2 * a8, in->ts, n * 8, hipMemcpyHostToDevice, h->stream));
        ZK_SEG_HIP(h, hipMemcpyAsync(s + 3 * a8, in->trace_id, n * 8, hipMemcpyHostToDevice, h->stream));
        ZK_SEG_HIP(h, hipMemcpyAsync(s + 4 * a8, in->service, n * 4, hipMemcpyHostToDevice, h->stream));
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
        if (timing && !e) ZK_SEG_HIP(h, hipEventCreate(&e));
    h->otimed = false;
    ZK_SEG_HIP(h, hipMemsetAsync(counts, 0, (size_t)S * 4, h->stream));
    ZK_SEG_HIP(h, hipMemsetAsync(stat, 0, 8, h->stream));
    if (timing) ZK_SEG_HIP(h, hipEventRecord(h->oev[0], h->stream));
    ZK_SEG_HIP(h, launch_checked("k_ax_count", k_ax_count, dim3(seg_grid((n + kCntItems - 1) / kCntItems, kSegHistGrid)), dim3(kSegWG), 0,
                                 h->stream, svc, (unsigned long long)n, S, counts, stat));
    if (timing) ZK_SEG_HIP(h, hipEventRecord(h->oev[1], h->stream));
    h->counts_host.resize(S);
    unsigned long long bad = 0;
    ZK_SEG_HIP(h, hipMemcpyAsync(h->counts_host.data(), counts, (size_t)S * 4, hipMemcpyDeviceToHost, h->stream));
    ZK_SEG_HIP(h, hipMemcpyAsync(&bad, stat, 8, hipMemcpyDeviceToHost, h->stream));
    ZK_SEG_HIP(h, hipStreamSynchronize(h->stream));  // the call's one synchronisation (also: the staging copies are done)
    if (bad) return seg_fail(h, ZK_ERR_SERVICE_RANGE, std::to_string(bad) + " entr(ies) with service >= num_services");
    Segment g;
    g.off.assign(S + 1, 0);
    for (uint32_t s = 0; s < S; ++s) g.off[s + 1] = g.off[s] + h->counts_host[s];
    g.n = g.off[S];
    if (g.n != n) return seg_fail(h, ZK_ERR_HIP, "entry count out of range");
    if (h->entries + g.n > kSegMaxEntries) return seg_fail(h, ZK_ERR_CAPACITY, "more than 2^32 - 1 entries in one index");
    if (h->segs.size() >= ZK_AX_MAX_SEGMENTS && (st = seg_merge_all(h)) != ZK_OK) return st;
    g.bytes = AxTraits::bytes_for(g.n);
    if ((st = seg_alloc(h, &g.block, g.bytes, "a segment (32 B per entry)")) != ZK_OK) return st;
    h->cursor_host.resize(S);
    for (uint32_t s = 0; s < S; ++s) h->cursor_host[s] = (uint32_t)g.off[s];
    uint32_t grid = (uint32_t)((n + kSegScatterPerWG - 1) / kSegScatterPerWG);
    grid = grid < 1 ? 1 : grid > kSegMaxGrid ? kSegMaxGrid : grid;
    const uint64_t chunk = ((n + grid - 1) / grid + kSegWG - 1) / kSegWG * kSegWG;
    hipError_t e = hipMemcpyAsync(cursor, h->cursor_host.data(), (size_t)S * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && timing) e = hipEventRecord(h->oev[2], h->stream);
    if (e == hipSuccess)
        e = launch_checked("k_ax_scatter", k_ax_scatter, dim3(grid), dim3(kSegWG), 0, h->stream, svc, key, val, ts, tid,
                           (unsigned long long)n, (unsigned long long)chunk, S, cursor, (unsigned long long)g.n, g.col(0), g.col(1),
                           g.col(2), g.col(3));
    if (e == hipSuccess && timing) e = hipEventRecord(h->oev[3], h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(g.block);
        return seg_fail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("k_ax_scatter: ") + launch_error_str(e));
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
    return h && out ? seg_passes_ms(h, h->otimed, h->oev, "no timed observe has added a segment", out) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

zk_status zk_ax_reset(zk_ax* h) {
    ZK_GUARD_BEGIN
    return h ? seg_reset(h) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

zk_status zk_ax_compact(zk_ax* h) {
    ZK_GUARD_BEGIN
    return h ? seg_compact(h) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

zk_status zk_ax_expire(zk_ax* h, int64_t min_ts, uint64_t* removed) {
    ZK_GUARD_BEGIN
    return h ? seg_expire(h, min_ts, removed) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

zk_status zk_ax_expire_ms(zk_ax* h, double out[3]) {
    ZK_GUARD_BEGIN
    return h && out ? seg_passes_ms(h, h->xtimed, h->xev, "no timed expiry has run a pass", out) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

zk_status zk_ax_info(zk_ax* h, uint64_t* entries, uint64_t* segments, uint64_t* bytes) {
    ZK_GUARD_BEGIN
    return h ? seg_info(h, entries, segments, bytes) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

zk_status zk_ax_service_counts(zk_ax* h, uint64_t* counts) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!counts) return seg_fail(h, ZK_ERR_INVALID_ARG, "null argument");
    memcpy(counts, h->svc_count.data(), (size_t)h->S * 8);
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_ax_trace_ids(zk_ax* h, uint32_t service, uint64_t key, uint64_t val, int64_t end_ts, uint32_t limit,
                          uint64_t* trace_id, int64_t* ts, uint32_t* n_out, uint64_t* matched_out) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!trace_id || !ts || !n_out) return seg_fail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (service >= h->S) return seg_fail(h, ZK_ERR_INVALID_ARG, "service >= num_services");
    if (limit < 1 || limit > ZK_AX_MAX_LIMIT) return seg_fail(h, ZK_ERR_INVALID_ARG, "limit outside 1..ZK_AX_MAX_LIMIT");
    return seg_trace_ids(h, service, AxFilter{(unsigned long long)end_ts ^ kTdSign, (unsigned long long)key, (unsigned long long)val}, limit,
                     trace_id, ts, n_out, matched_out);
    ZK_GUARD_END
}

zk_status zk_ax_query_ms(zk_ax* h, double* ms) {
    ZK_GUARD_BEGIN
    return h && ms ? seg_query_ms(h, ms) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

}  // extern "C"
