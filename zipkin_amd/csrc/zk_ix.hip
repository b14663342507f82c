// zk_ix.hip — the trace-id index by service and span name (include/zkindex.h): what is this index's own
// of the segment index of zk_seg_index.h, where segments, merge, select, expiry and the handle are. A
// segment has three columns, tkey[u64] = ts ^ sign, tid[u64], name[u16]: 18 B per entry. Here: the traits,
// k_ix_count and k_ix_scatter with zk_ix_observe, k_ix_names with zk_ix_span_names, the kernels that give
// the shared bodies their names, and the C functions' argument checks.
#include "zk_guard.h"
#include "zk_seg_index.h"
#include "zkindex.h"

namespace zk {
namespace {

// a service's entries in one segment, or (name == nullptr) a list of 16-B entries {tkey, traceId} at tkey
struct IxSlice {
    const unsigned long long* tkey;
    const unsigned long long* tid;
    const uint16_t* name;
    unsigned long long count;
};
// what a query takes of a slice (a list: everything)
struct IxFilter {
    unsigned long long max_key;  // end_ts ^ sign
    uint32_t name;               // ZK_IX_ANY_NAME or a name id
};
static_assert(sizeof(IxSlice) == 32, "slice layout");

// an old segment's entry into the expiry's new one: tid and name lie behind tkey (ix_name); 18 B written
struct IxPut {
    unsigned long long* tkey;
    unsigned long long* tid;
    uint16_t* name;
    __device__ void operator()(const ExpSeg& sg, unsigned long long i, unsigned long long k, unsigned long long at) const {
        const unsigned long long col = (sg.n * 8ull + 255ull) / 256ull * 32ull;  // a column of 8-B words, in words
        tkey[at] = k;
        tid[at] = sg.tkey[col + i];
        name[at] = ((const uint16_t*)(sg.tkey + 2ull * col))[i];
    }
};

uint16_t* ix_name(const Segment& g) { return (uint16_t*)g.col(2); }

// the entry's columns and the filter (the device side of the traits)
struct IxLayout {
    using Slice = IxSlice;
    using Filter = IxFilter;
    __device__ static bool load(const IxSlice& s, unsigned long long i, const IxFilter& f, IxEntry* e) {
        if (i >= s.count) return false;
        if (!s.name) {
            e->tkey = s.tkey[2 * i];
            e->id = s.tkey[2 * i + 1];
            return true;
        }
        if (f.name != ZK_IX_ANY_NAME && (uint32_t)s.name[i] != f.name) return false;
        e->tkey = s.tkey[i];
        if (e->tkey > f.max_key) return false;
        e->id = s.tid[i];
        return true;
    }
    static IxSlice list(const unsigned long long* p, unsigned long long n) { return IxSlice{p, nullptr, nullptr, n}; }
    static IxSlice slice(const Segment& g, uint64_t start, uint64_t n) {
        return IxSlice{g.tkey() + start, g.tid() + start, ix_name(g) + start, n};
    }
    static size_t bytes_for(uint64_t n) { return 2 * Segment::col8(n) + (size_t)((n * 2 + 255) / 256 * 256); }
    static IxPut put(const Segment& g) { return IxPut{g.tkey(), g.tid(), ix_name(g)}; }
};

// the INDEXED predicate of zkindex.h
__device__ inline bool ix_indexed(uint32_t f, uint32_t svc, uint32_t client) {
    if (!(f & ZK_F_HAS_ANNOTATIONS) || !(f & (ZK_F_SVC_CLIENT | ZK_F_SVC_SERVER))) return false;
    const uint32_t cs_cr = (f >> ZK_F_CS_SHIFT) & 0xFu;  // the cs and cr counts
    return !(client != ZK_IX_NO_CLIENT && svc == client && cs_cr != 0u);
}

// ---- observe -------------------------------------------------------------------------------------------
// counts[s] += the indexed records of service s (s < S); stat[0] += the indexed records with s >= S.
// The loop's bounds are the same for all threads of a workgroup, so every lane reaches the ballots.
__global__ __launch_bounds__(kSegWG) void k_ix_count(const uint32_t* __restrict__ svc, const uint32_t* __restrict__ fl,
                                                     unsigned long long n, uint32_t S, uint32_t client,
                                                     uint32_t* __restrict__ counts, unsigned long long* __restrict__ stat) {
    __shared__ uint32_t s_hist[kSegSvcBins];
    __shared__ uint32_t s_bad;
    for (uint32_t b = threadIdx.x; b < kSegSvcBins; b += kSegWG) s_hist[b] = 0u;
    if (threadIdx.x == 0) s_bad = 0u;
    __syncthreads();
    const unsigned long long stride = (unsigned long long)gridDim.x * kCntTile;
    for (unsigned long long base = (unsigned long long)blockIdx.x * kCntTile; base < n; base += stride) {
        uint32_t f[kCntItems], s[kCntItems];  // (the tile's loads first, then the ballots)
#pragma unroll
        for (int j = 0; j < kCntItems; ++j) {
            const unsigned long long i = base + (unsigned long long)j * kSegWG + threadIdx.x;
            f[j] = i < n ? fl[i] : 0u;
            s[j] = i < n ? svc[i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kCntItems; ++j) {
            const bool idx = base + (unsigned long long)j * kSegWG + threadIdx.x < n && ix_indexed(f[j], s[j], client);
            if (idx && s[j] >= S) atomicAdd(&s_bad, 1u);
            hist_add(s_hist, idx && s[j] < S, s[j]);
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kSegSvcBins; b += kSegWG) {
        const uint32_t c = s_hist[b];
        if (c && b < S) atomicAdd(&counts[b], c);
    }
    if (threadIdx.x == 0 && s_bad) atomicAdd(&stat[0], (unsigned long long)s_bad);
}

// Workgroup b owns records [b * chunk, (b + 1) * chunk) (chunk a multiple of the workgroup). cursor[s]
// starts at the segment's off[s]; `total` is the segment's size.
__global__ __launch_bounds__(kSegWG) void k_ix_scatter(const unsigned long long* __restrict__ tid, const long long* __restrict__ last,
                                                       const uint32_t* __restrict__ svc, const uint32_t* __restrict__ fl,
                                                       unsigned long long n, unsigned long long chunk, uint32_t S, uint32_t client,
                                                       uint32_t* __restrict__ cursor, unsigned long long total,
                                                       unsigned long long* __restrict__ out_tkey,
                                                       unsigned long long* __restrict__ out_tid, uint16_t* __restrict__ out_name) {
    __shared__ uint32_t s_cnt[kSegSvcBins];   // the stretch's records per service, then the ranks given out
    __shared__ uint32_t s_base[kSegSvcBins];  // where the workgroup's places of a service begin
    const unsigned long long lo = (unsigned long long)blockIdx.x * chunk;
    const unsigned long long hi = lo + chunk < n ? lo + chunk : n;
    for (uint32_t b = threadIdx.x; b < kSegSvcBins; b += kSegWG) s_cnt[b] = 0u;
    __syncthreads();
    for (unsigned long long base = lo; base < hi; base += kCntTile) {
        uint32_t f[kCntItems], s[kCntItems];
#pragma unroll
        for (int j = 0; j < kCntItems; ++j) {
            const unsigned long long i = base + (unsigned long long)j * kSegWG + threadIdx.x;
            f[j] = i < hi ? fl[i] : 0u;
            s[j] = i < hi ? svc[i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kCntItems; ++j)
            hist_add(s_cnt, base + (unsigned long long)j * kSegWG + threadIdx.x < hi && s[j] < S && ix_indexed(f[j], s[j], client),
                     s[j]);
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
        const uint32_t f = valid ? fl[i] : 0u, s = valid ? svc[i] : 0u;
        const bool take = valid && s < S && ix_indexed(f, s, client);
        const uint32_t rank = hist_rank(s_cnt, take, s);
        if (take) {
            const unsigned long long at = (unsigned long long)s_base[s] + rank;
            if (at < total) {
                out_tkey[at] = (unsigned long long)last[i] ^ kTdSign;
                out_tid[at] = tid[i];
                out_name[at] = (uint16_t)(f >> ZK_F_NAME_SHIFT);
            }
        }
    }
}

// bitmap[id / 32] |= 1 << id % 32 for every name id of the slices. A set bit stays set, so a plain LDS
// read that already shows the bit spares the atomic.
__global__ __launch_bounds__(kSegWG) void k_ix_names(const IxSlice* __restrict__ slices, uint32_t* __restrict__ bitmap) {
    __shared__ uint32_t s_bits[kIxNameWords];
    const IxSlice sl = slices[blockIdx.y];
    for (uint32_t w = threadIdx.x; w < kIxNameWords; w += kSegWG) s_bits[w] = 0u;
    __syncthreads();
    const unsigned long long stride = (unsigned long long)gridDim.x * kSegWG;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kSegWG + threadIdx.x; i < sl.count; i += stride) {
        const uint32_t id = sl.name[i], bit = 1u << (id & 31u);
        if (!(s_bits[id >> 5] & bit)) atomicOr(&s_bits[id >> 5], bit);
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < kIxNameWords; w += kSegWG) {
        const uint32_t v = s_bits[w];
        if (v) atomicOr(&bitmap[w], v);
    }
}

// ---- the wrappers of zk_seg_index.h's and zk_expire.h's bodies -----------------------------------------
__global__ __launch_bounds__(kSegWG) void k_ix_merge(const unsigned long long* __restrict__ src_tkey,
                                                     const unsigned long long* __restrict__ src_tid,
                                                     const uint16_t* __restrict__ src_name, unsigned long long n_src,
                                                     const unsigned long long* __restrict__ src_off,
                                                     const unsigned long long* __restrict__ dst_base, uint32_t S,
                                                     unsigned long long* __restrict__ dst_tkey, unsigned long long* __restrict__ dst_tid,
                                                     uint16_t* __restrict__ dst_name, unsigned long long dst_total) {
    seg_merge(n_src, src_off, dst_base, S, dst_total, [&](unsigned long long i, unsigned long long at) {
        dst_tkey[at] = src_tkey[i];
        dst_tid[at] = src_tid[i];
        dst_name[at] = src_name[i];
    });
}

__global__ __launch_bounds__(kSegWG) void k_ix_scan(const IxSlice* __restrict__ slices, IxSlice one, IxFilter flt,
                                                    unsigned long long* __restrict__ sel) {
    const IxSlice sl = slices ? slices[blockIdx.y] : one;
    const unsigned long long stride = (unsigned long long)gridDim.x * kSegWG;
    unsigned long long or_hi = 0, nor_hi = 0, or_lo = 0, nor_lo = 0, cnt = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kSegWG + threadIdx.x; i < sl.count; i += stride) {
        IxEntry e;
        if (!IxLayout::load(sl, i, flt, &e)) continue;
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

__global__ __launch_bounds__(kSegWG) void k_ix_hist(const IxSlice* __restrict__ slices, IxSlice one, IxFilter flt, uint32_t shift,
                                                    uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[kTdBins];
    const IxSlice sl = slices ? slices[blockIdx.y] : one;
    seg_hist<IxLayout>(sl, flt, shift, hist, s_hist);
}

__global__ __launch_bounds__(kSegWG) void k_ix_collect(const IxSlice* __restrict__ slices, IxSlice one, IxFilter flt, uint32_t shift,
                                                       uint32_t bin, unsigned long long* __restrict__ sel,
                                                       unsigned long long* __restrict__ certain, unsigned long long certain_cap,
                                                       unsigned long long* __restrict__ cand, unsigned long long cand_cap) {
    __shared__ uint32_t s_cnt[2][kColWaves];
    __shared__ unsigned long long s_base[2];
    const IxSlice sl = slices ? slices[blockIdx.y] : one;
    seg_collect<IxLayout>(sl, flt, shift, bin, sel, certain, certain_cap, cand, cand_cap, s_cnt, s_base);
}

__global__ __launch_bounds__(kExpWG) void k_ix_expire_count(const ExpSeg* __restrict__ segs, const ExpItem* __restrict__ items,
                                                            unsigned long long chunk, uint32_t S, unsigned long long cut,
                                                            uint32_t* __restrict__ surv) {
    __shared__ ExpLds lds;
    exp_count(segs, items, chunk, S, cut, surv, &lds);
}

__global__ __launch_bounds__(kExpWG) void k_ix_expire_rewrite(const ExpSeg* __restrict__ segs, const ExpItem* __restrict__ items,
                                                              unsigned long long chunk, uint32_t S, unsigned long long cut,
                                                              uint32_t* __restrict__ cursor, unsigned long long total, IxPut put) {
    __shared__ ExpLds lds;
    __shared__ uint32_t s_base[kExpBins];
    exp_rewrite(segs, items, chunk, S, cut, cursor, total, put, &lds, s_base);
}

// the host side of the traits: the limits, the kernels, the wording
struct IxTraits : IxLayout {
    static constexpr uint32_t MAX_SEGMENTS = ZK_IX_MAX_SEGMENTS, MAX_LIMIT = ZK_IX_MAX_LIMIT;
    static_assert(ZK_IX_MAX_SERVICES == kSegSvcBins, "the shared kernels' bins");
    static constexpr size_t EXTRA_SCRATCH = kIxNameWords * 4;  // zk_ix_span_names' bitmap
    static constexpr const char* MERGED = "the merged segment (18 B per entry)";
    static constexpr const char* SURVIVORS = "the survivors' segment (18 B per entry)";
    static constexpr const char* CONFIG = "zk_ix_config";
    static constexpr SegKernel<decltype(k_ix_scan)> scan{"k_ix_scan", k_ix_scan};
    static constexpr SegKernel<decltype(k_ix_hist)> hist{"k_ix_hist", k_ix_hist};
    static constexpr SegKernel<decltype(k_ix_collect)> collect{"k_ix_collect", k_ix_collect};
    static constexpr SegKernel<decltype(k_ix_expire_count)> expire_count{"k_ix_expire_count", k_ix_expire_count};
    static constexpr SegKernel<decltype(k_ix_expire_rewrite)> expire_rewrite{"k_ix_expire_rewrite", k_ix_expire_rewrite};

    static hipError_t merge(hipStream_t stream, const Segment& sg, const unsigned long long* plan, uint32_t S, const Segment& m) {
        return launch_checked("k_ix_merge", k_ix_merge, dim3(seg_grid(sg.n)), dim3(kSegWG), 0, stream, sg.tkey(), sg.tid(), ix_name(sg),
                              (unsigned long long)sg.n, plan, plan + S + 1, S, m.tkey(), m.tid(), ix_name(m), (unsigned long long)m.n);
    }
};

}  // namespace
}  // namespace zk

using namespace zk;

struct zk_ix : SegIndex<IxTraits> {
    uint32_t client = ZK_IX_NO_CLIENT;
};

extern "C" {

zk_status zk_ix_create(const zk_ix_config* cfg, zk_ix** out) {
    ZK_GUARD_BEGIN
    if (!cfg || !out) return ZK_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->num_services < 1 || cfg->num_services > ZK_IX_MAX_SERVICES) return ZK_ERR_INVALID_ARG;
    const zk_status st = seg_create(cfg->device, cfg->num_services, cfg->timing != 0, cfg->stream, out);
    if (st == ZK_OK) (*out)->client = cfg->client_service;
    return st;
    ZK_GUARD_END
}

zk_status zk_ix_destroy(zk_ix* h) {
    ZK_GUARD_BEGIN
    return h ? seg_destroy(h) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

const char* zk_ix_last_error(const zk_ix* h) { return h ? h->err.c_str() : "null handle"; }

zk_status zk_ix_observe(zk_ix* h, const zk_span_cols* in, uint32_t flags) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!in) return seg_fail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (flags & ~(ZK_BATCH_DEVICE_PTRS | ZK_BATCH_TRACE_CLUSTERED)) return seg_fail(h, ZK_ERR_INVALID_ARG, "unknown batch flag");
    const uint64_t n = in->n;
    if (n >= (1ull << 32)) return seg_fail(h, ZK_ERR_UNSUPPORTED, "2^32 records or more in one batch");
    if (n == 0) return ZK_OK;
    if (!in->trace_id || !in->last_ts || !in->service_id || !in->flags) return seg_fail(h, ZK_ERR_INVALID_ARG, "null column");
    ZK_SEG_HIP(h, hipSetDevice(h->device));
    const uint32_t S = h->S;
    zk_status st;
    if (!h->obs && (st = seg_alloc(h, &h->obs, kObsBytes, "the observe's counters")) != ZK_OK) return st;
    const unsigned long long* tid = (const unsigned long long*)in->trace_id;
    const long long* last = (const long long*)in->last_ts;
    const uint32_t* svc = in->service_id;
    const uint32_t* fl = in->flags;
    if (!(flags & ZK_BATCH_DEVICE_PTRS)) {
        // a host batch: the four columns the index reads, staged (each 256-B aligned)
        const size_t a8 = (n * 8 + 255) / 256 * 256, a4 = (n * 4 + 255) / 256 * 256;
        if ((st = seg_grow(h, &h->stage, &h->stage_bytes, 2 * a8 + 2 * a4, "staging a host batch (24 B per record)")) != ZK_OK)
            return st;
        uint8_t* s = (uint8_t*)h->stage;
        ZK_SEG_HIP(h, hipMemcpyAsync(s, in->trace_id, n * 8, hipMemcpyHostToDevice, h->stream));
        ZK_SEG_HIP(h, hipMemcpyAsync(s + a8, in->last_ts, n * 8, hipMemcpyHostToDevice, h->stream));
        ZK_SEG_HIP(h, hipMemcpyAsync(s + 2 * a8, in->service_id, n * 4, hipMemcpyHostToDevice, h->stream));
        ZK_SEG_HIP(h, hipMemcpyAsync(s + 2 * a8 + a4, in->flags, n * 4, hipMemcpyHostToDevice, h->stream));
        tid = (const unsigned long long*)s;
        last = (const long long*)(s + a8);
        svc = (const uint32_t*)(s + 2 * a8);
        fl = (const uint32_t*)(s + 2 * a8 + a4);
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
    ZK_SEG_HIP(h, launch_checked("k_ix_count", k_ix_count, dim3(seg_grid((n + kCntItems - 1) / kCntItems, kSegHistGrid)), dim3(kSegWG), 0,
                                 h->stream, svc, fl, (unsigned long long)n, S, h->client, counts, stat));
    if (timing) ZK_SEG_HIP(h, hipEventRecord(h->oev[1], h->stream));
    h->counts_host.resize(S);
    unsigned long long bad = 0;
    ZK_SEG_HIP(h, hipMemcpyAsync(h->counts_host.data(), counts, (size_t)S * 4, hipMemcpyDeviceToHost, h->stream));
    ZK_SEG_HIP(h, hipMemcpyAsync(&bad, stat, 8, hipMemcpyDeviceToHost, h->stream));
    ZK_SEG_HIP(h, hipStreamSynchronize(h->stream));  // the call's one synchronisation (also: the staging copies are done)
    if (bad) return seg_fail(h, ZK_ERR_SERVICE_RANGE, std::to_string(bad) + " indexed record(s) with service_id >= num_services");
    Segment g;
    g.off.assign(S + 1, 0);
    for (uint32_t s = 0; s < S; ++s) g.off[s + 1] = g.off[s] + h->counts_host[s];
    g.n = g.off[S];
    if (g.n > n) return seg_fail(h, ZK_ERR_HIP, "entry count out of range");
    if (g.n == 0) return ZK_OK;  // nothing of the batch is indexed: no segment
    if (h->entries + g.n > kSegMaxEntries) return seg_fail(h, ZK_ERR_CAPACITY, "more than 2^32 - 1 entries in one index");
    if (h->segs.size() >= ZK_IX_MAX_SEGMENTS && (st = seg_merge_all(h)) != ZK_OK) return st;
    g.bytes = IxTraits::bytes_for(g.n);
    if ((st = seg_alloc(h, &g.block, g.bytes, "a segment (18 B per entry)")) != ZK_OK) return st;
    h->cursor_host.resize(S);
    for (uint32_t s = 0; s < S; ++s) h->cursor_host[s] = (uint32_t)g.off[s];
    uint32_t grid = (uint32_t)((n + kSegScatterPerWG - 1) / kSegScatterPerWG);
    grid = grid < 1 ? 1 : grid > kSegMaxGrid ? kSegMaxGrid : grid;
    const uint64_t chunk = ((n + grid - 1) / grid + kSegWG - 1) / kSegWG * kSegWG;
    hipError_t e = hipMemcpyAsync(cursor, h->cursor_host.data(), (size_t)S * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && timing) e = hipEventRecord(h->oev[2], h->stream);
    if (e == hipSuccess)
        e = launch_checked("k_ix_scatter", k_ix_scatter, dim3(grid), dim3(kSegWG), 0, h->stream, tid, last, svc, fl,
                           (unsigned long long)n, (unsigned long long)chunk, S, h->client, cursor, (unsigned long long)g.n,
                           g.tkey(), g.tid(), ix_name(g));
    if (e == hipSuccess && timing) e = hipEventRecord(h->oev[3], h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(g.block);
        return seg_fail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("k_ix_scatter: ") + launch_error_str(e));
    }
    for (uint32_t s = 0; s < S; ++s) h->svc_count[s] += h->counts_host[s];
    h->entries += g.n;
    h->segs.push_back(std::move(g));
    h->otimed = timing;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_ix_observe_ms(zk_ix* h, double out[3]) {
    ZK_GUARD_BEGIN
    return h && out ? seg_passes_ms(h, h->otimed, h->oev, "no timed observe has added a segment", out) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

zk_status zk_ix_reset(zk_ix* h) {
    ZK_GUARD_BEGIN
    return h ? seg_reset(h) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

zk_status zk_ix_compact(zk_ix* h) {
    ZK_GUARD_BEGIN
    return h ? seg_compact(h) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

zk_status zk_ix_expire(zk_ix* h, int64_t min_ts, uint64_t* removed) {
    ZK_GUARD_BEGIN
    return h ? seg_expire(h, min_ts, removed) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

zk_status zk_ix_expire_ms(zk_ix* h, double out[3]) {
    ZK_GUARD_BEGIN
    return h && out ? seg_passes_ms(h, h->xtimed, h->xev, "no timed expiry has run a pass", out) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

zk_status zk_ix_info(zk_ix* h, uint64_t* entries, uint64_t* segments, uint64_t* bytes) {
    ZK_GUARD_BEGIN
    return h ? seg_info(h, entries, segments, bytes) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

zk_status zk_ix_service_counts(zk_ix* h, uint64_t* counts) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!counts) return seg_fail(h, ZK_ERR_INVALID_ARG, "null argument");
    memcpy(counts, h->svc_count.data(), (size_t)h->S * 8);
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_ix_trace_ids(zk_ix* h, uint32_t service, uint32_t name, int64_t end_ts, uint32_t limit, uint64_t* trace_id,
                          int64_t* ts, uint32_t* n_out, uint64_t* matched_out) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!trace_id || !ts || !n_out) return seg_fail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (service >= h->S) return seg_fail(h, ZK_ERR_INVALID_ARG, "service >= num_services");
    if (name == 0 || (name > ZK_F_NAME_MASK && name != ZK_IX_ANY_NAME))
        return seg_fail(h, ZK_ERR_INVALID_ARG, "name is 1..65535 or ZK_IX_ANY_NAME");
    if (limit < 1 || limit > ZK_IX_MAX_LIMIT) return seg_fail(h, ZK_ERR_INVALID_ARG, "limit outside 1..ZK_IX_MAX_LIMIT");
    return seg_trace_ids(h, service, IxFilter{(unsigned long long)end_ts ^ kTdSign, name}, limit, trace_id, ts, n_out, matched_out);
    ZK_GUARD_END
}

zk_status zk_ix_span_names(zk_ix* h, uint32_t service, uint16_t* name_ids, uint32_t cap, uint32_t* n_out) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!n_out || (cap && !name_ids)) return seg_fail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (service >= h->S) return seg_fail(h, ZK_ERR_INVALID_ARG, "service >= num_services");
    *n_out = 0;
    if (h->svc_count[service] == 0) return ZK_OK;
    ZK_SEG_HIP(h, hipSetDevice(h->device));
    uint64_t total = 0, longest = 0;
    zk_status st = seg_plan(h, service, &total, &longest);
    if (st != ZK_OK) return st;
    if (!total) return ZK_OK;
    uint8_t* sb = (uint8_t*)h->sel;
    uint32_t* bitmap = (uint32_t*)(sb + zk_ix::kSelExtraAt);
    const uint32_t ns = (uint32_t)h->spans.size();
    ZK_SEG_HIP(h, hipMemsetAsync(bitmap, 0, kIxNameWords * 4, h->stream));
    ZK_SEG_HIP(h, launch_checked("k_ix_names", k_ix_names, dim3(seg_grid(longest, std::max(1u, kSegHistGrid / ns)), ns), dim3(kSegWG), 0,
                                 h->stream, (const IxSlice*)(sb + zk_ix::kSelSlicesAt), bitmap));
    static thread_local std::vector<uint32_t> bits;
    bits.resize(kIxNameWords);
    ZK_SEG_HIP(h, hipMemcpyAsync(bits.data(), bitmap, kIxNameWords * 4, hipMemcpyDeviceToHost, h->stream));
    ZK_SEG_HIP(h, hipStreamSynchronize(h->stream));
    const uint32_t need = ix_names_of(bits.data(), nullptr, 0);
    *n_out = need;
    if (need > cap) return seg_fail(h, ZK_ERR_CAPACITY, "name_ids holds fewer than the service's span names");
    ix_names_of(bits.data(), name_ids, cap);
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_ix_query_ms(zk_ix* h, double* ms) {
    ZK_GUARD_BEGIN
    return h && ms ? seg_query_ms(h, ms) : ZK_ERR_INVALID_ARG;
    ZK_GUARD_END
}

}  // extern "C"
