// zk_lh.hip — per-link duration histogram (include/zksketch.h, zk_lh_*): p50/p99 of every
// dependency edge.
//
// A DependencyLink carries only Moments (Dependencies.scala:34). Bound to a dependency ctx, every
// link the job emits -- (cell << 40) | d, cell = parent * S + child, the rows ZipkinAggregateJob.scala:
// 25-37 sums -- is also counted into u32 hist[cell][bin], bin = zk_rt's log-linear bin of d
// (zk_sketch_internal.h rt_bin). Integer counts: independent of batch order and cuts, merged across
// traceId shards by SUM.
//
// k_lh_tiles runs after the link reduce and reads the bucket-ordered copy of the batch's links K2
// left behind (ReduceArgs.sorted, bucket b = cells [b << cb_shift, (b + 1) << cb_shift) at
// [bucket_base[b], bucket_base[b + 1]); 4-byte compact words, zk_internal.h: a long link's word is its
// slot in the K1 lists, which hold the full link until the next join). A bucket's rows (512 cells x
// 592 bins x 4 B = 1.2 MB at m = 4) do not fit the 160 KiB of LDS, so a bucket is tiled by cell sub-range: T = 2^tshift cells per tile,
// the largest power of two whose T x bins counters fit (lh_tile_shift: 128 cells at m = 2 and 3, 64
// at 4, 32 at 5, 16 at 6, 8 at 7). One workgroup per (bucket, tile) walks the bucket's links, counts
// those of its own cells with LDS atomics and then adds the non-zero counters to the rows in HBM with
// plain loads and stores: it is the only workgroup that touches those rows, so no global atomic is
// issued (a global atomic executes at the memory side, one 64-B request per scattered dword, an order
// of magnitude below contiguous traffic). Every tile of a bucket re-reads the bucket's links; the
// tiles of one bucket are placed on one XCD so the re-reads meet in its L2. With few buckets (small
// S) each (bucket, tile) is split over several workgroups by link range for parallelism, and only
// then the flush adds are atomic -- as K3 does (zk_reduce.hip).
//
// The spill kernel bypasses the link lists (zk_join.hip emit_link): it adds its links' bins with one
// device-scope atomic each (JoinArgs.lh_hist); spilled traces are rare. Without bucket order (S >
// 1024: the table itself is then reduced with global atomics, k_link_reduce_atomic) k_lh_lists reads
// the K1 lists and adds one atomic per link.
//
// The table is dense; what leaves it is not. zk_lh_snapshot compacts the non-zero counters into the
// canonical sparse snapshot of zksketch.h (k_lh_snap_count, three u64 scans, k_lh_snap_write) and
// zk_lh_merge adds one back (k_lh_merge); the host-only functions over snapshots are in
// zk_lh_snapshot.cpp. Neither touches the accumulate path above.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "zk_comm.h"
#include "zk_guard.h"
#include "zk_internal.h"
#include "zk_launch.h"
#include "zk_lh_internal.h"
#include "zk_lh_snapshot.h"
#include "zk_sketch_internal.h"
#include "zksketch.h"

namespace zk {
namespace {

constexpr int kLhWG = 1024;  // one workgroup per CU (its tile takes the LDS): 16 waves hide the link loads
constexpr int kLhU = 4;      // links per thread per iteration (the next iteration's in flight)
// LDS of one tile: what a CU has, less room for the kernel's static LDS and the runtime's own
constexpr uint64_t kLhLdsBudget = 152ull * 1024;
constexpr uint32_t kLhMaxQ = 8;  // quantiles per k_lh_quantiles pass
constexpr uint32_t kLhTargetWGs = 512;  // (bucket, tile) pairs below this are split by link range

struct LhArgs {
    const void* sorted;           // the batch's links in bucket order: compact words, or 8-byte links
    const uint64_t* links;        // the K1 lists (a compact escape's full link)
    const uint64_t* bucket_base;  // [nb + 1]
    uint32_t cb_shift;
    uint64_t cells;
    uint32_t* hist;               // [cells][bins]
    uint32_t bins, m;
    uint32_t tshift;              // tile = 2^tshift cells
    uint32_t nsub;                // tiles per bucket
    uint32_t splits;              // workgroups per (bucket, tile)
};

template <bool COMPACT>
__global__ __launch_bounds__(kLhWG) void k_lh_tiles(LhArgs a) {
    extern __shared__ uint32_t s_h[];  // [T][bins]
    using W = typename std::conditional<COMPACT, uint32_t, uint64_t>::type;
    using L = uint64_t;                   // one load
    constexpr int WPL = COMPACT ? 2 : 1;  // words per load
    const L* const units = static_cast<const L*>(a.sorted);
    const int tid = threadIdx.x;
    // XCD-aware order (dispatch puts block i on XCD i % 8): the blocks of one XCD take consecutive
    // work items, so the tiles of one bucket read its links through one L2
    const uint32_t gx = gridDim.x / 8, gr = gridDim.x % 8, xi = blockIdx.x % 8;
    const uint32_t item = xi * gx + (xi < gr ? xi : gr) + blockIdx.x / 8;
    const uint32_t per_bucket = a.nsub * a.splits;
    const uint32_t b = item / per_bucket, rem = item % per_bucket;
    const uint32_t sub = rem / a.splits, part = rem % a.splits;
    const uint64_t lo = a.bucket_base[b], hi = a.bucket_base[b + 1];
    const uint64_t per = (hi - lo + a.splits - 1) / a.splits;
    const uint64_t p0 = lo + per * part;
    const uint64_t p1 = (p0 + per < hi) ? p0 + per : hi;
    if (p0 >= p1) return;  // (uniform) no link in this range
    const uint32_t T = 1u << a.tshift;
    const uint32_t words = T * a.bins;
    for (uint32_t x = tid; x < words; x += kLhWG) s_h[x] = 0u;
    const uint64_t cell0 = (uint64_t)b << a.cb_shift;
    // (an 8-byte link is never all ones here: bucket order exists for S <= 1024 only, cell < 2^20;
    // nor is a compact word: zk_internal.h)
    auto count = [&](W w) {
        uint32_t c;
        uint64_t d;
        if constexpr (COMPACT) {
            if (w & kCompactEscape) {  // (the cell of a long link is in the lists only)
                const uint64_t x = a.links[w & ~kCompactEscape];
                c = (uint32_t)((x >> 40) - cell0);
                d = x & (kMaxDuration - 1);
            } else {
                c = w >> kCompactDurBits;
                d = w & kCompactDurMask;
            }
        } else {
            c = (uint32_t)((w >> 40) - cell0);
            d = w & (kMaxDuration - 1);
        }
        if ((c >> a.tshift) != sub) return;  // another tile's cell (sub < nsub bounds c to the bucket)
        atomicAdd(&s_h[(c & (T - 1)) * a.bins + rt_bin(d, a.m)], 1u);
    };
    // one 8-byte load is one link, or an aligned pair of compact words (as many bytes per load and in
    // flight either way: with one word per load the kernel ran 0.64-0.68 ms against 0.62 ms); the words
    // of the first and last pair outside [p0, p1) are skipped by their index
    const uint64_t u0 = p0 / WPL, u1 = (p1 + WPL - 1) / WPL;
    L nxt[kLhU];
#pragma unroll
    for (int k = 0; k < kLhU; ++k) {
        const uint64_t u = u0 + tid + (uint64_t)k * kLhWG;
        nxt[k] = u < u1 ? units[u] : ~(L)0;
    }
    __syncthreads();
    for (uint64_t base = u0; base < u1; base += (uint64_t)kLhWG * kLhU) {
        L v[kLhU];
#pragma unroll
        for (int k = 0; k < kLhU; ++k) {
            v[k] = nxt[k];
            const uint64_t u = base + (uint64_t)kLhWG * kLhU + tid + (uint64_t)k * kLhWG;
            nxt[k] = u < u1 ? units[u] : ~(L)0;
        }
#pragma unroll
        for (int k = 0; k < kLhU; ++k) {
            if (v[k] == ~(L)0) continue;
            if constexpr (COMPACT) {
                const uint64_t i = (base + tid + (uint64_t)k * kLhWG) * 2;
                const uint32_t w0 = (uint32_t)v[k], w1 = (uint32_t)(v[k] >> 32);
                if (i >= p0) count(w0);
                if (i + 1 < p1) count(w1);
            } else {
                count(v[k]);
            }
        }
    }
    __syncthreads();
    // one wave per row: the non-zero counters of a row added to HBM side by side
    const uint32_t wave = tid >> 6, lane = tid & 63;
    for (uint32_t r = wave; r < T; r += kLhWG / 64) {
        const uint64_t cell = cell0 + (uint64_t)sub * T + r;
        if (cell >= a.cells) break;  // (rows ascend) past the table's last cell
        uint32_t* dst = a.hist + cell * a.bins;
        const uint32_t* src = s_h + r * a.bins;
        for (uint32_t x = lane; x < a.bins; x += 64) {
            const uint32_t n = src[x];
            if (!n) continue;
            if (a.splits == 1)
                dst[x] += n;  // this workgroup owns the row
            else
                atomicAdd(&dst[x], n);
        }
    }
}

// no bucket order (S > 1024): the K1 lists as they are, one atomic per link
__global__ __launch_bounds__(256) void k_lh_lists(const uint64_t* __restrict__ links, const uint32_t* __restrict__ counts,
                                                  uint64_t stride, uint32_t lists, uint64_t cells,
                                                  uint32_t* __restrict__ hist, uint32_t bins, uint32_t m) {
    for (uint32_t w = blockIdx.x; w < lists; w += gridDim.x) {
        const uint32_t c = counts[w];
        const uint64_t* L = links + (uint64_t)w * stride;
        for (uint32_t i = threadIdx.x; i < c; i += 256) {
            const uint64_t v = L[i];
            const uint64_t cell = v >> 40;
            if (cell < cells) atomicAdd(&hist[cell * bins + rt_bin(v & (kMaxDuration - 1), m)], 1u);
        }
    }
}

// dropped += sign * (the ctx's duration-range counter summed over its stats shards)
__global__ __launch_bounds__(kStatShards) void k_lh_note_dropped(const unsigned long long* __restrict__ stats, int sign,
                                                                 unsigned long long* __restrict__ dropped) {
    __shared__ unsigned long long s_w[kStatShards / 64];
    unsigned long long v = stats[(uint64_t)threadIdx.x * ST_N + ST_DUR_RANGE];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kStatShards / 64; ++w) t += s_w[w];
        *dropped += sign > 0 ? t : 0ull - t;  // (wraps between the two calls of a batch)
    }
}

// One wave per cell: the row's total N, then for each q[i] the bin holding the nearest rank
// max(1, ceil(q N)), by a wave prefix over 64-bin chunks with a carried running count.
// count[cell] = N; qbin[cell * nq + i] = the bin (0 when N = 0).
__global__ __launch_bounds__(256) void k_lh_quantiles(const uint32_t* __restrict__ hist, uint64_t cells, uint32_t bins,
                                                      const double* __restrict__ q, uint32_t nq,
                                                      unsigned long long* __restrict__ count, uint32_t* __restrict__ qbin) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t cell = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= cells) return;
    const uint32_t* row = hist + cell * bins;
    unsigned long long n = 0;
    for (uint32_t x = lane; x < bins; x += 64) n += row[x];
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if (lane == 0) count[cell] = n;
    if (n == 0) {
        if (lane < nq) qbin[cell * nq + lane] = 0u;
        return;
    }
    unsigned long long rank[kLhMaxQ];
#pragma unroll
    for (uint32_t i = 0; i < kLhMaxQ; ++i) {
        unsigned long long r = 0;  // (0: no bin matches)
        if (i < nq) {
            r = (unsigned long long)ceil(q[i] * (double)n);
            if (r < 1) r = 1;
            if (r > n) r = n;
        }
        rank[i] = r;
    }
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < bins; base += 64) {
        const uint32_t x = base + lane;
        const unsigned long long v = x < bins ? row[x] : 0u;
        unsigned long long incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long o = __shfl_up(incl, off);
            if ((int)lane >= off) incl += o;
        }
        incl += carry;
        const unsigned long long excl = incl - v;
#pragma unroll
        for (uint32_t i = 0; i < kLhMaxQ; ++i)
            if (excl < rank[i] && rank[i] <= incl) qbin[cell * nq + i] = x;
        carry = __shfl(incl, 63);
    }
}

// [lo, hi] of a bin (oracle/realtime.py bin_bounds)
void lh_bin_bounds(uint32_t b, uint32_t m, int64_t* lo, int64_t* hi) {
    if (b < (1u << m)) {
        *lo = *hi = (int64_t)b;
        return;
    }
    const uint32_t g = b >> m, mant = b & ((1u << m) - 1u);
    const uint32_t e = g + m - 1u;
    *lo = (int64_t)(((1ull << m) | mant) << (e - m));
    *hi = *lo + (int64_t)(1ull << (e - m)) - 1;
}

// ---- snapshots (zksketch.h, zk_lh_snapshot / zk_lh_merge): the present bins only -----------------
//
// Count pass, one wave per cell (the shape of k_lh_quantiles): per 64-bin chunk a ballot of the
// non-zero counters and its popcount. nz[cell] = the cell's non-zero counters, present[cell] = whether
// it has any, sum[cell] = its links. The host then scans all three in place (inclusive, u64: at large
// S the entries pass 2^32), which fixes every row's and every entry's position: no atomic anywhere, so
// the bytes are the same on every run.
__global__ __launch_bounds__(256) void k_lh_snap_count(const uint32_t* __restrict__ hist, uint64_t cells, uint32_t bins,
                                                       unsigned long long* __restrict__ nz,
                                                       unsigned long long* __restrict__ present,
                                                       unsigned long long* __restrict__ sum) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t cell = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= cells) return;  // (uniform over the wave)
    const uint32_t* row = hist + cell * bins;
    uint32_t cnt = 0;
    unsigned long long s = 0;
    for (uint32_t base = 0; base < bins; base += 64) {
        const uint32_t x = base + lane;
        const uint32_t v = x < bins ? row[x] : 0u;
        cnt += (uint32_t)__popcll(__ballot(v != 0u));
        s += v;
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) {
        nz[cell] = cnt;
        present[cell] = cnt ? 1ull : 0ull;
        sum[cell] = s;
    }
}

// Write pass, one wave per cell; a wave whose cell is absent leaves at once. nz_incl / row_incl are the
// inclusive scans: the row is row_incl[cell] - 1 and its entries start at nz_incl[cell - 1]. Within a
// chunk a lane's position is the count of non-zero lanes below it (ballot + mbcnt), after a running
// count carried across the chunks; one 8-byte store per non-zero counter, lane 0 writes the descriptor.
// n_rows / n_entries (the scans' totals) bound every store.
__global__ __launch_bounds__(256) void k_lh_snap_write(const uint32_t* __restrict__ hist, uint64_t cells, uint32_t bins,
                                                       uint32_t S, const unsigned long long* __restrict__ nz_incl,
                                                       const unsigned long long* __restrict__ row_incl,
                                                       LhSnapRow* __restrict__ rows, unsigned long long n_rows,
                                                       unsigned long long* __restrict__ entries,
                                                       unsigned long long n_entries) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t cell = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= cells) return;
    const unsigned long long e0 = cell ? nz_incl[cell - 1] : 0ull, e1 = nz_incl[cell];
    if (e1 == e0) return;  // (uniform) no link on this edge
    const unsigned long long r = row_incl[cell] - 1;
    if (lane == 0 && r < n_rows) rows[r] = LhSnapRow{(uint32_t)(cell / S), (uint32_t)(cell % S), e0};
    const uint32_t* row = hist + cell * bins;
    unsigned long long at = e0;
    for (uint32_t base = 0; base < bins; base += 64) {
        const uint32_t x = base + lane;
        const uint32_t v = x < bins ? row[x] : 0u;
        const unsigned long long mask = __ballot(v != 0u);
        const unsigned long long pos = at + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (v && pos < n_entries) entries[pos] = ((unsigned long long)x << 32) | v;
        at += (unsigned long long)__popcll(mask);
    }
}

// Merge, one wave per snapshot row: the row's counters loaded, added and stored. Rows are distinct
// cells and a row's bins are distinct, so no two lanes meet: no atomic. The host validated the blob
// (bin < bins, parent and child < S, first ascending and within n_entries) before it was copied.
__global__ __launch_bounds__(256) void k_lh_merge(uint32_t* __restrict__ hist, uint32_t bins, uint32_t S,
                                                  const LhSnapRow* __restrict__ rows, unsigned long long n_rows,
                                                  const unsigned long long* __restrict__ entries,
                                                  unsigned long long n_entries, unsigned long long dropped_more,
                                                  unsigned long long* __restrict__ dropped) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r == 0 && lane == 0) *dropped += dropped_more;
    if (r >= n_rows) return;
    const LhSnapRow row = rows[r];
    const unsigned long long e1 = r + 1 < n_rows ? rows[r + 1].first : n_entries;
    uint32_t* dst = hist + ((uint64_t)row.parent * S + row.child) * bins;
    for (unsigned long long i = row.first + lane; i < e1; i += 64) {
        const unsigned long long e = entries[i];
        dst[e >> 32] += (uint32_t)e;
    }
}

}  // namespace
}  // namespace zk

using namespace zk;

struct zk_lh {
    int device = 0;
    hipStream_t stream = nullptr;  // the bound ctx's while bound, else `own`
    hipStream_t own = nullptr;
    uint32_t S = 0, m = 4, bins = 0;
    uint64_t cells = 0;
    uint32_t* hist = nullptr;                // [cells][bins]
    unsigned long long* dropped = nullptr;   // device: links dropped for their duration while bound
    uint64_t reserved = 0;                   // records accumulated since reset (links <= records)
    // quantiles_all: one pass of up to kLhMaxQ quantiles
    double* q_dev = nullptr;
    unsigned long long* q_cnt = nullptr;     // [cells]
    uint32_t* q_bin = nullptr;               // [cells][kLhMaxQ]
    // snapshot / merge scratch, allocated on first use: the three per-cell u64 arrays of the count
    // pass (scanned in place), the scan's workspace, and the rows + entries of one blob
    unsigned long long* s_cell = nullptr;    // [3][cells]: nz, present, sum
    void* s_tmp = nullptr;
    size_t s_tmp_bytes = 0;
    uint8_t* s_blob = nullptr;
    uint64_t s_blob_bytes = 0;
    hipEvent_t s_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool s_timed = false;
    std::string err;
};

namespace {

zk_status hfail(zk_lh* h, zk_status s, const std::string& m) {
    if (h) h->err = m;
    return s;
}

#define LH_HIP(h, call)                                                                            \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess) return hfail(h, is_refusal(_e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP,       \
                                           std::string(#call) + ": " + launch_error_str(_e));      \
    } while (0)

zk_status check_q(zk_lh* h, const double* q, uint32_t nq, const int64_t* lo, const int64_t* hi) {
    if (nq && (!q || !lo || !hi)) return hfail(h, ZK_ERR_INVALID_ARG, "null array");
    for (uint32_t i = 0; i < nq; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return hfail(h, ZK_ERR_INVALID_ARG, "quantile outside [0, 1]");
    return ZK_OK;
}

// the per-cell arrays, the scan's workspace and the events of zk_lh_snapshot, on first use; a refused
// allocation is ZK_ERR_CAPACITY and changes nothing
zk_status snap_scratch(zk_lh* h) {
    if (h->s_cell) return ZK_OK;
    size_t tb = 0;
    LH_HIP(h, hipcub::DeviceScan::InclusiveSum(nullptr, tb, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                               (int)h->cells, h->stream));
    for (hipEvent_t& e : h->s_ev)
        if (!e) LH_HIP(h, hipEventCreate(&e));
    void* tmp = nullptr;
    unsigned long long* cell = nullptr;
    if (hipMalloc(&tmp, tb ? tb : 8) != hipSuccess || hipMalloc(&cell, h->cells * 24) != hipSuccess) {
        (void)hipGetLastError();
        if (tmp) (void)hipFree(tmp);
        return hfail(h, ZK_ERR_CAPACITY, "no device memory for the snapshot's scratch (24 B per cell)");
    }
    h->s_tmp = tmp;
    h->s_tmp_bytes = tb;
    h->s_cell = cell;
    return ZK_OK;
}

// room for the rows and entries of one blob in HBM (kept, grown when a larger blob comes)
zk_status snap_blob(zk_lh* h, uint64_t bytes) {
    if (bytes <= h->s_blob_bytes) return ZK_OK;
    LH_HIP(h, hipStreamSynchronize(h->stream));
    uint8_t* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return hfail(h, ZK_ERR_CAPACITY, "no device memory for the snapshot's rows and entries");
    }
    if (h->s_blob) (void)hipFree(h->s_blob);
    h->s_blob = p;
    h->s_blob_bytes = bytes;
    return ZK_OK;
}

}  // namespace

namespace zk {

uint32_t lh_tile_shift(uint32_t bins, uint32_t cb_shift) {
    uint32_t t = 0;
    while (t < cb_shift && (2ull << t) * bins * 4 <= kLhLdsBudget) ++t;
    return t;
}

void lh_join_args(zk_lh* h, JoinArgs* a) {
    a->lh_hist = h->hist;
    a->lh_bins = h->bins;
    a->lh_m = h->m;
}

hipError_t lh_note_dropped(zk_lh* h, const unsigned long long* stats, int sign) {
    return launch_checked("k_lh_note_dropped", k_lh_note_dropped, dim3(1), dim3(kStatShards), 0, h->stream, stats, sign,
                          h->dropped);
}

hipError_t lh_accumulate(zk_lh* h, const ReduceArgs& r) {
    if (!r.lists) return hipSuccess;
    if (!r.nb) {
        const uint32_t grid = r.lists < 4096 ? r.lists : 4096;
        return launch_checked("k_lh_lists", k_lh_lists, dim3(grid), dim3(256), 0, h->stream, r.links, r.counts, r.stride,
                              r.lists, h->cells, h->hist, h->bins, h->m);
    }
    LhArgs a{};
    a.sorted = r.sorted;
    a.links = r.links;
    a.bucket_base = r.bucket_base;
    a.cb_shift = r.cb_shift;
    a.cells = h->cells;
    a.hist = h->hist;
    a.bins = h->bins;
    a.m = h->m;
    a.tshift = lh_tile_shift(h->bins, r.cb_shift);
    a.nsub = 1u << (r.cb_shift - a.tshift);
    const uint32_t pairs = r.nb * a.nsub;
    a.splits = pairs >= kLhTargetWGs ? 1u : (kLhTargetWGs + pairs - 1) / pairs;
    const size_t lds = ((size_t)h->bins << a.tshift) * 4;
    return r.compact ? launch_checked("k_lh_tiles", k_lh_tiles<true>, dim3(pairs * a.splits), dim3(kLhWG), lds, h->stream, a)
                     : launch_checked("k_lh_tiles", k_lh_tiles<false>, dim3(pairs * a.splits), dim3(kLhWG), lds, h->stream, a);
}

uint64_t lh_reserved(const zk_lh* h) { return h->reserved; }
void lh_reserve(zk_lh* h, uint64_t n) { h->reserved += n; }
int lh_device(const zk_lh* h) { return h->device; }
uint32_t lh_services(const zk_lh* h) { return h->S; }
void lh_set_stream(zk_lh* h, hipStream_t s) {
    hipStream_t ns = s ? s : h->own;
    if (ns != h->stream) {
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        h->stream = ns;
    }
}

zk_status lh_allreduce(zk_lh* h, zk_comm* comm) {
    if (!comm) return hfail(h, ZK_ERR_INVALID_ARG, "null communicator");
    LH_HIP(h, hipSetDevice(h->device));
    // bins and the drop counter by SUM, on the handle's (bound ctx's) stream
    zk_status st = comm_allreduce(comm, h->hist, h->cells * h->bins, kCommU32, kCommSum, h->device, h->stream, &h->err);
    if (st == ZK_OK) st = comm_allreduce(comm, h->dropped, 1, kCommU64, kCommSum, h->device, h->stream, &h->err);
    return st;
}

}  // namespace zk

extern "C" {

zk_status zk_lh_create(const zk_lh_config* cfg, zk_lh** out) {
    ZK_GUARD_BEGIN
    if (!cfg || !out) return ZK_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->num_services == 0 || cfg->num_services > kMaxServices) return ZK_ERR_INVALID_ARG;
    if (cfg->sub_bits != 0 && (cfg->sub_bits < 2 || cfg->sub_bits > 7)) return ZK_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) return ZK_ERR_NO_DEVICE;
    if (hipSetDevice(cfg->device) != hipSuccess) return ZK_ERR_HIP;
    zk_lh* h = new zk_lh();
    h->device = cfg->device;
    h->S = cfg->num_services;
    h->m = cfg->sub_bits ? cfg->sub_bits : 4u;
    h->bins = rt_nbins(h->m);
    h->cells = (uint64_t)h->S * h->S;
    if (cfg->stream) {
        h->stream = (hipStream_t)cfg->stream;
    } else if (hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return ZK_ERR_HIP;
    } else {
        h->stream = h->own;
    }
    // the whole state at once: no accumulate ever allocates
    if (hipMalloc(&h->hist, h->cells * h->bins * 4) != hipSuccess) {
        (void)hipGetLastError();
        h->hist = nullptr;
        zk_lh_destroy(h);
        return ZK_ERR_CAPACITY;
    }
    if (hipMalloc(&h->dropped, 8) != hipSuccess || zk_lh_reset(h) != ZK_OK) {
        (void)hipGetLastError();
        zk_lh_destroy(h);
        return ZK_ERR_HIP;
    }
    *out = h;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_lh_destroy(zk_lh* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void* p : {(void*)h->hist, (void*)h->dropped, (void*)h->q_dev, (void*)h->q_cnt, (void*)h->q_bin,
                    (void*)h->s_cell, h->s_tmp, (void*)h->s_blob})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : h->s_ev)
        if (e) (void)hipEventDestroy(e);
    if (h->own) (void)hipStreamDestroy(h->own);
    delete h;
    return ZK_OK;
    ZK_GUARD_END
}

const char* zk_lh_last_error(const zk_lh* h) { return h ? h->err.c_str() : "null handle"; }

zk_status zk_lh_reset(zk_lh* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    LH_HIP(h, hipSetDevice(h->device));
    LH_HIP(h, hipMemsetAsync(h->hist, 0, h->cells * h->bins * 4, h->stream));
    LH_HIP(h, hipMemsetAsync(h->dropped, 0, 8, h->stream));
    h->reserved = 0;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_lh_geometry(const zk_lh* h, uint32_t* bins) {
    if (!h || !bins) return ZK_ERR_INVALID_ARG;
    *bins = h->bins;
    return ZK_OK;
}

zk_status zk_lh_quantiles(zk_lh* h, uint32_t parent, uint32_t child, const double* q, uint32_t nq, int64_t* lo,
                          int64_t* hi, uint64_t* count) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (parent >= h->S || child >= h->S) return hfail(h, ZK_ERR_SERVICE_RANGE, "service id >= num_services");
    const zk_status cs = check_q(h, q, nq, lo, hi);
    if (cs != ZK_OK) return cs;
    LH_HIP(h, hipSetDevice(h->device));
    // one row to the host, scanned there
    std::vector<uint32_t> row(h->bins);
    const uint64_t cell = (uint64_t)parent * h->S + child;
    LH_HIP(h, hipMemcpyAsync(row.data(), h->hist + cell * h->bins, (uint64_t)h->bins * 4, hipMemcpyDeviceToHost, h->stream));
    LH_HIP(h, hipStreamSynchronize(h->stream));
    uint64_t N = 0;
    for (uint32_t c : row) N += c;
    if (count) *count = N;
    for (uint32_t i = 0; i < nq; ++i) {
        lo[i] = hi[i] = 0;
        if (!N) continue;
        uint64_t rank = (uint64_t)ceil(q[i] * (double)N);  // nearest rank, 1-based
        if (rank < 1) rank = 1;
        if (rank > N) rank = N;
        uint64_t cum = 0;
        for (uint32_t b = 0; b < h->bins; ++b) {
            cum += row[b];
            if (cum >= rank) {
                lh_bin_bounds(b, h->m, &lo[i], &hi[i]);
                break;
            }
        }
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_lh_quantiles_all(zk_lh* h, const double* q, uint32_t nq, int64_t* lo, int64_t* hi, uint64_t* count) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    const zk_status cs = check_q(h, q, nq, lo, hi);
    if (cs != ZK_OK) return cs;
    if (!nq && !count) return ZK_OK;
    LH_HIP(h, hipSetDevice(h->device));
    if (!h->q_bin) {
        if (hipMalloc(&h->q_dev, kLhMaxQ * sizeof(double)) != hipSuccess || hipMalloc(&h->q_cnt, h->cells * 8) != hipSuccess ||
            hipMalloc(&h->q_bin, h->cells * kLhMaxQ * 4) != hipSuccess) {
            (void)hipGetLastError();
            for (void* p : {(void*)h->q_dev, (void*)h->q_cnt, (void*)h->q_bin})
                if (p) (void)hipFree(p);
            h->q_dev = nullptr;
            h->q_cnt = nullptr;
            h->q_bin = nullptr;
            return hfail(h, ZK_ERR_CAPACITY, "no device memory for the quantile query (40 B per cell)");
        }
    }
    std::vector<unsigned long long> cnt(h->cells);
    std::vector<uint32_t> qb;
    const uint32_t grid = (uint32_t)((h->cells + 3) / 4);
    for (uint32_t i0 = 0; i0 < nq || i0 == 0; i0 += kLhMaxQ) {
        const uint32_t k = nq - i0 < kLhMaxQ ? nq - i0 : kLhMaxQ;
        if (k) LH_HIP(h, hipMemcpyAsync(h->q_dev, q + i0, k * sizeof(double), hipMemcpyHostToDevice, h->stream));
        LH_HIP(h, launch_checked("k_lh_quantiles", k_lh_quantiles, dim3(grid), dim3(256), 0, h->stream,
                                 (const uint32_t*)h->hist, h->cells, h->bins, (const double*)h->q_dev, k, h->q_cnt, h->q_bin));
        qb.resize((size_t)h->cells * k);
        LH_HIP(h, hipMemcpyAsync(cnt.data(), h->q_cnt, h->cells * 8, hipMemcpyDeviceToHost, h->stream));
        if (k) LH_HIP(h, hipMemcpyAsync(qb.data(), h->q_bin, h->cells * k * 4, hipMemcpyDeviceToHost, h->stream));
        LH_HIP(h, hipStreamSynchronize(h->stream));  // (also: q was read before the next pass overwrites it)
        for (uint64_t c = 0; c < h->cells; ++c) {
            if (count) count[c] = cnt[c];
            for (uint32_t i = 0; i < k; ++i) {
                int64_t* l = lo + c * nq + i0 + i;
                int64_t* u = hi + c * nq + i0 + i;
                if (cnt[c])
                    lh_bin_bounds(qb[c * k + i], h->m, l, u);
                else
                    *l = *u = 0;
            }
        }
        if (!nq) break;
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_lh_read(zk_lh* h, uint64_t first_cell, uint64_t n_cells, uint32_t* out) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (first_cell > h->cells || n_cells > h->cells - first_cell) return hfail(h, ZK_ERR_INVALID_ARG, "cell range past S * S");
    if (n_cells && !out) return hfail(h, ZK_ERR_INVALID_ARG, "null array");
    LH_HIP(h, hipSetDevice(h->device));
    if (n_cells)
        LH_HIP(h, hipMemcpyAsync(out, h->hist + first_cell * h->bins, n_cells * h->bins * 4, hipMemcpyDeviceToHost, h->stream));
    LH_HIP(h, hipStreamSynchronize(h->stream));
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_lh_snapshot(zk_lh* h, void* out, uint64_t cap, uint64_t* bytes) {
    ZK_GUARD_BEGIN
    if (!h || !bytes) return ZK_ERR_INVALID_ARG;
    LH_HIP(h, hipSetDevice(h->device));
    const zk_status ss = snap_scratch(h);
    if (ss != ZK_OK) return ss;
    const uint64_t cells = h->cells;
    unsigned long long* nz = h->s_cell;
    unsigned long long* present = h->s_cell + cells;
    unsigned long long* sum = h->s_cell + 2 * cells;
    const uint32_t grid = (uint32_t)((cells + 3) / 4);
    LH_HIP(h, hipEventRecord(h->s_ev[0], h->stream));
    LH_HIP(h, launch_checked("k_lh_snap_count", k_lh_snap_count, dim3(grid), dim3(256), 0, h->stream,
                             (const uint32_t*)h->hist, cells, h->bins, nz, present, sum));
    // inclusive scans in place (u64): entries before and in each cell, rows up to it, links up to it
    for (unsigned long long* a : {nz, present, sum})
        LH_HIP(h, hipcub::DeviceScan::InclusiveSum(h->s_tmp, h->s_tmp_bytes, a, a, (int)cells, h->stream));
    LH_HIP(h, hipEventRecord(h->s_ev[1], h->stream));
    unsigned long long tot[3] = {0, 0, 0}, dropped = 0;  // entries, rows, links
    for (int k = 0; k < 3; ++k)
        LH_HIP(h, hipMemcpyAsync(&tot[k], h->s_cell + (uint64_t)k * cells + cells - 1, 8, hipMemcpyDeviceToHost, h->stream));
    LH_HIP(h, hipMemcpyAsync(&dropped, h->dropped, 8, hipMemcpyDeviceToHost, h->stream));
    LH_HIP(h, hipStreamSynchronize(h->stream));
    const uint64_t body = tot[1] * 16 + tot[0] * 8;
    *bytes = sizeof(LhSnapHeader) + body;
    if (!out) return ZK_OK;
    if (cap < *bytes) return hfail(h, ZK_ERR_CAPACITY, "output capacity smaller than the snapshot");
    const zk_status bs = snap_blob(h, body);
    if (bs != ZK_OK) return bs;
    LhSnapRow* rows = (LhSnapRow*)h->s_blob;
    unsigned long long* entries = (unsigned long long*)(h->s_blob + tot[1] * 16);
    if (tot[1])
        LH_HIP(h, launch_checked("k_lh_snap_write", k_lh_snap_write, dim3(grid), dim3(256), 0, h->stream,
                                 (const uint32_t*)h->hist, cells, h->bins, h->S, (const unsigned long long*)nz,
                                 (const unsigned long long*)present, rows, tot[1], entries, tot[0]));
    LH_HIP(h, hipEventRecord(h->s_ev[2], h->stream));
    if (body)
        LH_HIP(h, hipMemcpyAsync((uint8_t*)out + sizeof(LhSnapHeader), h->s_blob, body, hipMemcpyDeviceToHost, h->stream));
    LH_HIP(h, hipEventRecord(h->s_ev[3], h->stream));
    LH_HIP(h, hipStreamSynchronize(h->stream));
    LhSnapHeader hd{};
    hd.magic = kLhSnapMagic;
    hd.version = ZK_LH_SNAPSHOT_VERSION;
    hd.m = h->m;
    hd.bins = h->bins;
    hd.rows = tot[1];
    hd.entries = tot[0];
    hd.links = tot[2];
    hd.dropped = dropped;
    memcpy(out, &hd, sizeof hd);
    h->s_timed = true;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_lh_snapshot_ms(zk_lh* h, double out[3]) {
    ZK_GUARD_BEGIN
    if (!h || !out) return ZK_ERR_INVALID_ARG;
    if (!h->s_timed) return hfail(h, ZK_ERR_INVALID_ARG, "no snapshot written yet");
    LH_HIP(h, hipSetDevice(h->device));
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        LH_HIP(h, hipEventElapsedTime(&ms, h->s_ev[k], h->s_ev[k + 1]));
        out[k] = ms;
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_lh_merge(zk_lh* h, const void* blob, uint64_t bytes) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    // everything that can refuse the blob comes before the first copy or launch
    LhSnapView v;
    if (!lh_snap_view(blob, bytes, &v)) return hfail(h, ZK_ERR_INVALID_ARG, "malformed snapshot");
    if (v.h.m != h->m) return hfail(h, ZK_ERR_INVALID_ARG, "snapshot and handle differ in sub_bits");
    for (uint64_t r = 0; r < v.h.rows; ++r) {
        const LhSnapRow row = v.row(r);
        if (row.parent >= h->S || row.child >= h->S) return hfail(h, ZK_ERR_SERVICE_RANGE, "snapshot row with a service id >= num_services");
    }
    if (v.h.links > kMaxRecordsSinceReset || h->reserved + v.h.links > kMaxRecordsSinceReset)
        return hfail(h, ZK_ERR_CAPACITY, "link histogram: more than 2^32-1 records and merged links since its reset");
    if (!v.h.rows && !v.h.dropped) return ZK_OK;
    LH_HIP(h, hipSetDevice(h->device));
    const uint64_t body = bytes - sizeof(LhSnapHeader);
    const zk_status bs = snap_blob(h, body);
    if (bs != ZK_OK) return bs;
    if (body)
        LH_HIP(h, hipMemcpyAsync(h->s_blob, (const uint8_t*)blob + sizeof(LhSnapHeader), body, hipMemcpyHostToDevice, h->stream));
    const uint32_t grid = v.h.rows ? (uint32_t)((v.h.rows + 3) / 4) : 1u;
    LH_HIP(h, launch_checked("k_lh_merge", k_lh_merge, dim3(grid), dim3(256), 0, h->stream, h->hist, h->bins, h->S,
                             (const LhSnapRow*)h->s_blob, (unsigned long long)v.h.rows,
                             (const unsigned long long*)(h->s_blob + v.h.rows * 16), (unsigned long long)v.h.entries,
                             (unsigned long long)v.h.dropped, h->dropped));
    h->reserved += v.h.links;
    LH_HIP(h, hipStreamSynchronize(h->stream));  // (the blob is borrowed, and s_blob is reused by the next call)
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_lh_partial(zk_lh* h, void** hist, uint64_t* bytes) {
    if (!h || !hist || !bytes) return ZK_ERR_INVALID_ARG;
    *hist = h->hist;
    *bytes = h->cells * h->bins * 4;
    return ZK_OK;
}

zk_status zk_lh_dropped(zk_lh* h, uint64_t* duration_range) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    LH_HIP(h, hipSetDevice(h->device));
    unsigned long long d = 0;
    LH_HIP(h, hipMemcpyAsync(&d, h->dropped, 8, hipMemcpyDeviceToHost, h->stream));
    LH_HIP(h, hipStreamSynchronize(h->stream));
    if (duration_range) *duration_range = d;
    return ZK_OK;
    ZK_GUARD_END
}

}  // extern "C"
