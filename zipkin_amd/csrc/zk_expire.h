// zk_expire.h — the device side of the segment indices' expiry (zk_seg_index.h's seg_expire(), which
// includes this file and checks its constants against the indices'; the kernels are the wrappers
// k_ix_expire_* in zk_ix.hip and k_ax_expire_* in zk_ax.hip): a workgroup's stretch of a segment, the
// services it touches, and the two passes' bodies.
//
// An entry's service is not stored: a segment's entries are grouped by service and the host keeps
// off[S + 1]. The passes get a copy of every segment's offsets (u32: a handle holds fewer than 2^32
// entries) and a list of work items (segment, chunk): workgroup w owns entries [chunk * c, chunk * (c + 1))
// of its segment. It resolves ONCE the first and the last service of that stretch (two binary searches
// over the segment's offsets, by two threads), copies the offsets between them into LDS, and a lane then
// finds its entry's service by a search over that LDS range only: zero steps when the stretch lies inside
// one service's slice, log2 of the services the stretch touches otherwise (all 4096 of them when they are
// short or empty). LDS bins are indexed by the service's place in the range, s - s_lo.
//
//   exp_count    survivors per (segment, service): the tkey column only (8 B per entry); hist_add into the
//                workgroup's bins, one atomicAdd per (workgroup, service with survivors)
//   exp_rewrite  the stretch walked twice, as k_ix_scatter walks its own: the survivors' histogram, ONE
//                returning atomic per workgroup and service to claim places behind the new segment's
//                cursor, then every survivor again with its rank from hist_rank; `put` copies the entry's
//                other columns. tkey is read twice, the other columns for survivors only.
//
// An entry survives when tkey >= cut (tkey = ts ^ sign, so the unsigned order is the signed one). Every
// store is bounded: a count goes to surv[seg * S + s] with s < S, a survivor to a place below the new
// segment's size. The loops' bounds are the same for all threads of a workgroup, so every lane reaches
// the ballots and the barriers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zk_hist.h"

namespace zk {

constexpr int kExpWG = 256;
constexpr int kExpItems = 4;                          // the counting loops: entries per thread and step
constexpr uint32_t kExpTile = kExpWG * kExpItems;
constexpr uint32_t kExpBins = 4096;                   // ZK_IX_MAX_SERVICES = ZK_AX_MAX_SERVICES
constexpr uint32_t kExpPerWG = 16384;                 // entries per workgroup at least (k_ix_scatter's stretch)
constexpr uint32_t kExpMaxItems = 4096;               // work items of one pass at most, plus one per segment

// a segment as the passes see it: its first column (the others lie behind it, see the handles' Segment),
// its size and its offsets[S + 1] on the device
struct ExpSeg {
    const unsigned long long* tkey;
    unsigned long long n;
    const uint32_t* off;
};
struct ExpItem {
    uint32_t seg, chunk;
};
static_assert(sizeof(ExpSeg) == 24 && sizeof(ExpItem) == 8, "the plan's layouts");

// the LDS of a pass
struct ExpLds {
    uint32_t off[kExpBins + 1];  // the offsets of the stretch's services, off[0] <= lo
    uint32_t cnt[kExpBins];      // survivors per service of the range, then the ranks given out
    uint32_t rng[2];             // the stretch's first and last service
};

// the last service whose offset is <= i (off[0] = 0 <= i < n = off[S]): the ones behind it that share the
// offset are empty
__device__ inline uint32_t exp_service_of(const uint32_t* __restrict__ off, uint32_t S, unsigned long long i) {
    uint32_t a = 0, b = S;
    while (b - a > 1) {
        const uint32_t mid = (a + b) >> 1;
        if ((unsigned long long)off[mid] <= i) a = mid; else b = mid;
    }
    return a;
}

// Resolve the stretch [lo, hi) of sg (lo < hi <= sg.n): lds->off[0 .. ns] = sg.off[s_lo .. s_lo + ns],
// lds->cnt[0 .. ns) = 0. Returns ns, the services in the range; *s_lo its first. Ends with a barrier.
__device__ inline uint32_t exp_resolve(const ExpSeg& sg, uint32_t S, unsigned long long lo, unsigned long long hi, ExpLds* lds,
                                       uint32_t* s_lo) {
    if (threadIdx.x == 0) lds->rng[0] = exp_service_of(sg.off, S, lo);
    if (threadIdx.x == 64) lds->rng[1] = exp_service_of(sg.off, S, hi - 1ull);
    __syncthreads();
    const uint32_t first = lds->rng[0], last = lds->rng[1];
    uint32_t ns = last >= first ? last - first + 1u : 1u;
    if (ns > S - first) ns = S - first;  // (first < S; offsets that do not rise would break it otherwise)
    for (uint32_t b = threadIdx.x; b <= ns; b += kExpWG) lds->off[b] = sg.off[first + b];
    for (uint32_t b = threadIdx.x; b < ns; b += kExpWG) lds->cnt[b] = 0u;
    __syncthreads();
    *s_lo = first;
    return ns;
}

// the place in the range of entry i's service (lds->off[0] <= lo <= i)
__device__ inline uint32_t exp_place(const ExpLds* lds, uint32_t ns, unsigned long long i) {
    uint32_t a = 0, b = ns;
    while (b - a > 1) {
        const uint32_t mid = (a + b) >> 1;
        if ((unsigned long long)lds->off[mid] <= i) a = mid; else b = mid;
    }
    return a;
}

// surv[seg * S + s] += the entries of service s in the item's stretch with tkey >= cut
__device__ inline void exp_count(const ExpSeg* __restrict__ segs, const ExpItem* __restrict__ items, unsigned long long chunk,
                                 uint32_t S, unsigned long long cut, uint32_t* __restrict__ surv, ExpLds* lds) {
    const ExpItem it = items[blockIdx.x];
    const ExpSeg sg = segs[it.seg];
    const unsigned long long lo = (unsigned long long)it.chunk * chunk;
    if (lo >= sg.n) return;  // (the same for the whole workgroup)
    const unsigned long long hi = lo + chunk < sg.n ? lo + chunk : sg.n;
    uint32_t s_lo = 0;
    const uint32_t ns = exp_resolve(sg, S, lo, hi, lds, &s_lo);
    for (unsigned long long base = lo; base < hi; base += kExpTile) {
        unsigned long long k[kExpItems];  // (the tile's loads first, then the ballots)
#pragma unroll
        for (int j = 0; j < kExpItems; ++j) {
            const unsigned long long i = base + (unsigned long long)j * kExpWG + threadIdx.x;
            k[j] = i < hi ? sg.tkey[i] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < kExpItems; ++j) {
            const unsigned long long i = base + (unsigned long long)j * kExpWG + threadIdx.x;
            const bool alive = i < hi && k[j] >= cut;
            hist_add(lds->cnt, alive, alive ? exp_place(lds, ns, i) : 0u);
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < ns; b += kExpWG) {
        const uint32_t c = lds->cnt[b];
        if (c && s_lo + b < S) atomicAdd(&surv[(size_t)it.seg * S + s_lo + b], c);
    }
}

// The item's survivors into the new segment: cursor[s] starts at the new segment's off[s], `total` is its
// size; put(sg, i, tkey, at) copies entry i of sg to place `at` (at < total). s_base: kExpBins words of
// LDS, where the workgroup's places of a service begin.
template <class Put>
__device__ inline void exp_rewrite(const ExpSeg* __restrict__ segs, const ExpItem* __restrict__ items, unsigned long long chunk,
                                   uint32_t S, unsigned long long cut, uint32_t* __restrict__ cursor, unsigned long long total,
                                   const Put& put, ExpLds* lds, uint32_t* s_base) {
    const ExpItem it = items[blockIdx.x];
    const ExpSeg sg = segs[it.seg];
    const unsigned long long lo = (unsigned long long)it.chunk * chunk;
    if (lo >= sg.n) return;  // (the same for the whole workgroup)
    const unsigned long long hi = lo + chunk < sg.n ? lo + chunk : sg.n;
    uint32_t s_lo = 0;
    const uint32_t ns = exp_resolve(sg, S, lo, hi, lds, &s_lo);
    for (unsigned long long base = lo; base < hi; base += kExpTile) {
        unsigned long long k[kExpItems];
#pragma unroll
        for (int j = 0; j < kExpItems; ++j) {
            const unsigned long long i = base + (unsigned long long)j * kExpWG + threadIdx.x;
            k[j] = i < hi ? sg.tkey[i] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < kExpItems; ++j) {
            const unsigned long long i = base + (unsigned long long)j * kExpWG + threadIdx.x;
            const bool alive = i < hi && k[j] >= cut;
            hist_add(lds->cnt, alive, alive ? exp_place(lds, ns, i) : 0u);
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < ns; b += kExpWG) {
        const uint32_t c = lds->cnt[b];
        if (c && s_lo + b < S) s_base[b] = atomicAdd(&cursor[s_lo + b], c);
        lds->cnt[b] = 0u;
    }
    __syncthreads();
    for (unsigned long long base = lo; base < hi; base += kExpWG) {
        const unsigned long long i = base + threadIdx.x;
        const unsigned long long k = i < hi ? sg.tkey[i] : 0ull;
        const bool alive = i < hi && k >= cut;
        const uint32_t b = alive ? exp_place(lds, ns, i) : 0u;
        const uint32_t rank = hist_rank(lds->cnt, alive, b);
        if (alive) {
            const unsigned long long at = (unsigned long long)s_base[b] + rank;
            if (at < total) put(sg, i, k, at);
        }
    }
}

}  // namespace zk
