// zk_hist.h — the LDS histogram adds of the segment indices (zk_ix.hip, zk_ax.hip): lanes of a wave that
// share a bin are peeled off by ballot and added once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zk {

constexpr int kPeel = 4;

__device__ inline uint32_t lane_id() { return threadIdx.x & 63; }

__device__ inline uint32_t rank_in(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// s_hist[bin] += 1 for every lane with todo. A batch of few services puts most of a wave into one bin
// and LDS atomics on one address serialise: the wave first peels off, up to kPeel times, the lanes that
// share the lowest active lane's bin and adds their number once; the rest add one each. Every lane of
// the wave calls it.
__device__ inline void hist_add(uint32_t* s_hist, bool todo, uint32_t bin) {
    for (int r = 0; r < kPeel; ++r) {
        const unsigned long long m = __ballot(todo);
        if (!m) break;
        const int lead = __ffsll((long long)m) - 1;
        const uint32_t lb = __shfl(bin, lead);
        const unsigned long long same = __ballot(todo && bin == lb);
        if ((int)lane_id() == lead) atomicAdd(&s_hist[lb], (uint32_t)__popcll(same));
        if (bin == lb) todo = false;
    }
    if (todo) atomicAdd(&s_hist[bin], 1u);
}

// the same with the old value back: the lane's own place among the adds to its bin (lanes without todo
// get nothing meaningful)
__device__ inline uint32_t hist_rank(uint32_t* s_hist, bool todo, uint32_t bin) {
    uint32_t rank = 0;
    for (int r = 0; r < kPeel; ++r) {
        const unsigned long long m = __ballot(todo);
        if (!m) break;
        const int lead = __ffsll((long long)m) - 1;
        const uint32_t lb = __shfl(bin, lead);
        const bool mine = todo && bin == lb;
        const unsigned long long same = __ballot(mine);
        uint32_t base = 0;
        if ((int)lane_id() == lead) base = atomicAdd(&s_hist[lb], (uint32_t)__popcll(same));
        base = __shfl(base, lead);
        if (mine) {
            rank = base + rank_in(same);
            todo = false;
        }
    }
    if (todo) rank = atomicAdd(&s_hist[bin], 1u);
    return rank;
}

}  // namespace zk
