// zk_lh_internal.h — glue of the per-link duration histogram (zk_lh.hip) used by zk_api.cpp and
// zk_comm.cpp.
#pragma once
#include "zk_internal.h"
#include "zksketch.h"

struct zk_comm;

namespace zk {
// point the spill kernel's JoinArgs at the histogram (its links bypass the link lists)
void lh_join_args(zk_lh* h, JoinArgs* a);
// the duration-range counter of the ctx's stats shards before (sign = -1) and after (+1) a batch:
// the difference is what the batch dropped, added to the handle's own counter
hipError_t lh_note_dropped(zk_lh* h, const unsigned long long* stats, int sign);
// the batch's links into the histogram, after the link reduce: the bucket-ordered copy K2 left in
// r.sorted (r.nb != 0), else the K1 lists themselves
hipError_t lh_accumulate(zk_lh* h, const ReduceArgs& r);
// records accumulated since the handle's reset (an upper bound of its links), and n more of them
uint64_t lh_reserved(const zk_lh* h);
void lh_reserve(zk_lh* h, uint64_t n);
int lh_device(const zk_lh* h);
uint32_t lh_services(const zk_lh* h);
void lh_set_stream(zk_lh* h, hipStream_t s);  // nullptr: back to the handle's own stream
// u32 SUM of the histogram (and u64 SUM of the drop counter) across the communicator's ranks
zk_status lh_allreduce(zk_lh* h, zk_comm* comm);
// cells per LDS tile (log2) of the accumulate kernel for `bins` bins and buckets of 2^cb_shift cells
uint32_t lh_tile_shift(uint32_t bins, uint32_t cb_shift);
}  // namespace zk
