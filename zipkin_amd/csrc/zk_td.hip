// zk_td.hip — the trace duration index (include/zkduration.h): traceId -> (start, end) in one HBM
// table, and the radix select of the first k traces by duration or start.
//
// The table is the trace-time table of zk_win.hip with a third word: open addressing, linear probing,
// 24 B per slot {key, start, end}; key 0 = empty, start / end = the times with the sign bit flipped;
// a fresh slot holds start = all ones and end = 0. slots is a power of two; traceId 0 lives in the
// extra slot at index `slots`, its key word a presence flag. The host keeps the load at or below 1/2
// (it sizes the table from k_td_runs' count BEFORE anything is inserted), so a probe always meets an
// empty slot; every probe loop is bounded by `slots` all the same and reports to tstat[kTsFull]
// instead of spinning.
//
// Why plain loads are safe in k_td_observe: within a table's life a key never changes once set, a
// start only falls and an end only rises. So whatever a plain (possibly stale, possibly torn: three
// separate 8-B words) load returns, a non-zero key is the slot's key for good, the start word is an
// upper bound of the slot's start and the end word a lower bound of its end. "stored start <= ours:
// skip the atomicMin" and "stored end >= ours: skip the atomicMax" are therefore safe (the true words
// are at least as extreme), a stale value on the other side only costs an atomic that changes nothing,
// and an empty-looking slot is settled by the CAS. The atomics are device scope, executed at the memory
// side on a hipMalloc'd table, and never see a cache. Clear, rehash and the reads of the queries are
// separate kernels on the same stream.
//
//   k_td_runs     the batch's run starts; the host sizes the table by them before anything is inserted
//   k_td_observe  one table update per (run, row of 64 records): a probe, at most one CAS on the key, at
//                 most one atomicMin on start and one atomicMax on end
//   k_td_rehash   the old table's entries into a grown one; k_td_clear empties a table
//   k_td_expire_count, k_td_expire_move   zk_td_expire: the traces that stay, then (when some go) the
//                 stayers into a fresh table sized for them (see there)
//   k_td_query    zk_td_lookup
//   k_td_scan, k_td_hist, k_td_collect   zk_td_top's passes (see there)
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>
#include <vector>

#include "zk_guard.h"
#include "zk_launch.h"
#include "zk_td_select.h"
#include "zk_tracegen.h"
#include "zkduration.h"

namespace zk {
namespace {

constexpr unsigned long long kTdSalt = ZK_TD_TABLE_SALT;
constexpr unsigned long long kAllOnes = ~0ull;
constexpr uint64_t kTdMinSlots = 1024;
constexpr uint64_t kTdMaxSlots = 1ull << 40;
constexpr uint64_t kTdMaxRecords = 1ull << 40;
constexpr int kTdWG = 256;
constexpr uint32_t kTdMaxGrid = 4096;
constexpr uint32_t kTdHistGrid = 1024;  // k_td_hist: every workgroup flushes up to 4096 bins
constexpr uint32_t kTdCap = ZK_TD_MAX_TOP;  // the most entries the select brings to the host
enum { kTsTraces = 0, kTsRuns = 1, kTsFull = 2, kTsAlive = 3, kTsWords = 4 };
// the select's counters: matched, certain entries appended, then what a round zeroes: the OR of the
// keys and of their complements (hi, lo) over the entries that stay candidates, and their number
enum { kSelMatched = 0, kSelCertain = 1, kSelOrHi = 2, kSelNorHi = 3, kSelOrLo = 4, kSelNorLo = 5, kSelCand = 6, kSelWords = 8 };
constexpr size_t kSelHistAt = 256;                         // byte offsets in the select's scratch block
constexpr size_t kSelCertainAt = kSelHistAt + kTdBins * 4;
constexpr size_t kSelBytes = kSelCertainAt + (size_t)kTdCap * sizeof(TdEntry);

static_assert(sizeof(TdEntry) == 24, "a slot is three 8-B words");
static_assert(kSelWords * 8 <= kSelHistAt && kSelCertainAt % 8 == 0, "the scratch block's layout");

__device__ inline uint32_t lane_id() { return threadIdx.x & 63; }

__device__ inline unsigned long long td_home(unsigned long long id, unsigned long long slots) {
    return zk_mix64(id ^ kTdSalt) & (slots - 1ull);
}

uint32_t td_grid(uint64_t items) {
    const uint64_t g = (items + kTdWG - 1) / kTdWG;
    return (uint32_t)(g < 1 ? 1 : g > kTdMaxGrid ? kTdMaxGrid : g);
}

// ---- the table ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTdWG) void k_td_clear(unsigned long long* __restrict__ tab, unsigned long long count) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kTdWG;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kTdWG + threadIdx.x; i < count; i += stride) {
        tab[3 * i] = 0ull;
        tab[3 * i + 1] = kAllOnes;
        tab[3 * i + 2] = 0ull;
    }
}

// the batch's run starts, into tstat[kTsRuns] (zeroed by the host before)
__global__ __launch_bounds__(kTdWG) void k_td_runs(const unsigned long long* __restrict__ tid, unsigned long long n,
                                                   unsigned long long* __restrict__ tstat) {
    __shared__ unsigned long long s_sum;
    const int t = threadIdx.x;
    if (t == 0) s_sum = 0ull;
    __syncthreads();
    const unsigned long long stride = (unsigned long long)gridDim.x * kTdWG;
    unsigned long long c = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kTdWG + t; i < n; i += stride)
        c += i == 0 || tid[i - 1] != tid[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if (lane_id() == 0 && c) atomicAdd(&s_sum, c);
    __syncthreads();
    if (t == 0 && s_sum) atomicAdd(&tstat[kTsRuns], s_sum);
}

// the old table's entries into the grown one: keys are unique, so the thread that claims a key is the
// only writer of its two times
__global__ __launch_bounds__(kTdWG) void k_td_rehash(const unsigned long long* __restrict__ old, unsigned long long old_slots,
                                                     unsigned long long* __restrict__ tab, unsigned long long slots,
                                                     unsigned long long* __restrict__ tstat) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kTdWG;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kTdWG + threadIdx.x; i <= old_slots; i += stride) {
        const unsigned long long key = old[3 * i], sk = old[3 * i + 1], ek = old[3 * i + 2];
        if (key == 0ull) continue;
        if (i == old_slots) {  // traceId 0
            tab[3 * slots] = 1ull;
            tab[3 * slots + 1] = sk;
            tab[3 * slots + 2] = ek;
            continue;
        }
        unsigned long long s = td_home(key, slots), tries = 0;
        for (; tries < slots; ++tries) {
            if (atomicCAS(&tab[3 * s], 0ull, key) == 0ull) {
                tab[3 * s + 1] = sk;
                tab[3 * s + 2] = ek;
                break;
            }
            s = (s + 1ull) & (slots - 1ull);
        }
        if (tries == slots) atomicAdd(&tstat[kTsFull], 1ull);
    }
}

// ---- expiry --------------------------------------------------------------------------------------------
// Linear probing has no delete in place: emptying a slot cuts the probe chain of every key that was
// displaced past it. zk_td_expire so counts the traces that stay (k_td_expire_count) and, when some go,
// moves the stayers into a fresh table sized for them (k_td_expire_move: k_td_rehash with the predicate).
// A trace stays when its end key is >= cut; the slot of traceId 0 follows the same rule.
__global__ __launch_bounds__(kTdWG) void k_td_expire_count(const unsigned long long* __restrict__ tab, unsigned long long slots,
                                                           unsigned long long cut, unsigned long long* __restrict__ tstat) {
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) s_sum = 0ull;
    __syncthreads();
    const unsigned long long stride = (unsigned long long)gridDim.x * kTdWG;
    unsigned long long c = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kTdWG + threadIdx.x; i <= slots; i += stride)
        c += tab[3 * i] != 0ull && tab[3 * i + 2] >= cut;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if (lane_id() == 0 && c) atomicAdd(&s_sum, c);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(&tstat[kTsAlive], s_sum);
}

// the old table's entries with end key >= cut into the fresh one (cleared, at load <= 1/2 for them): keys
// are unique, so the thread that claims a key is the only writer of its two times
__global__ __launch_bounds__(kTdWG) void k_td_expire_move(const unsigned long long* __restrict__ old, unsigned long long old_slots,
                                                          unsigned long long cut, unsigned long long* __restrict__ tab,
                                                          unsigned long long slots, unsigned long long* __restrict__ tstat) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kTdWG;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kTdWG + threadIdx.x; i <= old_slots; i += stride) {
        const unsigned long long key = old[3 * i], sk = old[3 * i + 1], ek = old[3 * i + 2];
        if (key == 0ull || ek < cut) continue;
        if (i == old_slots) {  // traceId 0
            tab[3 * slots] = 1ull;
            tab[3 * slots + 1] = sk;
            tab[3 * slots + 2] = ek;
            continue;
        }
        unsigned long long s = td_home(key, slots), tries = 0;
        for (; tries < slots; ++tries) {
            if (atomicCAS(&tab[3 * s], 0ull, key) == 0ull) {
                tab[3 * s + 1] = sk;
                tab[3 * s + 2] = ek;
                break;
            }
            s = (s + 1ull) & (slots - 1ull);
        }
        if (tries == slots) atomicAdd(&tstat[kTsFull], 1ull);
    }
}

// start[id] = min(start[id], smin), end[id] = max(end[id], emax), id entering the table when it is new;
// true when this call claimed it. The plain loads: see the head of the file.
__device__ inline bool td_update(unsigned long long* __restrict__ tab, unsigned long long slots, unsigned long long id,
                                 unsigned long long smin, unsigned long long emax, unsigned long long* __restrict__ tstat) {
    const unsigned long long want = id ? id : 1ull;
    unsigned long long s = id ? td_home(id, slots) : slots;
    for (unsigned long long tries = 0; tries < slots; ++tries) {
        unsigned long long* p = tab + 3 * s;
        unsigned long long k = p[0];
        const unsigned long long sk = p[1], ek = p[2];
        bool claimed = false;
        if (k == 0ull) {
            k = atomicCAS(p, 0ull, want);
            claimed = k == 0ull;
            if (claimed) k = want;
        }
        if (k == want) {
            if (sk > smin) atomicMin(p + 1, smin);
            if (ek < emax) atomicMax(p + 2, emax);
            return claimed;
        }
        s = (s + 1ull) & (slots - 1ull);
    }
    atomicAdd(&tstat[kTsFull], 1ull);
    return false;
}

__device__ inline bool td_find(const unsigned long long* __restrict__ tab, unsigned long long slots, unsigned long long id,
                               unsigned long long* sk, unsigned long long* ek) {
    if (slots == 0ull) return false;
    if (id == 0ull) {
        *sk = tab[3 * slots + 1];
        *ek = tab[3 * slots + 2];
        return tab[3 * slots] != 0ull;
    }
    unsigned long long s = td_home(id, slots);
    for (unsigned long long tries = 0; tries < slots; ++tries) {
        const unsigned long long k = tab[3 * s];
        if (k == id) {
            *sk = tab[3 * s + 1];
            *ek = tab[3 * s + 2];
            return true;
        }
        if (k == 0ull) return false;
        s = (s + 1ull) & (slots - 1ull);
    }
    return false;
}

// the row's pieces of runs: lanes [s, e] around this lane with equal traceId (lane 0 starts a piece
// whatever came before the row); lane s gets the minimum start key and the maximum end key over the
// piece (untimed lanes bring all ones / 0, which never win)
struct TdPiece {
    uint32_t s;
    bool any_timed;
    unsigned long long smin, emax;
};

__device__ inline TdPiece td_row_piece(unsigned long long mask, bool timed, unsigned long long skey, unsigned long long ekey) {
    const uint32_t lane = lane_id();
    const unsigned long long mm = mask & (~0ull >> (63 - lane));
    const unsigned long long above = lane == 63 ? 0ull : mask & (~0ull << (lane + 1));
    TdPiece p;
    p.s = mm ? 63u - (uint32_t)__clzll((long long)mm) : 0u;
    const uint32_t e = above ? (uint32_t)__ffsll((long long)above) - 2u : 63u;
    const unsigned long long seg = (~0ull >> (63 - e)) & (~0ull << p.s);
    p.any_timed = (__ballot(timed) & seg) != 0ull;
    p.smin = skey;
    p.emax = ekey;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long os = __shfl_down(p.smin, off);
        const unsigned long long oe = __shfl_down(p.emax, off);
        if (lane + off <= e) {
            if (os < p.smin) p.smin = os;
            if (oe > p.emax) p.emax = oe;
        }
    }
    return p;
}

// one table update per (run, row of 64 records); a wave walks rows
__global__ __launch_bounds__(kTdWG) void k_td_observe(const unsigned long long* __restrict__ tid,
                                                      const long long* __restrict__ first, const long long* __restrict__ last,
                                                      const uint32_t* __restrict__ fl, unsigned long long n,
                                                      unsigned long long* __restrict__ tab, unsigned long long slots,
                                                      unsigned long long* __restrict__ tstat) {
    const uint32_t lane = lane_id();
    const unsigned long long waves = (unsigned long long)gridDim.x * (kTdWG / 64);
    const unsigned long long rows = (n + 63ull) / 64ull;
    uint32_t claimed = 0;
    for (unsigned long long row = (unsigned long long)blockIdx.x * (kTdWG / 64) + (threadIdx.x >> 6); row < rows;
         row += waves) {
        const unsigned long long i = row * 64ull + lane;
        const bool valid = i < n;
        const unsigned long long id = valid ? tid[i] : 0ull;
        const unsigned long long prev = valid && lane > 0 ? tid[i - 1] : 0ull;
        const uint32_t f = valid ? fl[i] : 0u;
        const long long a = valid ? first[i] : 0ll;
        const long long b = valid ? last[i] : 0ll;
        const bool timed = (f & ZK_F_HAS_ANNOTATIONS) != 0u;
        const unsigned long long mask = __ballot(valid && (lane == 0 || id != prev));
        const TdPiece p = td_row_piece(mask, timed, timed ? (unsigned long long)a ^ kTdSign : kAllOnes,
                                       timed ? (unsigned long long)b ^ kTdSign : 0ull);
        bool c = false;
        if (valid && lane == p.s && p.any_timed) c = td_update(tab, slots, id, p.smin, p.emax, tstat);
        claimed += (uint32_t)__popcll(__ballot(c));
    }
    if (lane == 0 && claimed) atomicAdd(&tstat[kTsTraces], (unsigned long long)claimed);
}

// zk_td_lookup
__global__ __launch_bounds__(kTdWG) void k_td_query(const unsigned long long* __restrict__ ids, unsigned long long n,
                                                    const unsigned long long* __restrict__ tab, unsigned long long slots,
                                                    long long* __restrict__ start_out, long long* __restrict__ dur_out,
                                                    uint8_t* __restrict__ found_out) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kTdWG;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kTdWG + threadIdx.x; i < n; i += stride) {
        unsigned long long sk = kAllOnes, ek = 0ull;
        const bool found = td_find(tab, slots, ids[i], &sk, &ek);
        start_out[i] = (long long)(sk ^ kTdSign);
        dur_out[i] = (long long)td_duration(sk, ek);
        found_out[i] = found ? 1 : 0;
    }
}

// ---- the select ----------------------------------------------------------------------------------------
// zk_td_top finds the first k entries by the 128-bit key (order key, traceId) without sorting the table:
//   k_td_scan     over the table: the start-range filter, the number of matching entries and the OR of
//                 their keys and of the keys' complements, whose AND is the set of bits in which the
//                 matching keys differ;
//   k_td_hist     a 4096-bin histogram of the 12-bit digit that starts at the highest differing bit (so
//                 the bins always split the entries), per workgroup in LDS, flushed with atomics;
//   (host)        the bin in which the running count crosses the k still wanted;
//   k_td_collect  appends the entries below that bin to the CERTAIN list (they are in the answer) and
//                 the entries in it to a CANDIDATE list, and gathers the differing bits of the candidates
//                 for the next round.
// The table is so read three times at most (twice when everything that matches fits the host's cap).
// While certain + candidates exceed the cap the hist / collect pair repeats over the candidate list
// alone, which shrinks every round; every round consumes the next differing bits of the 128, so after
// at most 11 rounds the candidates differ in nothing, and traceIds are unique.
struct TdSrc {
    const unsigned long long* w;  // entries of three words
    unsigned long long count;     // entries to read
    unsigned long long zero_at;   // the table: the index of traceId 0's slot (= slots); a list: no such index
    unsigned long long lo, hi;    // start keys taken (a list: everything)
    uint32_t table;               // 1: word 0 is a slot's key (0 = empty), 0: it is the traceId
};

__device__ inline bool td_src_load(const TdSrc& s, unsigned long long i, TdEntry* e) {
    if (i >= s.count) return false;
    const unsigned long long k = s.w[3 * i];
    e->skey = s.w[3 * i + 1];
    e->ekey = s.w[3 * i + 2];
    e->id = s.table && i == s.zero_at ? 0ull : k;
    return (!s.table || k != 0ull) && e->skey >= s.lo && e->skey <= s.hi;
}

__device__ inline unsigned long long wave_or(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off);
    return v;
}

// the OR of the keys and of their complements over this thread's entries, folded into sel by one lane
// of every wave whose entries brought any
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

__global__ __launch_bounds__(kTdWG) void k_td_scan(TdSrc src, uint32_t order, unsigned long long* __restrict__ sel) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kTdWG;
    unsigned long long or_hi = 0, nor_hi = 0, or_lo = 0, nor_lo = 0, cnt = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kTdWG + threadIdx.x; i < src.count; i += stride) {
        TdEntry e;
        if (!td_src_load(src, i, &e)) continue;
        const unsigned long long hi = td_order_key(order, e.skey, e.ekey);
        or_hi |= hi;
        nor_hi |= ~hi;
        or_lo |= e.id;
        nor_lo |= ~e.id;
        ++cnt;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if (lane_id() == 0 && cnt) atomicAdd(&sel[kSelMatched], cnt);
    flush_bits(or_hi, nor_hi, or_lo, nor_lo, sel);
}

__global__ __launch_bounds__(kTdWG) void k_td_hist(TdSrc src, uint32_t order, uint32_t shift, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[kTdBins];
    for (uint32_t b = threadIdx.x; b < kTdBins; b += kTdWG) s_hist[b] = 0u;
    __syncthreads();
    // Few distinct keys (start times by the hour, a handful of durations) put most of a wave into one
    // bin, and LDS atomics on one address serialise: the wave first peels off, up to kPeel times, the
    // lanes that share the lowest active lane's bin and adds their number once; the rest add one each.
    constexpr int kPeel = 4;
    const unsigned long long stride = (unsigned long long)gridDim.x * kTdWG;
    for (unsigned long long base = (unsigned long long)blockIdx.x * kTdWG; base < src.count; base += stride) {
        TdEntry e{0, 0, 0};
        bool todo = td_src_load(src, base + threadIdx.x, &e);
        const uint32_t d = td_digit(td_order_key(order, e.skey, e.ekey), e.id, shift);
        for (int r = 0; r < kPeel; ++r) {
            const unsigned long long m = __ballot(todo);
            if (!m) break;
            const int lead = __ffsll((long long)m) - 1;
            const uint32_t ld = __shfl(d, lead);
            const unsigned long long same = __ballot(todo && d == ld);
            if ((int)lane_id() == lead) atomicAdd(&s_hist[ld], (uint32_t)__popcll(same));
            if (d == ld) todo = false;
        }
        if (todo) atomicAdd(&s_hist[d], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kTdBins; b += kTdWG) {
        const uint32_t c = s_hist[b];
        if (c) atomicAdd(&hist[b], c);
    }
}

// digit < bin: certain; digit == bin: a candidate (bin = kTdBins: every matching entry is certain).
// A workgroup walks tiles of kColTile entries, kColItems per thread. Each wave ranks its takers of both
// kinds with ballots, the workgroup sums its waves' counts in LDS and ONE thread per list draws the
// tile's stretch with a returning atomicAdd: one per 1024 entries and list. (One per wave was one per
// 64: with start times by the hour nearly every wave of the table holds a candidate, and a quarter of
// a million returning atomics on one word took longer than the table's bytes.) The loop's bounds are
// the same for all threads of a workgroup, so every lane reaches the ballots and the barriers.
constexpr int kColItems = 4;
constexpr uint32_t kColTile = kTdWG * kColItems;
constexpr int kColWaves = kTdWG / 64;

__device__ inline void put_entry(unsigned long long* __restrict__ out, unsigned long long cap, unsigned long long at,
                                 const TdEntry& e) {
    if (at < cap) {
        out[3 * at] = e.id;
        out[3 * at + 1] = e.skey;
        out[3 * at + 2] = e.ekey;
    }
}

__global__ __launch_bounds__(kTdWG) void k_td_collect(TdSrc src, uint32_t order, uint32_t shift, uint32_t bin,
                                                      unsigned long long* __restrict__ sel,
                                                      unsigned long long* __restrict__ certain, unsigned long long certain_cap,
                                                      unsigned long long* __restrict__ cand, unsigned long long cand_cap) {
    __shared__ uint32_t s_cnt[2][kColWaves];
    __shared__ unsigned long long s_base[2];
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const unsigned long long stride = (unsigned long long)gridDim.x * kColTile;
    unsigned long long or_hi = 0, nor_hi = 0, or_lo = 0, nor_lo = 0;
    for (unsigned long long tile = (unsigned long long)blockIdx.x * kColTile; tile < src.count; tile += stride) {
        TdEntry e[kColItems];
        uint32_t kind[kColItems], rank[kColItems];  // kind: 0 dropped, 1 certain, 2 candidate; rank in the wave's takers
        uint32_t wc = 0, ws = 0;                    // the wave's takers so far (wave-uniform)
#pragma unroll
        for (int j = 0; j < kColItems; ++j) {
            e[j] = TdEntry{0, 0, 0};
            const bool ok = td_src_load(src, tile + (unsigned long long)j * kTdWG + threadIdx.x, &e[j]);
            const unsigned long long hi = td_order_key(order, e[j].skey, e[j].ekey);
            const uint32_t d = td_digit(hi, e[j].id, shift);
            const bool below = ok && d < bin, stays = ok && d == bin;
            const unsigned long long mb = __ballot(below), ms = __ballot(stays);
            const unsigned long long mine = below ? mb : ms;
            kind[j] = below ? 1u : stays ? 2u : 0u;
            rank[j] = (below ? wc : ws) +
                      __builtin_amdgcn_mbcnt_hi((uint32_t)(mine >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mine, 0u));
            wc += (uint32_t)__popcll(mb);
            ws += (uint32_t)__popcll(ms);
            if (stays) {
                or_hi |= hi;
                nor_hi |= ~hi;
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

}  // namespace
}  // namespace zk

using namespace zk;

struct zk_td {
    int device = 0;
    hipStream_t stream = nullptr, own = nullptr;
    bool timing = false;
    void* table = nullptr;   // three u64 words [slots + 1]
    void* tstat = nullptr;   // u64 [kTsWords]: traces, the last batch's runs, probe loops that ran out, the last expiry's stayers
    void* stage = nullptr;   // the four columns of a host batch
    void* query = nullptr;   // zk_td_lookup: ids, starts, durations, found
    void* sel = nullptr;     // zk_td_top: counters, histogram, the certain list (kSelBytes)
    void* list[2] = {nullptr, nullptr};  // zk_td_top: the candidate lists, written in turn
    uint64_t slots = 0;
    size_t stage_bytes = 0, query_bytes = 0, sel_bytes = 0, list_bytes[2] = {0, 0};
    hipEvent_t oev[4] = {};  // around the passes of the last observe (zk_td_observe_ms)
    hipEvent_t tev[2] = {};  // around the last top (zk_td_top_ms)
    hipEvent_t xev[4] = {};  // around the passes of the last expiry (zk_td_expire_ms)
    bool otimed = false, ttimed = false, xtimed = false;
    std::string err;
};

namespace {

zk_status tfail(zk_td* h, zk_status s, const std::string& m) {
    if (h) h->err = m;
    return s;
}

#define TD_HIP(h, call)                                                                            \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess) return tfail(h, is_refusal(_e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP,       \
                                           std::string(#call) + ": " + launch_error_str(_e));      \
    } while (0)

// at least `need` bytes behind *p: a larger block first, then the old one freed; a refused allocation
// is ZK_ERR_CAPACITY and leaves *p as it was
zk_status grow(zk_td* h, void** p, size_t* have, size_t need, const char* what) {
    if (need <= *have && *p) return ZK_OK;
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, need ? need : 8);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (e != hipErrorOutOfMemory) return tfail(h, ZK_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        return tfail(h, ZK_ERR_CAPACITY, std::string("no device memory for ") + what);
    }
    if (*p) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(*p);
    }
    *p = q;
    *have = need;
    return ZK_OK;
}

zk_status ensure_tstat(zk_td* h) {
    if (h->tstat) return ZK_OK;
    void* q = nullptr;
    size_t have = 0;
    const zk_status st = grow(h, &q, &have, kTsWords * 8, "the table's counters");
    if (st != ZK_OK) return st;
    TD_HIP(h, hipMemsetAsync(q, 0, kTsWords * 8, h->stream));
    h->tstat = q;
    return ZK_OK;
}

// The table at `want` slots or more (a power of two, at least kTdMinSlots): a new table is made and
// cleared, the old one's entries move into it (k_td_rehash) and the old one is freed after the stream
// has drained. A refused allocation changes nothing.
zk_status ensure_slots(zk_td* h, uint64_t want) {
    if (want <= h->slots && h->table) return ZK_OK;
    if (want > kTdMaxSlots) return tfail(h, ZK_ERR_CAPACITY, "a duration table of more than 2^40 slots");
    uint64_t slots = kTdMinSlots;
    while (slots < want) slots <<= 1;
    zk_status st = ensure_tstat(h);
    if (st != ZK_OK) return st;
    void* q = nullptr;
    size_t have = 0;
    if ((st = grow(h, &q, &have, (size_t)(slots + 1) * sizeof(TdEntry), "the duration table (24 B per slot)")) != ZK_OK)
        return st;
    hipError_t e = launch_checked("k_td_clear", k_td_clear, dim3(td_grid(slots + 1)), dim3(kTdWG), 0, h->stream,
                                  (unsigned long long*)q, (unsigned long long)(slots + 1));
    if (e == hipSuccess && h->table)
        e = launch_checked("k_td_rehash", k_td_rehash, dim3(td_grid(h->slots + 1)), dim3(kTdWG), 0, h->stream,
                           (const unsigned long long*)h->table, (unsigned long long)h->slots, (unsigned long long*)q,
                           (unsigned long long)slots, (unsigned long long*)h->tstat);
    if (e == hipSuccess && h->table) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(q);
        return tfail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("growing the duration table: ") + launch_error_str(e));
    }
    if (h->table) (void)hipFree(h->table);
    h->table = q;
    h->slots = slots;
    return ZK_OK;
}

bool order_ok(uint32_t order) { return order <= ZK_TD_DURATION_DESC; }

}  // namespace

extern "C" {

zk_status zk_td_create(const zk_td_config* cfg, zk_td** out) {
    ZK_GUARD_BEGIN
    if (!cfg || !out) return ZK_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || cfg->device < 0 || cfg->device >= ndev) return ZK_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return ZK_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return ZK_ERR_NO_DEVICE;
    if (hipSetDevice(cfg->device) != hipSuccess) return ZK_ERR_HIP;
    zk_td* h = new zk_td();
    h->device = cfg->device;
    h->timing = cfg->timing != 0;
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

zk_status zk_td_destroy(zk_td* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void* p : {h->table, h->tstat, h->stage, h->query, h->sel, h->list[0], h->list[1]})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : h->oev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->tev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->xev)
        if (e) (void)hipEventDestroy(e);
    if (h->own) (void)hipStreamDestroy(h->own);
    delete h;
    return ZK_OK;
    ZK_GUARD_END
}

const char* zk_td_last_error(const zk_td* h) { return h ? h->err.c_str() : "null handle"; }

zk_status zk_td_observe(zk_td* h, const zk_span_cols* in, uint32_t flags) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!in) return tfail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (flags & ~(ZK_BATCH_DEVICE_PTRS | ZK_BATCH_TRACE_CLUSTERED)) return tfail(h, ZK_ERR_INVALID_ARG, "unknown batch flag");
    const uint64_t n = in->n;
    if (n > kTdMaxRecords) return tfail(h, ZK_ERR_UNSUPPORTED, "more than 2^40 records in one batch");
    if (n == 0) return ZK_OK;
    if (!in->trace_id || !in->first_ts || !in->last_ts || !in->flags) return tfail(h, ZK_ERR_INVALID_ARG, "null column");
    TD_HIP(h, hipSetDevice(h->device));
    zk_status st = ensure_tstat(h);
    if (st != ZK_OK) return st;
    const unsigned long long* tid = (const unsigned long long*)in->trace_id;
    const long long* first = (const long long*)in->first_ts;
    const long long* last = (const long long*)in->last_ts;
    const uint32_t* fl = in->flags;
    if (!(flags & ZK_BATCH_DEVICE_PTRS)) {
        // a host batch: the four columns the table reads, staged (each 256-B aligned)
        const size_t a8 = (n * 8 + 255) / 256 * 256, a4 = (n * 4 + 255) / 256 * 256;
        if ((st = grow(h, &h->stage, &h->stage_bytes, 3 * a8 + a4, "staging a host batch (28 B per record)")) != ZK_OK)
            return st;
        uint8_t* s = (uint8_t*)h->stage;
        TD_HIP(h, hipMemcpyAsync(s, in->trace_id, n * 8, hipMemcpyHostToDevice, h->stream));
        TD_HIP(h, hipMemcpyAsync(s + a8, in->first_ts, n * 8, hipMemcpyHostToDevice, h->stream));
        TD_HIP(h, hipMemcpyAsync(s + 2 * a8, in->last_ts, n * 8, hipMemcpyHostToDevice, h->stream));
        TD_HIP(h, hipMemcpyAsync(s + 3 * a8, in->flags, n * 4, hipMemcpyHostToDevice, h->stream));
        tid = (const unsigned long long*)s;
        first = (const long long*)(s + a8);
        last = (const long long*)(s + 2 * a8);
        fl = (const uint32_t*)(s + 3 * a8);
    }
    unsigned long long* tstat = (unsigned long long*)h->tstat;
    const bool timing = h->timing;
    for (hipEvent_t& e : h->oev)
        if (timing && !e) TD_HIP(h, hipEventCreate(&e));
    h->otimed = false;
    TD_HIP(h, hipMemsetAsync(tstat + kTsRuns, 0, 8, h->stream));
    if (timing) TD_HIP(h, hipEventRecord(h->oev[0], h->stream));
    TD_HIP(h, launch_checked("k_td_runs", k_td_runs, dim3(td_grid(n)), dim3(kTdWG), 0, h->stream, tid, (unsigned long long)n,
                             tstat));
    if (timing) TD_HIP(h, hipEventRecord(h->oev[1], h->stream));
    unsigned long long host[kTsWords];
    TD_HIP(h, hipMemcpyAsync(host, tstat, sizeof host, hipMemcpyDeviceToHost, h->stream));
    TD_HIP(h, hipStreamSynchronize(h->stream));  // the call's one synchronisation (also: the staging copies are done)
    if (host[kTsFull]) return tfail(h, ZK_ERR_HIP, "the duration table ran full (the sizing rule was broken)");
    if (host[kTsRuns] == 0 || host[kTsRuns] > n) return tfail(h, ZK_ERR_HIP, "run count out of range");
    // load <= 1/2 whatever the batch holds: every run might be a new trace
    if ((st = ensure_slots(h, 2 * (host[kTsTraces] + host[kTsRuns]))) != ZK_OK) return st;
    if (timing) TD_HIP(h, hipEventRecord(h->oev[2], h->stream));
    const uint64_t rows = (n + 63) / 64;
    TD_HIP(h, launch_checked("k_td_observe", k_td_observe, dim3(td_grid(rows * 64)), dim3(kTdWG), 0, h->stream, tid, first,
                             last, fl, (unsigned long long)n, (unsigned long long*)h->table, (unsigned long long)h->slots,
                             tstat));
    if (timing) TD_HIP(h, hipEventRecord(h->oev[3], h->stream));
    h->otimed = timing;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_td_observe_ms(zk_td* h, double out[3]) {
    ZK_GUARD_BEGIN
    if (!h || !out) return ZK_ERR_INVALID_ARG;
    if (!h->otimed) return tfail(h, ZK_ERR_INVALID_ARG, "no timed observe has run (zk_td_config.timing)");
    TD_HIP(h, hipSetDevice(h->device));
    TD_HIP(h, hipEventSynchronize(h->oev[3]));
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        TD_HIP(h, hipEventElapsedTime(&ms, h->oev[k], h->oev[k + 1]));
        out[k] = ms;
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_td_reset(zk_td* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!h->table) return ZK_OK;
    TD_HIP(h, hipSetDevice(h->device));
    TD_HIP(h, launch_checked("k_td_clear", k_td_clear, dim3(td_grid(h->slots + 1)), dim3(kTdWG), 0, h->stream,
                             (unsigned long long*)h->table, (unsigned long long)(h->slots + 1)));
    TD_HIP(h, hipMemsetAsync(h->tstat, 0, kTsWords * 8, h->stream));
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_td_reserve(zk_td* h, uint64_t traces) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (traces > kTdMaxSlots / 2) return tfail(h, ZK_ERR_CAPACITY, "a duration table of more than 2^40 slots");
    TD_HIP(h, hipSetDevice(h->device));
    return ensure_slots(h, 2 * traces);
    ZK_GUARD_END
}

zk_status zk_td_expire(zk_td* h, int64_t min_end, uint64_t* removed) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (removed) *removed = 0;
    h->xtimed = false;
    if (!h->table) return ZK_OK;
    TD_HIP(h, hipSetDevice(h->device));
    const unsigned long long cut = (unsigned long long)min_end ^ kTdSign;
    unsigned long long* tstat = (unsigned long long*)h->tstat;
    const bool timing = h->timing;
    for (hipEvent_t& e : h->xev)
        if (timing && !e) TD_HIP(h, hipEventCreate(&e));
    TD_HIP(h, hipMemsetAsync(tstat + kTsAlive, 0, 8, h->stream));
    if (timing) TD_HIP(h, hipEventRecord(h->xev[0], h->stream));
    TD_HIP(h, launch_checked("k_td_expire_count", k_td_expire_count, dim3(td_grid(h->slots + 1)), dim3(kTdWG), 0, h->stream,
                             (const unsigned long long*)h->table, (unsigned long long)h->slots, cut, tstat));
    if (timing) TD_HIP(h, hipEventRecord(h->xev[1], h->stream));
    unsigned long long host[kTsWords];
    TD_HIP(h, hipMemcpyAsync(host, tstat, sizeof host, hipMemcpyDeviceToHost, h->stream));
    TD_HIP(h, hipStreamSynchronize(h->stream));  // the sizing synchronisation
    if (host[kTsFull]) return tfail(h, ZK_ERR_HIP, "the duration table ran full (the sizing rule was broken)");
    const uint64_t alive = host[kTsAlive];
    if (alive > host[kTsTraces]) return tfail(h, ZK_ERR_HIP, "the expiry counted more traces than the table holds");
    if (alive == host[kTsTraces]) {  // nothing goes: the table stays where and as it is
        if (timing) TD_HIP(h, hipEventRecord(h->xev[2], h->stream));
        if (timing) TD_HIP(h, hipEventRecord(h->xev[3], h->stream));
        h->xtimed = timing;
        return ZK_OK;
    }
    // the SIZING rule for the stayers alone: this is the one place where the table may shrink
    uint64_t slots = kTdMinSlots;
    while (slots < 2 * alive) slots <<= 1;
    void* q = nullptr;
    size_t have = 0;
    const zk_status st = grow(h, &q, &have, (size_t)(slots + 1) * sizeof(TdEntry), "the duration table (24 B per slot)");
    if (st != ZK_OK) return st;
    const unsigned long long stay = alive;  // (a queued copy reads it; every path below synchronises)
    hipError_t e = timing ? hipEventRecord(h->xev[2], h->stream) : hipSuccess;
    if (e == hipSuccess)
        e = launch_checked("k_td_clear", k_td_clear, dim3(td_grid(slots + 1)), dim3(kTdWG), 0, h->stream, (unsigned long long*)q,
                           (unsigned long long)(slots + 1));
    if (e == hipSuccess)
        e = launch_checked("k_td_expire_move", k_td_expire_move, dim3(td_grid(h->slots + 1)), dim3(kTdWG), 0, h->stream,
                           (const unsigned long long*)h->table, (unsigned long long)h->slots, cut, (unsigned long long*)q,
                           (unsigned long long)slots, tstat);
    if (e == hipSuccess && timing) e = hipEventRecord(h->xev[3], h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(tstat + kTsTraces, &stay, 8, hipMemcpyHostToDevice, h->stream);  // the stayers' count
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(q);
        return tfail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("rebuilding the duration table: ") + launch_error_str(e));
    }
    // the new table is complete: the old one leaves
    (void)hipFree(h->table);
    h->table = q;
    h->slots = slots;
    h->xtimed = timing;
    if (removed) *removed = host[kTsTraces] - alive;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_td_expire_ms(zk_td* h, double out[3]) {
    ZK_GUARD_BEGIN
    if (!h || !out) return ZK_ERR_INVALID_ARG;
    if (!h->xtimed) return tfail(h, ZK_ERR_INVALID_ARG, "no timed expiry has run a pass (zk_td_config.timing)");
    TD_HIP(h, hipSetDevice(h->device));
    TD_HIP(h, hipEventSynchronize(h->xev[3]));
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        TD_HIP(h, hipEventElapsedTime(&ms, h->xev[k], h->xev[k + 1]));
        out[k] = ms;
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_td_info(zk_td* h, uint64_t* slots, uint64_t* traces, uint64_t* bytes) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    unsigned long long host[kTsWords] = {};
    if (h->tstat) {
        TD_HIP(h, hipSetDevice(h->device));
        TD_HIP(h, hipMemcpyAsync(host, h->tstat, sizeof host, hipMemcpyDeviceToHost, h->stream));
        TD_HIP(h, hipStreamSynchronize(h->stream));
        if (host[kTsFull]) return tfail(h, ZK_ERR_HIP, "the duration table ran full (the sizing rule was broken)");
    }
    if (slots) *slots = h->slots;
    if (traces) *traces = host[kTsTraces];
    if (bytes) *bytes = h->table ? (h->slots + 1) * sizeof(TdEntry) : 0;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_td_lookup(zk_td* h, const uint64_t* trace_ids, uint64_t n, uint32_t flags, int64_t* start, int64_t* duration,
                       uint8_t* found) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (flags & ~ZK_BATCH_DEVICE_PTRS) return tfail(h, ZK_ERR_INVALID_ARG, "unknown flag");
    if (n > kTdMaxRecords) return tfail(h, ZK_ERR_UNSUPPORTED, "more than 2^40 ids in one call");
    if (n == 0) return ZK_OK;
    if (!trace_ids || !start || !duration || !found) return tfail(h, ZK_ERR_INVALID_ARG, "null argument");
    TD_HIP(h, hipSetDevice(h->device));
    const bool dev = (flags & ZK_BATCH_DEVICE_PTRS) != 0;
    const size_t a8 = (n * 8 + 255) / 256 * 256;
    zk_status st = grow(h, &h->query, &h->query_bytes, 3 * a8 + n, "the lookup's ids and answers (25 B per id)");
    if (st != ZK_OK) return st;
    uint8_t* q = (uint8_t*)h->query;
    const unsigned long long* ids = (const unsigned long long*)trace_ids;
    if (!dev) {
        TD_HIP(h, hipMemcpyAsync(q, trace_ids, n * 8, hipMemcpyHostToDevice, h->stream));
        ids = (const unsigned long long*)q;
    }
    TD_HIP(h, launch_checked("k_td_query", k_td_query, dim3(td_grid(n)), dim3(kTdWG), 0, h->stream, ids, (unsigned long long)n,
                             (const unsigned long long*)h->table, (unsigned long long)h->slots, (long long*)(q + a8),
                             (long long*)(q + 2 * a8), q + 3 * a8));
    TD_HIP(h, hipMemcpyAsync(start, q + a8, n * 8, hipMemcpyDeviceToHost, h->stream));
    TD_HIP(h, hipMemcpyAsync(duration, q + 2 * a8, n * 8, hipMemcpyDeviceToHost, h->stream));
    TD_HIP(h, hipMemcpyAsync(found, q + 3 * a8, n, hipMemcpyDeviceToHost, h->stream));
    TD_HIP(h, hipStreamSynchronize(h->stream));
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_td_top(zk_td* h, uint32_t order, int64_t start_lo, int64_t start_hi, uint32_t k, uint64_t* trace_id,
                    int64_t* start, int64_t* duration, uint32_t* n_out, uint64_t* matched_out) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!trace_id || !start || !duration || !n_out) return tfail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (k < 1 || k > ZK_TD_MAX_TOP) return tfail(h, ZK_ERR_INVALID_ARG, "k outside 1..ZK_TD_MAX_TOP");
    if (!order_ok(order)) return tfail(h, ZK_ERR_INVALID_ARG, "unknown order");
    if (start_lo > start_hi) return tfail(h, ZK_ERR_INVALID_ARG, "start_lo > start_hi");
    *n_out = 0;
    if (matched_out) *matched_out = 0;
    if (!h->table) return ZK_OK;
    TD_HIP(h, hipSetDevice(h->device));
    zk_status st = grow(h, &h->sel, &h->sel_bytes, kSelBytes, "the select's counters and lists");
    if (st != ZK_OK) return st;
    uint8_t* sb = (uint8_t*)h->sel;
    unsigned long long* sel = (unsigned long long*)sb;
    uint32_t* hist = (uint32_t*)(sb + kSelHistAt);
    unsigned long long* certain_list = (unsigned long long*)(sb + kSelCertainAt);
    const bool timing = h->timing;
    for (hipEvent_t& e : h->tev)
        if (timing && !e) TD_HIP(h, hipEventCreate(&e));
    h->ttimed = false;

    TdSrc src{(const unsigned long long*)h->table, h->slots + 1, h->slots, (unsigned long long)start_lo ^ kTdSign,
              (unsigned long long)start_hi ^ kTdSign, 1u};
    unsigned long long host[kSelWords];
    // pass 1 over the table: how many match, and the bits in which their keys differ
    TD_HIP(h, hipMemsetAsync(sel, 0, kSelWords * 8, h->stream));
    if (timing) TD_HIP(h, hipEventRecord(h->tev[0], h->stream));
    TD_HIP(h, launch_checked("k_td_scan", k_td_scan, dim3(td_grid(src.count)), dim3(kTdWG), 0, h->stream, src, order, sel));
    TD_HIP(h, hipMemcpyAsync(host, sel, sizeof host, hipMemcpyDeviceToHost, h->stream));
    TD_HIP(h, hipStreamSynchronize(h->stream));
    const uint64_t matched = host[kSelMatched];
    if (matched > h->slots + 1) return tfail(h, ZK_ERR_HIP, "the select counted more entries than slots");
    uint64_t certain = 0, cand = matched, want = k;
    int cur = -1;  // the list that holds the candidates; -1: they are still the table's
    static thread_local std::vector<uint32_t> hh;
    hh.resize(kTdBins);
    while (matched && certain + cand > kTdCap) {
        const uint64_t diff_hi = host[kSelOrHi] & host[kSelNorHi], diff_lo = host[kSelOrLo] & host[kSelNorLo];
        if (!(diff_hi | diff_lo)) return tfail(h, ZK_ERR_HIP, "the select's candidates do not differ");
        const uint32_t shift = td_shift_of(diff_hi, diff_lo);
        TD_HIP(h, hipMemsetAsync(hist, 0, kTdBins * 4, h->stream));
        TD_HIP(h, launch_checked("k_td_hist", k_td_hist, dim3(std::min(td_grid(src.count), kTdHistGrid)), dim3(kTdWG), 0, h->stream, src, order, shift,
                                 hist));
        TD_HIP(h, hipMemcpyAsync(hh.data(), hist, kTdBins * 4, hipMemcpyDeviceToHost, h->stream));
        TD_HIP(h, hipStreamSynchronize(h->stream));
        uint64_t below = 0;
        const uint32_t bin = td_pick_bin(hh.data(), want, &below);
        if (bin >= kTdBins || hh[bin] >= cand || below >= want)
            return tfail(h, ZK_ERR_HIP, "the select's histogram does not split its candidates");
        const uint64_t stay = hh[bin];
        const int dst = cur == 0 ? 1 : 0;
        if ((st = grow(h, &h->list[dst], &h->list_bytes[dst], (size_t)stay * sizeof(TdEntry),
                       "the select's candidate list (24 B per entry)")) != ZK_OK)
            return st;
        TD_HIP(h, hipMemsetAsync(sel + kSelOrHi, 0, (kSelCand + 1 - kSelOrHi) * 8, h->stream));
        TD_HIP(h, launch_checked("k_td_collect", k_td_collect, dim3(td_grid((src.count + kColItems - 1) / kColItems)), dim3(kTdWG), 0, h->stream, src, order,
                                 shift, bin, sel, certain_list, (unsigned long long)kTdCap, (unsigned long long*)h->list[dst],
                                 (unsigned long long)stay));
        certain += below;
        want -= below;
        cand = stay;
        cur = dst;
        src = TdSrc{(const unsigned long long*)h->list[dst], stay, kAllOnes, 0ull, kAllOnes, 0u};
        if (certain + cand > kTdCap) {
            TD_HIP(h, hipMemcpyAsync(host, sel, sizeof host, hipMemcpyDeviceToHost, h->stream));
            TD_HIP(h, hipStreamSynchronize(h->stream));
        }
    }
    if (matched && cur < 0) {
        // everything that matches fits the cap: one pass appends it all to the certain list
        TD_HIP(h, launch_checked("k_td_collect", k_td_collect, dim3(td_grid((src.count + kColItems - 1) / kColItems)), dim3(kTdWG), 0, h->stream, src, order,
                                 0u, kTdBins, sel, certain_list, (unsigned long long)kTdCap, (unsigned long long*)nullptr,
                                 0ull));
        certain = matched;
        cand = 0;
    }
    static thread_local std::vector<TdEntry> ent;
    ent.resize(certain + cand);
    if (certain) TD_HIP(h, hipMemcpyAsync(ent.data(), certain_list, certain * sizeof(TdEntry), hipMemcpyDeviceToHost, h->stream));
    if (cand)
        TD_HIP(h, hipMemcpyAsync(ent.data() + certain, h->list[cur], cand * sizeof(TdEntry), hipMemcpyDeviceToHost, h->stream));
    if (timing) TD_HIP(h, hipEventRecord(h->tev[1], h->stream));
    TD_HIP(h, hipStreamSynchronize(h->stream));
    h->ttimed = timing;
    *n_out = td_emit(ent.data(), ent.size(), order, k, trace_id, start, duration);
    if (matched_out) *matched_out = matched;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_td_top_ms(zk_td* h, double* ms) {
    ZK_GUARD_BEGIN
    if (!h || !ms) return ZK_ERR_INVALID_ARG;
    if (!h->ttimed) return tfail(h, ZK_ERR_INVALID_ARG, "no timed top has run (zk_td_config.timing)");
    TD_HIP(h, hipSetDevice(h->device));
    float f = 0.f;
    TD_HIP(h, hipEventElapsedTime(&f, h->tev[0], h->tev[1]));
    *ms = f;
    return ZK_OK;
    ZK_GUARD_END
}

}  // extern "C"
