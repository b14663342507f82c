// zk_win.hip — the device trace-time partition (include/zkwindow.h, zk_win_*): a trace-clustered batch
// split by time window, stably, so that every window's slice is again a trace-clustered batch.
//
// Geometry (zk_win_plan): the input is cut into `ranges` contiguous workgroup ranges of whole chunks
// (kWinChunk records, the unit a workgroup holds in LDS); one workgroup walks one range front to back
// in every pass, so every position is fixed by counts and one scan: no atomic touches global memory
// and the output bytes are a function of the input alone.
//
//   k_win_time     per range, chunk by chunk: run starts by neighbour compare and ballots, every
//                  record's run head by the highest start bit at or below its lane (rows of 64) and a
//                  per-row carry, the run's minimum timed first_ts by an LDS minimum on the head's
//                  slot, the class by the window rule. A run that lies inside the range gets its class
//                  written to u16 win[n] (one that crosses chunks when it closes). The run that enters
//                  the range from before and the one that leaves it are not written: their keys go to
//                  the range's summary (WinRange).
//   k_win_resolve  one workgroup: the summaries in LDS; the thread of a range whose last run leaves it
//                  chains that run across the range edges (a run may cover any number of whole
//                  ranges) and gives every range the class of the run entering it (head_id) and of
//                  the run leaving it (tail_id). Nothing is written back into win[]: the later passes
//                  pick head_id / tail_id by two index compares per record. It also finds the
//                  batch's last run (ZK_WIN_HOLD_LAST).
//   k_win_hist     per range: LDS histogram of the classes into the window-major u64 matrix
//                  M[W + 1][ranges] (+ one total slot). One exclusive hipcub scan of M gives every
//                  (window, range) its output base; the row bases are the offsets.
//   k_win_scatter  per range: per-window cursors in LDS; per chunk every record's stable rank (equal
//                  classes of a row by ballot matching, rows in order per wave, waves by a per-wave
//                  count), then the seven columns move from registers. Adjacent records of one window
//                  have adjacent positions, so a wave's stores form one contiguous piece per run of
//                  equal windows in its row.
//   k_win_final    one workgroup: offsets (row bases of the scanned M) and the counts, gathered into
//                  one small buffer for the call's single device-to-host copy.
//
// HBM traffic per record: 20 B read by the time pass (traceId, first_ts, flags), 2 B written and 4 B
// read of win[], 48 B read and 48 B written by the scatter.
//
// Table mode (ZK_WIN_TRACE_TABLE), for records in any order and traces cut at a batch edge: a trace's
// time comes from a traceId-keyed table in HBM that zk_win_observe fills from every batch first.
//   k_wt_runs      the batch's run starts; the host sizes the table by them before anything is inserted
//   k_wt_observe   one table update per (run, row of 64 records): a probe, then at most one CAS on the
//                  key and one 64-bit atomic minimum on the time
//   k_wt_rehash    the old table's keys into a grown one; k_wt_clear empties a table
//   k_wt_lookup    stands in for k_win_time and k_win_resolve: win[i] from the table for every record;
//                  every range is left without an entering or a leaving run, so the passes from
//                  k_win_hist on run as they are
//   k_wt_query     zk_win_table_lookup
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <string.h>

#include <string>

#include "zk_guard.h"
#include "zk_launch.h"
#include "zk_tracegen.h"
#include "zkwindow.h"

namespace zk {
namespace {

constexpr int kWinWG = 256;
constexpr int kWinRows = 4;                       // rows of 64 records per wave and chunk
constexpr uint32_t kWinChunkRows = 16;            // rows per chunk (4 waves x kWinRows)
constexpr uint32_t kWinChunk = 64 * kWinChunkRows;
constexpr uint64_t kWinMaxRanges = 2048;
constexpr uint64_t kWinMaxRecords = 1ull << 40;   // (positions are u64; a range's counts stay below 2^32)
constexpr uint32_t kWinMaxClasses = ZK_WIN_MAX_WINDOWS + 3;
constexpr unsigned long long kKeyNone = ~0ull;
constexpr unsigned long long kSign = 1ull << 63;

static_assert(kWinChunk == (uint32_t)kWinWG * kWinRows, "a thread holds kWinRows records of a chunk");

struct WinRule {
    int64_t origin;
    uint64_t window;
    uint32_t W;
};

// class of a run: 0..W-1 its window, W before, W + 1 after, W + 2 untimed. key = first_ts with the
// sign bit flipped (unsigned order = signed order).
__host__ __device__ inline uint32_t win_class(unsigned long long key, bool timed, WinRule r) {
    if (!timed) return r.W + 2;
    const int64_t t = (int64_t)(key ^ kSign);
    if (t < r.origin) return r.W;
    const uint64_t w = ((uint64_t)t - (uint64_t)r.origin) / r.window;
    return w >= r.W ? r.W + 1 : (uint32_t)w;
}

enum : uint32_t {
    RF_HEAD = 1,         // the range's first record continues a run from before the range
    RF_WHOLE = 2,        // ... and no run starts in the range
    RF_CONT = 4,         // the range's last run continues past the range
    RF_HEAD_TIMED = 8,
    RF_TAIL_TIMED = 16,
};

struct WinRange {
    unsigned long long first_start;  // first record of the range that starts a run; the range's end when none
    unsigned long long tail_start;   // start of the range's last run (unless RF_WHOLE)
    unsigned long long head_key;     // minimum timed key of the entering run's records in this range
    unsigned long long tail_key;     // ... of the leaving run's (RF_CONT)
    uint32_t flags;
    uint32_t tail_cls;               // class of the last run when it ends with the range
    uint32_t runs[4];                // runs closed by k_win_time: window, before, after, untimed
    uint32_t recs[3];                // k_win_hist: records before, after, untimed
    uint32_t head_id, tail_id;       // k_win_resolve: class of the entering / leaving run
    uint32_t pad;
};

// gstat (k_win_resolve): [0..3] runs that cross range edges by category (less the held run), [4]
// held_from, [5] held runs
constexpr int kGstatWords = 8;
// res (k_win_final): offsets[W + 2], then runs[4], records before/after/untimed, held_from, held runs
constexpr int kResTail = 9;
constexpr int kWinPhases = 6;  // time, resolve, hist, scan, scatter, final

__device__ inline uint32_t lane_id() { return threadIdx.x & 63; }

// Lanes of the wave with equal `b` (among `valid` lanes): rank = equal lanes below this one, cnt =
// their number, lead = the lowest of them. The loop runs once per distinct value (wave-uniform).
__device__ inline void match_equal(uint32_t b, bool valid, uint32_t* rank, uint32_t* cnt, uint32_t* lead) {
    const uint32_t lane = lane_id();
    unsigned long long todo = __ballot(valid);
    *rank = 0;
    *cnt = 0;
    *lead = lane;
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        const uint32_t lb = __shfl(b, l);
        const unsigned long long m = __ballot(valid && b == lb);
        if (valid && b == lb) {
            *rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            *cnt = (uint32_t)__popcll(m);
            *lead = (uint32_t)l;
        }
        todo &= ~m;
    }
}

__global__ __launch_bounds__(kWinWG) void k_win_time(const unsigned long long* __restrict__ tid,
                                                     const long long* __restrict__ ts,
                                                     const uint32_t* __restrict__ fl, unsigned long long n,
                                                     unsigned long long range_records, WinRule rule,
                                                     uint16_t* __restrict__ win, WinRange* __restrict__ rs) {
    __shared__ unsigned long long s_key[kWinChunk];  // minimum timed key of the run whose head is this slot
    __shared__ uint32_t s_timed[kWinChunk];
    __shared__ int s_rfirst[kWinChunkRows], s_rlast[kWinChunkRows];  // first / last start of a row, -1 none
    __shared__ unsigned long long s_ckey;  // this chunk's part of the carried run
    __shared__ uint32_t s_ctimed;
    __shared__ uint32_t s_runs[4];
    const int t = threadIdx.x;
    const uint32_t lane = t & 63, wave = t >> 6;
    const unsigned long long r0 = (unsigned long long)blockIdx.x * range_records;
    const unsigned long long r1 = r0 + range_records < n ? r0 + range_records : n;
    const bool head = r0 > 0 && tid[r0] == tid[r0 - 1];
    const bool cont = r1 < n && tid[r1] == tid[r1 - 1];
    // the run open at the chunk's first record (the same in every thread): the range's entering run
    // (c_entering: its class is not known here) or the previous chunk's last run, started at c_head
    bool c_has = head, c_entering = head, c_timed = false;
    unsigned long long c_head = r0, c_key = kKeyNone;
    unsigned long long first_start = r1, h_key = kKeyNone;
    bool h_timed = false;
    uint32_t runs_w = 0, runs_b = 0, runs_a = 0, runs_u = 0;
    if (t < 4) s_runs[t] = 0;
#define WIN_COUNT_RUN(cls)                \
    do {                                  \
        runs_w += (cls) < rule.W;         \
        runs_b += (cls) == rule.W;        \
        runs_a += (cls) == rule.W + 1;    \
        runs_u += (cls) == rule.W + 2;    \
    } while (0)
    for (unsigned long long base = r0; base < r1; base += kWinChunk) {
        const uint32_t cnt = r1 - base < kWinChunk ? (uint32_t)(r1 - base) : kWinChunk;
        unsigned long long key[kWinRows], mask[kWinRows];
        bool timed[kWinRows];
        // every load of the chunk first, none depending on another (the neighbour's id straight from
        // memory, the time whether or not the fragment is timed): one memory latency per chunk
        unsigned long long v_id[kWinRows], v_prev[kWinRows];
        long long v_ts[kWinRows];
        uint32_t v_fl[kWinRows];
#pragma unroll
        for (int k = 0; k < kWinRows; ++k) {
            const uint32_t j = (wave * kWinRows + k) * 64 + lane;
            const unsigned long long i = base + j;
            const bool valid = j < cnt;
            v_id[k] = valid ? tid[i] : 0ull;
            v_prev[k] = valid && i > 0 ? tid[i - 1] : 0ull;
            v_fl[k] = valid ? fl[i] : 0u;
            v_ts[k] = valid ? ts[i] : 0ll;
        }
#pragma unroll
        for (int k = 0; k < kWinRows; ++k) {
            const uint32_t R = wave * kWinRows + k, j = R * 64 + lane;
            const unsigned long long i = base + j;
            const bool valid = j < cnt;
            s_key[j] = kKeyNone;
            s_timed[j] = 0u;
            const bool start = valid && (i == 0 || v_id[k] != v_prev[k]);
            mask[k] = __ballot(start);
            timed[k] = (v_fl[k] & ZK_F_HAS_ANNOTATIONS) != 0u;
            key[k] = timed[k] ? (unsigned long long)v_ts[k] ^ kSign : kKeyNone;
            if (lane == 0) {
                s_rfirst[R] = mask[k] ? (int)(R * 64) + __ffsll((long long)mask[k]) - 1 : -1;
                s_rlast[R] = mask[k] ? (int)(R * 64) + 63 - __clzll((long long)mask[k]) : -1;
            }
        }
        if (t == 0) {
            s_ckey = kKeyNone;
            s_ctimed = 0u;
        }
        __syncthreads();
        int hd[kWinRows];  // the head's slot in this chunk, -1: the carried run
#pragma unroll
        for (int k = 0; k < kWinRows; ++k) {
            const int R = (int)(wave * kWinRows) + k;
            const unsigned long long mm = mask[k] & (~0ull >> (63 - lane));
            int h = -1;
            if (mm) {
                h = R * 64 + 63 - __clzll((long long)mm);
            } else {
                for (int q = R - 1; q >= 0; --q) {
                    const int v = s_rlast[q];
                    if (v >= 0) {
                        h = v;
                        break;
                    }
                }
            }
            hd[k] = h;
            // the row's part of the run first, in registers: lanes [s, e] of this lane's run, a
            // suffix minimum over them, and one LDS minimum per run and row (by lane s) instead of
            // one per record on the same address
            const unsigned long long above = lane == 63 ? 0ull : mask[k] & (~0ull << (lane + 1));
            const uint32_t s = mm ? 63u - (uint32_t)__clzll((long long)mm) : 0u;
            const uint32_t e = above ? (uint32_t)__ffsll((long long)above) - 2u : 63u;
            const unsigned long long seg = (~0ull >> (63 - e)) & (~0ull << s);
            const bool any_timed = (__ballot(timed[k]) & seg) != 0ull;
            unsigned long long kmin = key[k];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned long long o = __shfl_down(kmin, off);
                if (lane + off <= e && o < kmin) kmin = o;
            }
            if (lane == s && any_timed) {
                if (h >= 0) {
                    atomicMin(&s_key[h], kmin);
                    s_timed[h] = 1u;
                } else {
                    atomicMin(&s_ckey, kmin);
                    s_ctimed = 1u;
                }
            }
        }
        __syncthreads();
        int fs = -1, ls = -1;  // first / last start of the chunk
        for (uint32_t q = 0; q < kWinChunkRows; ++q) {
            const int a = s_rfirst[q], b = s_rlast[q];
            if (fs < 0 && a >= 0) fs = a;
            if (b >= 0) ls = b;
        }
        if (c_has) {
            const unsigned long long ck = s_ckey;
            c_key = ck < c_key ? ck : c_key;
            c_timed = c_timed || s_ctimed != 0u;
        }
        const bool close_last = base + cnt == r1 && !cont;  // the chunk's last run ends with the range
        const bool carry_final = fs >= 0 || close_last;
        const uint32_t c_cls = win_class(c_key, c_timed, rule);
#pragma unroll
        for (int k = 0; k < kWinRows; ++k) {
            const uint32_t j = (wave * kWinRows + k) * 64 + lane;
            if (j >= cnt) continue;
            const int h = hd[k];
            bool fin;
            uint32_t cls;
            if (h < 0) {
                fin = carry_final && !c_entering;
                cls = c_cls;
            } else {
                fin = h != ls || close_last;
                cls = win_class(s_key[h], s_timed[h] != 0u, rule);
            }
            if (fin) {
                win[base + j] = (uint16_t)cls;
                if ((mask[k] >> lane) & 1ull) WIN_COUNT_RUN(cls);
            }
        }
        if (c_has && !c_entering && carry_final) {
            // the carried run closes here: its records in the earlier chunks
            for (unsigned long long x = c_head + t; x < base; x += kWinWG) win[x] = (uint16_t)c_cls;
            if (t == 0) WIN_COUNT_RUN(c_cls);
        }
        if (c_has && c_entering && fs >= 0) {
            h_key = c_key;
            h_timed = c_timed;
        }
        if (fs >= 0 && first_start == r1) first_start = base + (uint32_t)fs;
        if (ls >= 0) {
            c_has = true;
            c_entering = false;
            c_head = base + (uint32_t)ls;
            c_key = s_key[ls];
            c_timed = s_timed[ls] != 0u;
        }
        __syncthreads();  // (the next chunk re-initialises the slots)
    }
#undef WIN_COUNT_RUN
    if (runs_w) atomicAdd(&s_runs[0], runs_w);
    if (runs_b) atomicAdd(&s_runs[1], runs_b);
    if (runs_a) atomicAdd(&s_runs[2], runs_a);
    if (runs_u) atomicAdd(&s_runs[3], runs_u);
    __syncthreads();
    if (t == 0) {
        WinRange o{};
        const bool whole = head && first_start == r1;
        o.first_start = first_start;
        o.flags = (head ? RF_HEAD : 0u) | (whole ? RF_WHOLE : 0u);
        if (whole) {
            h_key = c_key;
            h_timed = c_timed;
        } else {
            o.tail_start = c_head;
            if (cont) {
                o.flags |= RF_CONT | (c_timed ? RF_TAIL_TIMED : 0u);
                o.tail_key = c_key;
            } else {
                o.tail_cls = win_class(c_key, c_timed, rule);
            }
        }
        o.head_key = h_key;
        if (h_timed) o.flags |= RF_HEAD_TIMED;
        for (int c = 0; c < 4; ++c) o.runs[c] = s_runs[c];
        rs[blockIdx.x] = o;
    }
}

__global__ __launch_bounds__(kWinWG) void k_win_resolve(WinRange* __restrict__ rs, uint32_t ranges, unsigned long long n,
                                                        WinRule rule, int hold, long long* __restrict__ gstat) {
    __shared__ unsigned long long s_hkey[kWinMaxRanges], s_tkey[kWinMaxRanges];
    __shared__ uint32_t s_flags[kWinMaxRanges], s_hid[kWinMaxRanges], s_tid[kWinMaxRanges];
    __shared__ uint32_t s_adj[4], s_last[2];  // crossing runs by category; owner and class of the one reaching the end
    const int t = threadIdx.x;
    for (uint32_t r = t; r < ranges; r += kWinWG) {
        s_hkey[r] = rs[r].head_key;
        s_tkey[r] = rs[r].tail_key;
        s_flags[r] = rs[r].flags;
        s_hid[r] = 0u;
        s_tid[r] = 0u;
    }
    if (t < 4) s_adj[t] = 0u;
    if (t < 2) s_last[t] = 0u;
    __syncthreads();
    // every range whose last run leaves it owns that run: its thread walks on while the run covers
    // whole ranges (any number of them) and closes it in the first range that has a start, or at the
    // batch's end. Runs are disjoint, so no two threads write the same slot.
    uint32_t adj_w = 0, adj_b = 0, adj_a = 0, adj_u = 0;
    for (uint32_t r = t; r < ranges; r += kWinWG) {
        const uint32_t f = s_flags[r];
        if ((f & RF_WHOLE) || !(f & RF_CONT)) continue;
        unsigned long long key = s_tkey[r];
        bool timed = (f & RF_TAIL_TIMED) != 0u;
        uint32_t q = r + 1;
        bool to_end = true;  // the run reaches the batch's end through whole ranges
        for (; q < ranges; ++q) {
            const uint32_t fq = s_flags[q];
            key = s_hkey[q] < key ? s_hkey[q] : key;
            timed = timed || (fq & RF_HEAD_TIMED);
            if (!(fq & RF_WHOLE)) {
                to_end = false;
                break;
            }
        }
        const uint32_t e = q < ranges ? q : ranges - 1;
        const uint32_t cls = win_class(key, timed, rule);
        s_tid[r] = cls;
        for (uint32_t x = r + 1; x <= e; ++x) s_hid[x] = cls;
        adj_w += cls < rule.W;
        adj_b += cls == rule.W;
        adj_a += cls == rule.W + 1;
        adj_u += cls == rule.W + 2;
        if (to_end) {
            s_last[0] = r;
            s_last[1] = cls;
        }
    }
    if (adj_w) atomicAdd(&s_adj[0], adj_w);
    if (adj_b) atomicAdd(&s_adj[1], adj_b);
    if (adj_a) atomicAdd(&s_adj[2], adj_a);
    if (adj_u) atomicAdd(&s_adj[3], adj_u);
    __syncthreads();
    if (t == 0) {
        // the batch's last run: the last range's own last run, or the crossing run that reaches the end
        const uint32_t L = ranges - 1;
        unsigned long long held_from = n;
        long long held_runs = 0, sub_w = 0, sub_b = 0, sub_a = 0, sub_u = 0;
        if (hold) {
            const bool whole = (s_flags[L] & RF_WHOLE) != 0u;
            held_from = whole ? rs[s_last[0]].tail_start : rs[L].tail_start;
            const uint32_t cls = whole ? s_last[1] : rs[L].tail_cls;
            sub_w = cls < rule.W;
            sub_b = cls == rule.W;
            sub_a = cls == rule.W + 1;
            sub_u = cls == rule.W + 2;
            held_runs = 1;
        }
        gstat[0] = (long long)s_adj[0] - sub_w;
        gstat[1] = (long long)s_adj[1] - sub_b;
        gstat[2] = (long long)s_adj[2] - sub_a;
        gstat[3] = (long long)s_adj[3] - sub_u;
        gstat[4] = (long long)held_from;
        gstat[5] = held_runs;
    }
    __syncthreads();
    for (uint32_t r = t; r < ranges; r += kWinWG) {
        rs[r].head_id = s_hid[r];
        rs[r].tail_id = s_tid[r];
    }
}

// what the later passes need of a range: its records less the held ones, and the class of a record
struct RangeView {
    unsigned long long r0, r1, first_start, tail_start;
    uint32_t head_id, tail_id;
    bool cont;
};

__device__ inline RangeView range_view(const WinRange* __restrict__ rs, unsigned long long n,
                                       unsigned long long range_records, const long long* __restrict__ gstat) {
    RangeView v;
    const WinRange& g = rs[blockIdx.x];
    const unsigned long long held_from = (unsigned long long)gstat[4];
    v.r0 = (unsigned long long)blockIdx.x * range_records;
    v.r1 = v.r0 + range_records < n ? v.r0 + range_records : n;
    if (v.r1 > held_from) v.r1 = held_from;
    v.first_start = g.first_start;
    v.tail_start = g.tail_start;
    v.head_id = g.head_id;
    v.tail_id = g.tail_id;
    v.cont = (g.flags & RF_CONT) != 0u && (g.flags & RF_WHOLE) == 0u;
    return v;
}

__device__ inline uint32_t record_class(const RangeView& v, const uint16_t* __restrict__ win, unsigned long long i) {
    if (i < v.first_start) return v.head_id;
    if (v.cont && i >= v.tail_start) return v.tail_id;
    return win[i];
}

__global__ __launch_bounds__(kWinWG) void k_win_hist(const uint16_t* __restrict__ win, WinRange* __restrict__ rs,
                                                     unsigned long long n, unsigned long long range_records,
                                                     uint32_t W, uint32_t ranges, const long long* __restrict__ gstat,
                                                     unsigned long long* __restrict__ M) {
    __shared__ uint32_t s_h[kWinMaxClasses];
    const int t = threadIdx.x;
    const RangeView v = range_view(rs, n, range_records, gstat);
    for (uint32_t b = t; b < W + 3; b += kWinWG) s_h[b] = 0u;
    __syncthreads();
    for (unsigned long long base = v.r0; base < v.r1; base += kWinWG) {
        const unsigned long long i = base + t;
        const bool valid = i < v.r1;
        uint32_t cls = valid ? record_class(v, win, i) : 0u;
        if (cls > W + 2) cls = W + 2;  // (never: keeps the LDS index in bounds whatever win[] holds)
        uint32_t rank, cnt, lead;
        match_equal(cls, valid, &rank, &cnt, &lead);
        if (valid && lane_id() == lead) atomicAdd(&s_h[cls], cnt);
    }
    __syncthreads();
    for (uint32_t b = t; b <= W; b += kWinWG)
        M[(unsigned long long)b * ranges + blockIdx.x] = b < W ? s_h[b] : (unsigned long long)s_h[W] + s_h[W + 1] + s_h[W + 2];
    if (t == 0) {
        for (int c = 0; c < 3; ++c) rs[blockIdx.x].recs[c] = s_h[W + c];
        if (blockIdx.x == 0) M[(unsigned long long)(W + 1) * ranges] = 0ull;  // the scan puts the total here
    }
}

struct WinCols {
    const unsigned long long* trace_id;
    const unsigned long long* span_id;
    const unsigned long long* parent_id;
    const long long* first_ts;
    const long long* last_ts;
    const uint32_t* service_id;
    const uint32_t* flags;
};
struct WinOutCols {
    unsigned long long* trace_id;
    unsigned long long* span_id;
    unsigned long long* parent_id;
    long long* first_ts;
    long long* last_ts;
    uint32_t* service_id;
    uint32_t* flags;
};

__global__ __launch_bounds__(kWinWG) void k_win_scatter(WinCols in, WinOutCols out, const uint16_t* __restrict__ win,
                                                        const WinRange* __restrict__ rs, unsigned long long n,
                                                        unsigned long long range_records, uint32_t W, uint32_t ranges,
                                                        const long long* __restrict__ gstat,
                                                        const unsigned long long* __restrict__ M) {
    constexpr uint32_t NB = ZK_WIN_MAX_WINDOWS + 1;
    __shared__ unsigned long long s_base[NB];  // the range's first output position of every part
    __shared__ uint32_t s_cur[NB];             // records of the part moved by the chunks before
    __shared__ uint32_t s_wcnt[kWinWG / 64][NB];  // this chunk's records of the part, per wave
    const int t = threadIdx.x;
    const uint32_t lane = t & 63, wave = t >> 6;
    const RangeView v = range_view(rs, n, range_records, gstat);
    for (uint32_t b = t; b <= W; b += kWinWG) {
        s_base[b] = M[(unsigned long long)b * ranges + blockIdx.x];
        s_cur[b] = 0u;
        for (int w = 0; w < kWinWG / 64; ++w) s_wcnt[w][b] = 0u;
    }
    __syncthreads();
    for (unsigned long long base = v.r0; base < v.r1; base += kWinChunk) {
        unsigned long long c_tid[kWinRows], c_sid[kWinRows], c_pid[kWinRows];
        long long c_fts[kWinRows], c_lts[kWinRows];
        uint32_t c_svc[kWinRows], c_fl[kWinRows];
        uint32_t bk[kWinRows], wrank[kWinRows], gcnt[kWinRows];
        bool lead[kWinRows];
        // the classes first (the ranking waits for them alone), then the 48 B that only the stores need
#pragma unroll
        for (int k = 0; k < kWinRows; ++k) {
            const unsigned long long i = base + (wave * kWinRows + k) * 64 + lane;
            const uint32_t b = i < v.r1 ? record_class(v, win, i) : 0u;
            bk[k] = b < W ? b : W;
        }
#pragma unroll
        for (int k = 0; k < kWinRows; ++k) {
            const unsigned long long i = base + (wave * kWinRows + k) * 64 + lane;
            if (i < v.r1) {
                c_tid[k] = in.trace_id[i];
                c_sid[k] = in.span_id[i];
                c_pid[k] = in.parent_id[i];
                c_fts[k] = in.first_ts[i];
                c_lts[k] = in.last_ts[i];
                c_svc[k] = in.service_id[i];
                c_fl[k] = in.flags[i];
            }
        }
#pragma unroll
        for (int k = 0; k < kWinRows; ++k) {
            const unsigned long long i = base + (wave * kWinRows + k) * 64 + lane;
            const bool valid = i < v.r1;
            const uint32_t b = bk[k];
            // rows in order: the wave's count of the part so far is the row's base (only this wave
            // touches its counters between the barriers)
            uint32_t rank, cnt, ld;
            match_equal(b, valid, &rank, &cnt, &ld);
            uint32_t old = 0u;
            lead[k] = valid && lane == ld;
            if (lead[k]) old = atomicAdd(&s_wcnt[wave][b], cnt);
            old = __shfl(old, (int)ld);
            wrank[k] = old + rank;
            gcnt[k] = cnt;
        }
        __syncthreads();
        unsigned long long pos[kWinRows];
#pragma unroll
        for (int k = 0; k < kWinRows; ++k) {
            const uint32_t b = bk[k];
            uint32_t before = s_cur[b] + wrank[k];
            for (uint32_t w = 0; w < wave; ++w) before += s_wcnt[w][b];
            pos[k] = s_base[b] + before;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kWinRows; ++k) {
            if (lead[k]) {
                atomicAdd(&s_cur[bk[k]], gcnt[k]);
                s_wcnt[wave][bk[k]] = 0u;
            }
            const unsigned long long i = base + (wave * kWinRows + k) * 64 + lane;
            const unsigned long long p = pos[k];
            if (i < v.r1 && p < n) {
                out.trace_id[p] = c_tid[k];
                out.span_id[p] = c_sid[k];
                out.parent_id[p] = c_pid[k];
                out.first_ts[p] = c_fts[k];
                out.last_ts[p] = c_lts[k];
                out.service_id[p] = c_svc[k];
                out.flags[p] = c_fl[k];
            }
        }
    }
}

__global__ __launch_bounds__(kWinWG) void k_win_final(const unsigned long long* __restrict__ M, uint32_t ranges, uint32_t W,
                                                      const WinRange* __restrict__ rs, const long long* __restrict__ gstat,
                                                      unsigned long long* __restrict__ res) {
    __shared__ unsigned long long s_sum[7];
    const int t = threadIdx.x;
    if (t < 7) s_sum[t] = 0ull;
    __syncthreads();
    for (uint32_t b = t; b <= W + 1; b += kWinWG) res[b] = M[(unsigned long long)b * ranges];
    unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0;
    for (uint32_t r = t; r < ranges; r += kWinWG) {
        a0 += rs[r].runs[0];
        a1 += rs[r].runs[1];
        a2 += rs[r].runs[2];
        a3 += rs[r].runs[3];
        a4 += rs[r].recs[0];
        a5 += rs[r].recs[1];
        a6 += rs[r].recs[2];
    }
    atomicAdd(&s_sum[0], a0);
    atomicAdd(&s_sum[1], a1);
    atomicAdd(&s_sum[2], a2);
    atomicAdd(&s_sum[3], a3);
    atomicAdd(&s_sum[4], a4);
    atomicAdd(&s_sum[5], a5);
    atomicAdd(&s_sum[6], a6);
    __syncthreads();
    if (t < 4) res[W + 2 + t] = s_sum[t] + (unsigned long long)gstat[t];
    if (t >= 4 && t < 7) res[W + 2 + t] = s_sum[t];
    if (t == 7) res[W + 2 + 7] = (unsigned long long)gstat[4];
    if (t == 8) res[W + 2 + 8] = (unsigned long long)gstat[5];
}

// ---- the trace-time table (ZK_WIN_TRACE_TABLE) ---------------------------------------------------
// traceId -> minimum timed first_ts over every observed batch: open addressing, linear probing, 16 B
// per slot {key, time}; key 0 = empty, time = first_ts with the sign bit flipped, all ones when the
// slot is made. slots is a power of two; traceId 0 lives in the extra slot at index `slots`, its key
// word a presence flag. The host keeps the load at or below 1/2 (it sizes the table from k_wt_runs'
// count BEFORE anything is inserted), so a probe always meets an empty slot; every probe loop is
// bounded by `slots` all the same and reports to tstat[kTsFull] instead of spinning.
//
// Times only fall and keys never change once set, so whatever a plain (possibly stale, possibly torn)
// 16-B load returns, its time word is an upper bound of the slot's time and a non-zero key is the
// slot's key for good: "stored time <= ours: skip" is safe, an empty-looking slot is settled by the
// CAS, and the atomics (device scope, executed at the memory side on a hipMalloc'd table) never see
// a cache.
constexpr unsigned long long kWinTableSalt = ZK_WIN_TABLE_SALT;
constexpr uint64_t kWtMinSlots = 1024;
constexpr uint64_t kWtMaxSlots = 1ull << 40;
constexpr int kWtWG = 256;
constexpr uint32_t kWtMaxGrid = 4096;
enum { kTsTraces = 0, kTsRuns = 1, kTsFull = 2, kTsWords = 4 };

struct alignas(16) WtSlot {
    unsigned long long key, time;
};

__device__ inline WtSlot wt_load(const WtSlot* p) {
    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(p);
    return WtSlot{v.x, v.y};
}

__device__ inline unsigned long long wt_home(unsigned long long id, unsigned long long slots) {
    return zk_mix64(id ^ kWinTableSalt) & (slots - 1ull);
}

__global__ __launch_bounds__(kWtWG) void k_wt_clear(WtSlot* __restrict__ tab, unsigned long long count) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kWtWG;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kWtWG + threadIdx.x; i < count; i += stride)
        *reinterpret_cast<ulonglong2*>(tab + i) = ulonglong2{0ull, kKeyNone};
}

// the batch's run starts, into tstat[kTsRuns] (zeroed by the host before)
__global__ __launch_bounds__(kWtWG) void k_wt_runs(const unsigned long long* __restrict__ tid, unsigned long long n,
                                                   unsigned long long* __restrict__ tstat) {
    __shared__ unsigned long long s_sum;
    const int t = threadIdx.x;
    if (t == 0) s_sum = 0ull;
    __syncthreads();
    const unsigned long long stride = (unsigned long long)gridDim.x * kWtWG;
    unsigned long long c = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kWtWG + t; i < n; i += stride)
        c += i == 0 || tid[i - 1] != tid[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if (lane_id() == 0 && c) atomicAdd(&s_sum, c);
    __syncthreads();
    if (t == 0 && s_sum) atomicAdd(&tstat[kTsRuns], s_sum);
}

// the old table's keys into the grown one: keys are unique, so the thread that claims a key is the
// only writer of its time
__global__ __launch_bounds__(kWtWG) void k_wt_rehash(const WtSlot* __restrict__ old, unsigned long long old_slots,
                                                     WtSlot* __restrict__ tab, unsigned long long slots,
                                                     unsigned long long* __restrict__ tstat) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kWtWG;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kWtWG + threadIdx.x; i <= old_slots; i += stride) {
        const WtSlot v = wt_load(old + i);
        if (v.key == 0ull) continue;
        if (i == old_slots) {  // traceId 0
            *reinterpret_cast<ulonglong2*>(tab + slots) = ulonglong2{1ull, v.time};
            continue;
        }
        unsigned long long s = wt_home(v.key, slots), tries = 0;
        for (; tries < slots; ++tries) {
            if (atomicCAS(&tab[s].key, 0ull, v.key) == 0ull) {
                tab[s].time = v.time;
                break;
            }
            s = (s + 1ull) & (slots - 1ull);
        }
        if (tries == slots) atomicAdd(&tstat[kTsFull], 1ull);
    }
}

// time[id] = min(time[id], kmin), id entering the table when it is new; true when this call claimed it
__device__ inline bool wt_update(WtSlot* __restrict__ tab, unsigned long long slots, unsigned long long id,
                                 unsigned long long kmin, unsigned long long* __restrict__ tstat) {
    const unsigned long long want = id ? id : 1ull;
    unsigned long long s = id ? wt_home(id, slots) : slots;
    for (unsigned long long tries = 0; tries < slots; ++tries) {
        WtSlot* p = tab + s;
        const WtSlot v = wt_load(p);
        unsigned long long k = v.key;
        bool claimed = false;
        if (k == 0ull) {
            k = atomicCAS(&p->key, 0ull, want);
            claimed = k == 0ull;
            if (claimed) k = want;
        }
        if (k == want) {
            if (v.time > kmin) atomicMin(&p->time, kmin);
            return claimed;
        }
        s = (s + 1ull) & (slots - 1ull);
    }
    atomicAdd(&tstat[kTsFull], 1ull);
    return false;
}

__device__ inline bool wt_find(const WtSlot* __restrict__ tab, unsigned long long slots, unsigned long long id,
                               unsigned long long* time) {
    if (slots == 0ull) return false;
    if (id == 0ull) {
        const WtSlot v = wt_load(tab + slots);
        *time = v.time;
        return v.key != 0ull;
    }
    unsigned long long s = wt_home(id, slots);
    for (unsigned long long tries = 0; tries < slots; ++tries) {
        const WtSlot v = wt_load(tab + s);
        if (v.key == id) {
            *time = v.time;
            return true;
        }
        if (v.key == 0ull) return false;
        s = (s + 1ull) & (slots - 1ull);
    }
    return false;
}

// the row's pieces of runs: lanes [s, e] around this lane with equal traceId (lane 0 starts a piece
// whatever came before the row), and the minimum timed key over them in lane s (k_win_time's scheme)
struct RowPiece {
    uint32_t s;
    bool any_timed;
    unsigned long long kmin;
};

__device__ inline RowPiece row_piece(unsigned long long mask, bool timed, unsigned long long key) {
    const uint32_t lane = lane_id();
    const unsigned long long mm = mask & (~0ull >> (63 - lane));
    const unsigned long long above = lane == 63 ? 0ull : mask & (~0ull << (lane + 1));
    RowPiece p;
    p.s = mm ? 63u - (uint32_t)__clzll((long long)mm) : 0u;
    const uint32_t e = above ? (uint32_t)__ffsll((long long)above) - 2u : 63u;
    const unsigned long long seg = (~0ull >> (63 - e)) & (~0ull << p.s);
    p.any_timed = (__ballot(timed) & seg) != 0ull;
    p.kmin = key;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_down(p.kmin, off);
        if (lane + off <= e && o < p.kmin) p.kmin = o;
    }
    return p;
}

// one table update per (run, row of 64 records); a wave walks rows
__global__ __launch_bounds__(kWtWG) void k_wt_observe(const unsigned long long* __restrict__ tid,
                                                      const long long* __restrict__ ts, const uint32_t* __restrict__ fl,
                                                      unsigned long long n, WtSlot* __restrict__ tab,
                                                      unsigned long long slots, unsigned long long* __restrict__ tstat) {
    const uint32_t lane = lane_id();
    const unsigned long long waves = (unsigned long long)gridDim.x * (kWtWG / 64);
    const unsigned long long rows = (n + 63ull) / 64ull;
    uint32_t claimed = 0;
    for (unsigned long long row = (unsigned long long)blockIdx.x * (kWtWG / 64) + (threadIdx.x >> 6); row < rows;
         row += waves) {
        const unsigned long long i = row * 64ull + lane;
        const bool valid = i < n;
        const unsigned long long id = valid ? tid[i] : 0ull;
        const unsigned long long prev = valid && lane > 0 ? tid[i - 1] : 0ull;
        const uint32_t f = valid ? fl[i] : 0u;
        const long long t = valid ? ts[i] : 0ll;
        const bool timed = (f & ZK_F_HAS_ANNOTATIONS) != 0u;
        const unsigned long long mask = __ballot(valid && (lane == 0 || id != prev));
        const RowPiece p = row_piece(mask, timed, timed ? (unsigned long long)t ^ kSign : kKeyNone);
        bool c = false;
        if (valid && lane == p.s && p.any_timed) c = wt_update(tab, slots, id, p.kmin, tstat);
        claimed += (uint32_t)__popcll(__ballot(c));
    }
    if (lane == 0 && claimed) atomicAdd(&tstat[kTsTraces], (unsigned long long)claimed);
}

// table mode's time pass: win[i] = class of record i by its trace's time in the table. The first lane
// of every row piece probes, the piece takes its answer. Every range is left with no entering and no
// leaving run, so record_class() is win[i] and the later passes run as they are.
__global__ __launch_bounds__(kWinWG) void k_wt_lookup(const unsigned long long* __restrict__ tid,
                                                      const uint32_t* __restrict__ fl, unsigned long long n,
                                                      unsigned long long range_records, WinRule rule,
                                                      const WtSlot* __restrict__ tab, unsigned long long slots,
                                                      uint16_t* __restrict__ win, WinRange* __restrict__ rs,
                                                      long long* __restrict__ gstat,
                                                      unsigned long long* __restrict__ unobserved) {
    __shared__ uint32_t s_c[5];
    const int t = threadIdx.x;
    const uint32_t lane = lane_id();
    const unsigned long long r0 = (unsigned long long)blockIdx.x * range_records;
    const unsigned long long r1 = r0 + range_records < n ? r0 + range_records : n;
    if (t < 5) s_c[t] = 0u;
    __syncthreads();
    uint32_t c_w = 0, c_b = 0, c_a = 0, c_u = 0, c_x = 0;
    for (unsigned long long base = r0; base < r1; base += kWinWG) {
        const unsigned long long i = base + t;
        const bool valid = i < r1;
        const unsigned long long id = valid ? tid[i] : 0ull;
        const unsigned long long prev = valid && i > 0 ? tid[i - 1] : 0ull;
        const uint32_t f = valid ? fl[i] : 0u;
        const bool diff = valid && (i == 0 || id != prev);  // a run starts here
        const unsigned long long mask = __ballot(valid && (lane == 0 || diff));
        const unsigned long long mm = mask & (~0ull >> (63 - lane));
        const uint32_t s = mm ? 63u - (uint32_t)__clzll((long long)mm) : 0u;
        uint32_t cls = 0u;
        if (valid && lane == s) {
            unsigned long long key = kKeyNone;
            const bool found = wt_find(tab, slots, id, &key);
            cls = win_class(key, found, rule) | (found ? 0u : 0x8000u);
        }
        cls = __shfl(cls, (int)s);
        const bool found = (cls & 0x8000u) == 0u;
        cls &= 0x7FFFu;
        if (valid) {
            win[i] = (uint16_t)cls;
            if (diff) {
                c_w += cls < rule.W;
                c_b += cls == rule.W;
                c_a += cls == rule.W + 1;
                c_u += cls == rule.W + 2;
            }
            c_x += !found && (f & ZK_F_HAS_ANNOTATIONS) != 0u;
        }
    }
    if (c_w) atomicAdd(&s_c[0], c_w);
    if (c_b) atomicAdd(&s_c[1], c_b);
    if (c_a) atomicAdd(&s_c[2], c_a);
    if (c_u) atomicAdd(&s_c[3], c_u);
    if (c_x) atomicAdd(&s_c[4], c_x);
    __syncthreads();
    if (t == 0) {
        WinRange o{};
        o.first_start = r0;
        for (int c = 0; c < 4; ++c) o.runs[c] = s_c[c];
        o.pad = s_c[4];  // the range's unobserved records
        rs[blockIdx.x] = o;
        if (s_c[4]) atomicAdd(unobserved, (unsigned long long)s_c[4]);
        if (blockIdx.x == 0) {
            for (int c = 0; c < 4; ++c) gstat[c] = 0;
            gstat[4] = (long long)n;  // held_from: nothing is held
            gstat[5] = 0;
        }
    }
}

// zk_win_table_lookup
__global__ __launch_bounds__(kWtWG) void k_wt_query(const unsigned long long* __restrict__ ids, unsigned long long n,
                                                    const WtSlot* __restrict__ tab, unsigned long long slots,
                                                    long long* __restrict__ t_out, uint8_t* __restrict__ found_out) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kWtWG;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kWtWG + threadIdx.x; i < n; i += stride) {
        unsigned long long key = kKeyNone;
        const bool found = wt_find(tab, slots, ids[i], &key);
        t_out[i] = (long long)(key ^ kSign);
        found_out[i] = found ? 1 : 0;
    }
}

uint32_t wt_grid(uint64_t items) {
    const uint64_t g = (items + kWtWG - 1) / kWtWG;
    return (uint32_t)(g < 1 ? 1 : g > kWtMaxGrid ? kWtMaxGrid : g);
}

bool rule_ok(int64_t window_us, uint32_t W) { return window_us > 0 && W >= 1 && W <= ZK_WIN_MAX_WINDOWS; }

void win_plan(uint64_t n, uint64_t* range_records, uint64_t* ranges) {
    const uint64_t chunks = (n + kWinChunk - 1) / kWinChunk;
    uint64_t per = (chunks + kWinMaxRanges - 1) / kWinMaxRanges;
    if (per == 0) per = 1;
    *range_records = per * kWinChunk;
    *ranges = (n + *range_records - 1) / *range_records;
}

}  // namespace
}  // namespace zk

using namespace zk;

struct zk_win {
    int device = 0;
    hipStream_t stream = nullptr, own = nullptr;
    WinRule rule{0, 1, 1};
    // scratch, allocated on first use and grown
    void* win = nullptr;     // u16 [n]
    void* ranges = nullptr;  // WinRange [kWinMaxRanges] + gstat
    void* matrix = nullptr;  // u64 [(W + 1) * ranges + 1]
    void* tmp = nullptr;     // the scan's workspace
    void* res = nullptr;     // u64 [W + 2 + kResTail]
    void* stage = nullptr;   // the seven columns of a host batch
    hipEvent_t ev[kWinPhases + 1] = {};  // around the passes of the last partition (zk_win_phase_ms)
    bool timing = false;  // zk_win_config.timing: record the events
    bool timed = false;
    bool timed_table = false;  // the last timed partition ran in table mode
    size_t win_bytes = 0, ranges_bytes = 0, matrix_bytes = 0, tmp_bytes = 0, res_bytes = 0, stage_bytes = 0;
    // the trace-time table
    void* table = nullptr;   // WtSlot [slots + 1]
    void* tstat = nullptr;   // u64 [kTsWords]: traces, the last batch's runs, probe loops that ran out
    void* query = nullptr;   // zk_win_table_lookup: ids, times, found
    uint64_t slots = 0;
    size_t query_bytes = 0;
    hipEvent_t oev[4] = {};  // around the passes of the last observe (zk_win_observe_ms)
    bool otimed = false;
    std::string err;
};

namespace {

zk_status wfail(zk_win* h, zk_status s, const std::string& m) {
    if (h) h->err = m;
    return s;
}

#define WIN_HIP(h, call)                                                                           \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess) return wfail(h, is_refusal(_e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP,       \
                                           std::string(#call) + ": " + launch_error_str(_e));      \
    } while (0)

// at least `need` bytes behind *p: a larger block first, then the old one freed; a refused allocation
// is ZK_ERR_CAPACITY and leaves *p as it was
zk_status grow(zk_win* h, void** p, size_t* have, size_t need, const char* what) {
    if (need <= *have && *p) return ZK_OK;
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, need ? need : 8);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (e != hipErrorOutOfMemory) return wfail(h, ZK_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        return wfail(h, ZK_ERR_CAPACITY, std::string("no device memory for ") + what);
    }
    if (*p) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(*p);
    }
    *p = q;
    *have = need;
    return ZK_OK;
}

constexpr size_t kColBytes[7] = {8, 8, 8, 8, 8, 4, 4};

const void* col_ptr(const zk_span_cols* c, int k) {
    switch (k) {
        case 0: return c->trace_id;
        case 1: return c->span_id;
        case 2: return c->parent_id;
        case 3: return c->first_ts;
        case 4: return c->last_ts;
        case 5: return c->service_id;
        default: return c->flags;
    }
}

zk_status ensure_tstat(zk_win* h) {
    if (h->tstat) return ZK_OK;
    void* q = nullptr;
    size_t have = 0;
    const zk_status st = grow(h, &q, &have, kTsWords * 8, "the table's counters");
    if (st != ZK_OK) return st;
    WIN_HIP(h, hipMemsetAsync(q, 0, kTsWords * 8, h->stream));
    h->tstat = q;
    return ZK_OK;
}

// The table at `want` slots or more (a power of two, at least kWtMinSlots): a new table is made and
// cleared, the old one's keys move into it (k_wt_rehash) and the old one is freed after the stream
// has drained. rehashed: whether the table grew. A refused allocation changes nothing.
zk_status ensure_slots(zk_win* h, uint64_t want, bool* rehashed) {
    if (rehashed) *rehashed = false;
    if (want <= h->slots && h->table) return ZK_OK;
    if (want > kWtMaxSlots) return wfail(h, ZK_ERR_CAPACITY, "a trace-time table of more than 2^40 slots");
    uint64_t slots = kWtMinSlots;
    while (slots < want) slots <<= 1;
    zk_status st = ensure_tstat(h);
    if (st != ZK_OK) return st;
    void* q = nullptr;
    size_t have = 0;
    if ((st = grow(h, &q, &have, (size_t)(slots + 1) * sizeof(WtSlot), "the trace-time table (16 B per slot)")) != ZK_OK)
        return st;
    hipError_t e = launch_checked("k_wt_clear", k_wt_clear, dim3(wt_grid(slots + 1)), dim3(kWtWG), 0, h->stream, (WtSlot*)q,
                                  (unsigned long long)(slots + 1));
    if (e == hipSuccess && h->table)
        e = launch_checked("k_wt_rehash", k_wt_rehash, dim3(wt_grid(h->slots + 1)), dim3(kWtWG), 0, h->stream,
                           (const WtSlot*)h->table, (unsigned long long)h->slots, (WtSlot*)q, (unsigned long long)slots,
                           (unsigned long long*)h->tstat);
    if (e == hipSuccess && h->table) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(q);
        return wfail(h, is_refusal(e) ? ZK_ERR_CAPACITY : ZK_ERR_HIP, std::string("growing the trace-time table: ") + launch_error_str(e));
    }
    if (h->table) (void)hipFree(h->table);
    if (rehashed) *rehashed = h->table != nullptr;
    h->table = q;
    h->slots = slots;
    return ZK_OK;
}

}  // namespace

extern "C" {

zk_status zk_win_index(int64_t t, int64_t origin_us, int64_t window_us, uint32_t num_windows, uint32_t* w) {
    if (!w || !rule_ok(window_us, num_windows)) return ZK_ERR_INVALID_ARG;
    const uint32_t c = win_class((unsigned long long)t ^ kSign, true, WinRule{origin_us, (uint64_t)window_us, num_windows});
    *w = c < num_windows ? c : num_windows;
    return ZK_OK;
}

zk_status zk_win_create(const zk_win_config* cfg, zk_win** out) {
    ZK_GUARD_BEGIN
    if (!cfg || !out) return ZK_ERR_INVALID_ARG;
    *out = nullptr;
    if (!rule_ok(cfg->window_us, cfg->num_windows)) return ZK_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || cfg->device < 0 || cfg->device >= ndev) return ZK_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return ZK_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return ZK_ERR_NO_DEVICE;
    if (hipSetDevice(cfg->device) != hipSuccess) return ZK_ERR_HIP;
    zk_win* h = new zk_win();
    h->device = cfg->device;
    h->rule = WinRule{cfg->origin_us, (uint64_t)cfg->window_us, cfg->num_windows};
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

zk_status zk_win_destroy(zk_win* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void* p : {h->win, h->ranges, h->matrix, h->tmp, h->res, h->stage, h->table, h->tstat, h->query})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->oev)
        if (e) (void)hipEventDestroy(e);
    if (h->own) (void)hipStreamDestroy(h->own);
    delete h;
    return ZK_OK;
    ZK_GUARD_END
}

const char* zk_win_last_error(const zk_win* h) { return h ? h->err.c_str() : "null handle"; }

zk_status zk_win_set_windows(zk_win* h, int64_t origin_us, int64_t window_us, uint32_t num_windows) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!rule_ok(window_us, num_windows)) return wfail(h, ZK_ERR_INVALID_ARG, "window_us <= 0, or num_windows outside 1..1024");
    h->rule = WinRule{origin_us, (uint64_t)window_us, num_windows};
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_win_plan(const zk_win* h, uint64_t n, uint64_t* chunk_records, uint64_t* range_records, uint64_t* ranges) {
    (void)h;  // (the geometry does not depend on the handle: NULL is accepted, so a host without a device can plan)
    if (n > kWinMaxRecords) return ZK_ERR_INVALID_ARG;
    uint64_t rr = 0, nr = 0;
    win_plan(n, &rr, &nr);
    if (chunk_records) *chunk_records = kWinChunk;
    if (range_records) *range_records = rr;
    if (ranges) *ranges = nr;
    return ZK_OK;
}

zk_status zk_win_phase_ms(zk_win* h, double out[6]) {
    ZK_GUARD_BEGIN
    if (!h || !out) return ZK_ERR_INVALID_ARG;
    if (!h->timed) return wfail(h, ZK_ERR_INVALID_ARG, "no timed partition has run (zk_win_config.timing)");
    WIN_HIP(h, hipSetDevice(h->device));
    for (int k = 0; k < kWinPhases; ++k) {
        float ms = 0.f;
        WIN_HIP(h, hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]));
        out[k] = ms;
    }
    if (h->timed_table) out[1] = 0.0;  // (no resolve in table mode: slot 0 is the lookup)
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_win_partition(zk_win* h, const zk_span_cols* in, uint32_t flags, const zk_span_cols* out, uint64_t* offsets,
                           zk_win_counts* counts) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!in || !out || !offsets) return wfail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (flags & ~(ZK_BATCH_DEVICE_PTRS | ZK_BATCH_TRACE_CLUSTERED | ZK_WIN_HOLD_LAST | ZK_WIN_TRACE_TABLE))
        return wfail(h, ZK_ERR_INVALID_ARG, "unknown batch flag");
    const bool table_mode = (flags & ZK_WIN_TRACE_TABLE) != 0;
    if (table_mode && (flags & ZK_WIN_HOLD_LAST))
        return wfail(h, ZK_ERR_INVALID_ARG, "ZK_WIN_HOLD_LAST with ZK_WIN_TRACE_TABLE: nothing needs holding");
    if (!table_mode && !(flags & ZK_BATCH_TRACE_CLUSTERED))
        return wfail(h, ZK_ERR_UNSUPPORTED,
                     "without ZK_WIN_TRACE_TABLE the window partition takes trace-clustered batches only");
    const uint64_t n = in->n;
    const uint32_t W = h->rule.W;
    if (n > kWinMaxRecords) return wfail(h, ZK_ERR_UNSUPPORTED, "more than 2^40 records in one batch");
    zk_win_counts cz;
    memset(&cz, 0, sizeof cz);
    if (n == 0) {
        for (uint32_t w = 0; w < W + 2; ++w) offsets[w] = 0;
        if (counts) *counts = cz;
        return ZK_OK;
    }
    const bool dev_in = (flags & ZK_BATCH_DEVICE_PTRS) != 0;
    for (int k = 0; k < 7; ++k)
        if (!col_ptr(in, k) || !col_ptr(out, k)) return wfail(h, ZK_ERR_INVALID_ARG, "null column");
    for (int a = 0; dev_in && a < 7; ++a) {
        const uintptr_t o0 = (uintptr_t)col_ptr(out, a), o1 = o0 + n * kColBytes[a];
        for (int b = 0; b < 7; ++b) {
            const uintptr_t i0 = (uintptr_t)col_ptr(in, b), i1 = i0 + n * kColBytes[b];
            if (o0 < i1 && i0 < o1) return wfail(h, ZK_ERR_INVALID_ARG, "out overlaps in");
        }
    }
    WIN_HIP(h, hipSetDevice(h->device));
    uint64_t rr = 0, nr = 0;
    win_plan(n, &rr, &nr);
    const uint32_t ranges = (uint32_t)nr;
    const uint64_t items = (uint64_t)(W + 1) * ranges + 1;
    size_t tb = 0;
    WIN_HIP(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                (int)items, h->stream));
    zk_status st;
    if ((st = grow(h, &h->win, &h->win_bytes, n * 2, "the window ids (2 B per record)")) != ZK_OK) return st;
    if ((st = grow(h, &h->ranges, &h->ranges_bytes, kWinMaxRanges * sizeof(WinRange) + kGstatWords * 8,
                   "the range summaries")) != ZK_OK)
        return st;
    if ((st = grow(h, &h->matrix, &h->matrix_bytes, items * 8, "the window x range counts")) != ZK_OK) return st;
    if ((st = grow(h, &h->tmp, &h->tmp_bytes, tb ? tb : 8, "the scan's workspace")) != ZK_OK) return st;
    if ((st = grow(h, &h->res, &h->res_bytes, (ZK_WIN_MAX_WINDOWS + 2 + kResTail + 1) * 8, "the result words")) != ZK_OK)
        return st;
    WinCols ic{};
    if (dev_in) {
        ic = WinCols{(const unsigned long long*)in->trace_id, (const unsigned long long*)in->span_id,
                     (const unsigned long long*)in->parent_id, (const long long*)in->first_ts, (const long long*)in->last_ts,
                     in->service_id, in->flags};
    } else {
        // a host batch: staged column by column (each 256-B aligned)
        size_t at[7], total = 0;
        for (int k = 0; k < 7; ++k) {
            at[k] = total;
            total += (n * kColBytes[k] + 255) / 256 * 256;
        }
        if ((st = grow(h, &h->stage, &h->stage_bytes, total, "staging a host batch (48 B per record)")) != ZK_OK) return st;
        uint8_t* s = (uint8_t*)h->stage;
        for (int k = 0; k < 7; ++k)
            WIN_HIP(h, hipMemcpyAsync(s + at[k], col_ptr(in, k), n * kColBytes[k], hipMemcpyHostToDevice, h->stream));
        ic = WinCols{(const unsigned long long*)(s + at[0]), (const unsigned long long*)(s + at[1]),
                     (const unsigned long long*)(s + at[2]), (const long long*)(s + at[3]), (const long long*)(s + at[4]),
                     (const uint32_t*)(s + at[5]), (const uint32_t*)(s + at[6])};
    }
    const WinOutCols oc{(unsigned long long*)out->trace_id, (unsigned long long*)out->span_id, (unsigned long long*)out->parent_id,
                        (long long*)out->first_ts, (long long*)out->last_ts, (uint32_t*)out->service_id, (uint32_t*)out->flags};
    uint16_t* win = (uint16_t*)h->win;
    WinRange* rs = (WinRange*)h->ranges;
    long long* gstat = (long long*)((uint8_t*)h->ranges + kWinMaxRanges * sizeof(WinRange));
    unsigned long long* M = (unsigned long long*)h->matrix;
    unsigned long long* res = (unsigned long long*)h->res;
    const int hold = (flags & ZK_WIN_HOLD_LAST) ? 1 : 0;
    const bool timing = h->timing;
    for (hipEvent_t& e : h->ev)
        if (timing && !e) WIN_HIP(h, hipEventCreate(&e));
    h->timed = false;
    unsigned long long* unobserved = res + W + 2 + kResTail;  // (after what k_win_final writes)
    if (table_mode) WIN_HIP(h, hipMemsetAsync(unobserved, 0, 8, h->stream));
    if (timing) WIN_HIP(h, hipEventRecord(h->ev[0], h->stream));
    if (table_mode) {
        WIN_HIP(h, launch_checked("k_wt_lookup", k_wt_lookup, dim3(ranges), dim3(kWinWG), 0, h->stream, ic.trace_id, ic.flags,
                                  (unsigned long long)n, (unsigned long long)rr, h->rule, (const WtSlot*)h->table,
                                  (unsigned long long)h->slots, win, rs, gstat, unobserved));
        if (timing) WIN_HIP(h, hipEventRecord(h->ev[1], h->stream));
    } else {
        WIN_HIP(h, launch_checked("k_win_time", k_win_time, dim3(ranges), dim3(kWinWG), 0, h->stream, ic.trace_id,
                                  ic.first_ts, ic.flags, (unsigned long long)n, (unsigned long long)rr, h->rule, win, rs));
        if (timing) WIN_HIP(h, hipEventRecord(h->ev[1], h->stream));
        WIN_HIP(h, launch_checked("k_win_resolve", k_win_resolve, dim3(1), dim3(kWinWG), 0, h->stream, rs, ranges,
                                  (unsigned long long)n, h->rule, hold, gstat));
    }
    if (timing) WIN_HIP(h, hipEventRecord(h->ev[2], h->stream));
    WIN_HIP(h, launch_checked("k_win_hist", k_win_hist, dim3(ranges), dim3(kWinWG), 0, h->stream, (const uint16_t*)win, rs,
                              (unsigned long long)n, (unsigned long long)rr, W, ranges, (const long long*)gstat, M));
    if (timing) WIN_HIP(h, hipEventRecord(h->ev[3], h->stream));
    WIN_HIP(h, hipcub::DeviceScan::ExclusiveSum(h->tmp, tb, M, M, (int)items, h->stream));
    if (timing) WIN_HIP(h, hipEventRecord(h->ev[4], h->stream));
    WIN_HIP(h, launch_checked("k_win_scatter", k_win_scatter, dim3(ranges), dim3(kWinWG), 0, h->stream, ic, oc,
                              (const uint16_t*)win, (const WinRange*)rs, (unsigned long long)n, (unsigned long long)rr, W, ranges,
                              (const long long*)gstat, (const unsigned long long*)M));
    if (timing) WIN_HIP(h, hipEventRecord(h->ev[5], h->stream));
    WIN_HIP(h, launch_checked("k_win_final", k_win_final, dim3(1), dim3(kWinWG), 0, h->stream, (const unsigned long long*)M,
                              ranges, W, (const WinRange*)rs, (const long long*)gstat, res));
    if (timing) WIN_HIP(h, hipEventRecord(h->ev[6], h->stream));
    unsigned long long host[ZK_WIN_MAX_WINDOWS + 2 + kResTail + 1];
    WIN_HIP(h, hipMemcpyAsync(host, res, (size_t)(W + 2 + kResTail + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    WIN_HIP(h, hipStreamSynchronize(h->stream));  // (also: the staging copies have read the host batch)
    h->timed = timing;
    h->timed_table = table_mode;
    for (uint32_t w = 0; w < W + 2; ++w) offsets[w] = host[w];
    const unsigned long long* tail = host + W + 2;
    cz.partitioned_runs = tail[0];
    cz.before_runs = tail[1];
    cz.after_runs = tail[2];
    cz.untimed_runs = tail[3];
    cz.partitioned_records = host[W];
    cz.before_records = tail[4];
    cz.after_records = tail[5];
    cz.untimed_records = tail[6];
    cz.held_from = tail[7];
    cz.held_runs = tail[8];
    cz.held_records = n - tail[7];
    cz.unobserved_records = table_mode ? tail[kResTail] : 0;
    if (counts) *counts = cz;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_win_observe(zk_win* h, const zk_span_cols* in, uint32_t flags) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!in) return wfail(h, ZK_ERR_INVALID_ARG, "null argument");
    if (flags & ~(ZK_BATCH_DEVICE_PTRS | ZK_BATCH_TRACE_CLUSTERED)) return wfail(h, ZK_ERR_INVALID_ARG, "unknown batch flag");
    const uint64_t n = in->n;
    if (n > kWinMaxRecords) return wfail(h, ZK_ERR_UNSUPPORTED, "more than 2^40 records in one batch");
    if (n == 0) return ZK_OK;
    if (!in->trace_id || !in->first_ts || !in->flags) return wfail(h, ZK_ERR_INVALID_ARG, "null column");
    WIN_HIP(h, hipSetDevice(h->device));
    zk_status st = ensure_tstat(h);
    if (st != ZK_OK) return st;
    const unsigned long long* tid = (const unsigned long long*)in->trace_id;
    const long long* ts = (const long long*)in->first_ts;
    const uint32_t* fl = in->flags;
    if (!(flags & ZK_BATCH_DEVICE_PTRS)) {
        // a host batch: the three columns the table reads, staged (each 256-B aligned)
        const size_t a8 = (n * 8 + 255) / 256 * 256, a4 = (n * 4 + 255) / 256 * 256;
        if ((st = grow(h, &h->stage, &h->stage_bytes, 2 * a8 + a4, "staging a host batch (20 B per record)")) != ZK_OK)
            return st;
        uint8_t* s = (uint8_t*)h->stage;
        WIN_HIP(h, hipMemcpyAsync(s, in->trace_id, n * 8, hipMemcpyHostToDevice, h->stream));
        WIN_HIP(h, hipMemcpyAsync(s + a8, in->first_ts, n * 8, hipMemcpyHostToDevice, h->stream));
        WIN_HIP(h, hipMemcpyAsync(s + 2 * a8, in->flags, n * 4, hipMemcpyHostToDevice, h->stream));
        tid = (const unsigned long long*)s;
        ts = (const long long*)(s + a8);
        fl = (const uint32_t*)(s + 2 * a8);
    }
    unsigned long long* tstat = (unsigned long long*)h->tstat;
    const bool timing = h->timing;
    for (hipEvent_t& e : h->oev)
        if (timing && !e) WIN_HIP(h, hipEventCreate(&e));
    h->otimed = false;
    WIN_HIP(h, hipMemsetAsync(tstat + kTsRuns, 0, 8, h->stream));
    if (timing) WIN_HIP(h, hipEventRecord(h->oev[0], h->stream));
    WIN_HIP(h, launch_checked("k_wt_runs", k_wt_runs, dim3(wt_grid(n)), dim3(kWtWG), 0, h->stream, tid, (unsigned long long)n,
                              tstat));
    if (timing) WIN_HIP(h, hipEventRecord(h->oev[1], h->stream));
    unsigned long long host[kTsWords];
    WIN_HIP(h, hipMemcpyAsync(host, tstat, sizeof host, hipMemcpyDeviceToHost, h->stream));
    WIN_HIP(h, hipStreamSynchronize(h->stream));  // the call's one synchronisation (also: the staging copies are done)
    if (host[kTsFull]) return wfail(h, ZK_ERR_HIP, "the trace-time table ran full (the sizing rule was broken)");
    if (host[kTsRuns] == 0 || host[kTsRuns] > n) return wfail(h, ZK_ERR_HIP, "run count out of range");
    // load <= 1/2 whatever the batch holds: every run might be a new trace
    if ((st = ensure_slots(h, 2 * (host[kTsTraces] + host[kTsRuns]), nullptr)) != ZK_OK) return st;
    if (timing) WIN_HIP(h, hipEventRecord(h->oev[2], h->stream));
    const uint64_t rows = (n + 63) / 64;
    WIN_HIP(h, launch_checked("k_wt_observe", k_wt_observe, dim3(wt_grid(rows * 64)), dim3(kWtWG), 0,
                              h->stream, tid, ts, fl, (unsigned long long)n, (WtSlot*)h->table, (unsigned long long)h->slots,
                              tstat));
    if (timing) WIN_HIP(h, hipEventRecord(h->oev[3], h->stream));
    h->otimed = timing;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_win_observe_ms(zk_win* h, double out[3]) {
    ZK_GUARD_BEGIN
    if (!h || !out) return ZK_ERR_INVALID_ARG;
    if (!h->otimed) return wfail(h, ZK_ERR_INVALID_ARG, "no timed observe has run (zk_win_config.timing)");
    WIN_HIP(h, hipSetDevice(h->device));
    WIN_HIP(h, hipEventSynchronize(h->oev[3]));
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        WIN_HIP(h, hipEventElapsedTime(&ms, h->oev[k], h->oev[k + 1]));
        out[k] = ms;
    }
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_win_table_reset(zk_win* h) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (!h->table) return ZK_OK;
    WIN_HIP(h, hipSetDevice(h->device));
    WIN_HIP(h, launch_checked("k_wt_clear", k_wt_clear, dim3(wt_grid(h->slots + 1)), dim3(kWtWG), 0, h->stream,
                              (WtSlot*)h->table, (unsigned long long)(h->slots + 1)));
    WIN_HIP(h, hipMemsetAsync(h->tstat, 0, kTsWords * 8, h->stream));
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_win_table_reserve(zk_win* h, uint64_t traces) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (traces > kWtMaxSlots / 2) return wfail(h, ZK_ERR_CAPACITY, "a trace-time table of more than 2^40 slots");
    WIN_HIP(h, hipSetDevice(h->device));
    return ensure_slots(h, 2 * traces, nullptr);
    ZK_GUARD_END
}

zk_status zk_win_table_info(zk_win* h, uint64_t* slots, uint64_t* traces, uint64_t* bytes) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    unsigned long long host[kTsWords] = {};
    if (h->tstat) {
        WIN_HIP(h, hipSetDevice(h->device));
        WIN_HIP(h, hipMemcpyAsync(host, h->tstat, sizeof host, hipMemcpyDeviceToHost, h->stream));
        WIN_HIP(h, hipStreamSynchronize(h->stream));
        if (host[kTsFull]) return wfail(h, ZK_ERR_HIP, "the trace-time table ran full (the sizing rule was broken)");
    }
    if (slots) *slots = h->slots;
    if (traces) *traces = host[kTsTraces];
    if (bytes) *bytes = h->table ? (h->slots + 1) * sizeof(WtSlot) : 0;
    return ZK_OK;
    ZK_GUARD_END
}

zk_status zk_win_table_lookup(zk_win* h, const uint64_t* trace_ids, uint64_t n, uint32_t flags, int64_t* t, uint8_t* found) {
    ZK_GUARD_BEGIN
    if (!h) return ZK_ERR_INVALID_ARG;
    if (flags & ~ZK_BATCH_DEVICE_PTRS) return wfail(h, ZK_ERR_INVALID_ARG, "unknown flag");
    if (n > kWinMaxRecords) return wfail(h, ZK_ERR_UNSUPPORTED, "more than 2^40 ids in one call");
    if (n == 0) return ZK_OK;
    if (!trace_ids || !t || !found) return wfail(h, ZK_ERR_INVALID_ARG, "null argument");
    WIN_HIP(h, hipSetDevice(h->device));
    const bool dev = (flags & ZK_BATCH_DEVICE_PTRS) != 0;
    const size_t a8 = (n * 8 + 255) / 256 * 256;
    zk_status st = grow(h, &h->query, &h->query_bytes, 2 * a8 + n, "the lookup's ids and answers (17 B per id)");
    if (st != ZK_OK) return st;
    uint8_t* q = (uint8_t*)h->query;
    const unsigned long long* ids = (const unsigned long long*)trace_ids;
    if (!dev) {
        WIN_HIP(h, hipMemcpyAsync(q, trace_ids, n * 8, hipMemcpyHostToDevice, h->stream));
        ids = (const unsigned long long*)q;
    }
    WIN_HIP(h, launch_checked("k_wt_query", k_wt_query, dim3(wt_grid(n)), dim3(kWtWG), 0, h->stream, ids, (unsigned long long)n,
                              (const WtSlot*)h->table, (unsigned long long)h->slots, (long long*)(q + a8), q + 2 * a8));
    WIN_HIP(h, hipMemcpyAsync(t, q + a8, n * 8, hipMemcpyDeviceToHost, h->stream));
    WIN_HIP(h, hipMemcpyAsync(found, q + 2 * a8, n, hipMemcpyDeviceToHost, h->stream));
    WIN_HIP(h, hipStreamSynchronize(h->stream));
    return ZK_OK;
    ZK_GUARD_END
}

}  // extern "C"
