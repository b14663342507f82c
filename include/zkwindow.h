/*
 * zkwindow.h -- dependencies per time window: the device trace-time partition.
 *
 * ZipkinAggregateJob turns its whole input into ONE record, Dependencies(0, now, links). To store one
 * record per hour or day (the Cassandra store keys its rows by day, getDependencies(start, end) sums
 * records over a window) a batch of span fragments has to be split by time first. This pass does that
 * split in HBM: it gives every trace a time and moves the records of a trace-clustered batch into
 * window order, so that every window's slice is again a trace-clustered batch of whole traces that
 * zk_deps_accumulate (zkagg.h) takes with ZK_BATCH_DEVICE_PTRS | ZK_BATCH_TRACE_CLUSTERED.
 *
 * Semantics
 *  - A TRACE RUN is a maximal stretch of adjacent records with equal trace_id (the definition the join
 *    uses). Two non-adjacent runs with the same id are two runs.
 *  - A fragment is TIMED when flags & ZK_F_HAS_ANNOTATIONS. The first_ts of any other fragment is not
 *    meaningful and is ignored, also when it is smaller than every real time.
 *  - A run's TRACE TIME t is the minimum first_ts over its timed fragments. A run without a timed
 *    fragment is UNTIMED.
 *  - The WINDOW of a timed run follows from (origin_us, window_us > 0, num_windows = W),
 *    1 <= W <= ZK_WIN_MAX_WINDOWS:
 *      t < origin_us                                       the run is BEFORE
 *      w = ((uint64)t - (uint64)origin_us) / window_us     w >= W: the run is AFTER, else its window is w
 *    No signed subtraction happens: t and origin_us may lie anywhere in int64.
 *  - Output: the input's records in window order 0, 1, ..., W-1, then the REST (the records of the
 *    before, after and untimed runs). Inside each of these W + 1 parts the records keep the input's
 *    relative order: a stable partition. So every trace's fragments stay adjacent, and the output
 *    bytes are a function of the input alone.
 *
 * Conventions are those of zkagg.h: every entry point returns zk_status; a handle is not
 * thread-safe; all device work of a handle is ordered on one HIP stream.
 */
#ifndef ZKWINDOW_H
#define ZKWINDOW_H

#include "zkagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZK_WIN_MAX_WINDOWS 1024u

/* batch flag of zk_win_partition, beside ZK_BATCH_DEVICE_PTRS and ZK_BATCH_TRACE_CLUSTERED: the
   batch's last run is left out of the output (a streaming reader's last trace may continue in its
   next batch); zk_win_counts.held_from is its first record. Carrying those records over is the
   caller's business: nothing is held in the handle. */
#define ZK_WIN_HOLD_LAST (1u << 8)

typedef struct zk_win_config {
    int32_t  device;        /* HIP device ordinal */
    uint32_t num_windows;   /* W, 1..ZK_WIN_MAX_WINDOWS */
    void*    stream;        /* hipStream_t to run on, or NULL for a private stream */
    int64_t  origin_us;     /* start of window 0 */
    int64_t  window_us;     /* > 0 */
    uint32_t timing;        /* 1: record HIP events around the passes (zk_win_phase_ms) */
    uint32_t reserved[7];
} zk_win_config;

/* runs and records of one zk_win_partition call, by what became of them */
typedef struct zk_win_counts {
    uint64_t partitioned_runs, partitioned_records;   /* in a window 0..W-1 */
    uint64_t before_runs, before_records;             /* t < origin */
    uint64_t after_runs, after_records;               /* w >= W */
    uint64_t untimed_runs, untimed_records;           /* no timed fragment */
    uint64_t held_runs, held_records;                 /* ZK_WIN_HOLD_LAST: the last run (else 0) */
    uint64_t held_from;                               /* first held record of the input; n when none */
    uint64_t reserved[5];
} zk_win_counts;

typedef struct zk_win zk_win;

/* A bad config (NULL, window_us <= 0, num_windows 0 or > ZK_WIN_MAX_WINDOWS) is ZK_ERR_INVALID_ARG
   before any device is touched. Scratch (2 B per record and a few MB) is allocated on first use
   and grown; a refused allocation is ZK_ERR_CAPACITY and changes nothing. */
zk_status   zk_win_create(const zk_win_config* cfg, zk_win** out);
zk_status   zk_win_destroy(zk_win* win);
const char* zk_win_last_error(const zk_win* win);
/* re-aim a handle between jobs */
zk_status   zk_win_set_windows(zk_win* win, int64_t origin_us, int64_t window_us, uint32_t num_windows);
/* The geometry the kernels use for n records (no device work): records per LDS chunk, records per
   workgroup range (whole chunks), number of ranges. Any of the three pointers may be NULL, and so may
   `win`: the geometry depends on n alone, so a host without a device can ask for it. */
zk_status   zk_win_plan(const zk_win* win, uint64_t n, uint64_t* chunk_records, uint64_t* range_records,
                        uint64_t* ranges);
/* Partition `in` (n records) into `out` by the handle's windows.
 *   flags    ZK_BATCH_TRACE_CLUSTERED is required (else ZK_ERR_UNSUPPORTED: any-order input is not
 *            taken). ZK_BATCH_DEVICE_PTRS: `in` holds device pointers; without it `in` is host memory,
 *            staged, and the call waits for the staging copy. ZK_WIN_HOLD_LAST: see above.
 *   out      always seven DEVICE columns of capacity in->n (out->n is ignored); it must not overlap
 *            `in` (ZK_ERR_INVALID_ARG). A refused call leaves it unwritten.
 *   offsets  host array of W + 2 entries: window w is out[offsets[w], offsets[w + 1]), the rest is
 *            out[offsets[W], offsets[W + 1]); offsets[W + 1] = n less the held records. The parts lie
 *            back to back, so a part that starts on an odd record is 8-byte (u64 columns) / 4-byte
 *            (u32) aligned only: zk_deps_accumulate wants 16 / 8 for clustered device columns, and
 *            such a part has to be copied to aligned columns first (an even start is used in place).
 *   counts   may be NULL.
 * The call synchronises the stream once, to bring offsets and counts to the host (which needs them to
 * slice). n == 0 is ZK_OK with all zeros. */
zk_status   zk_win_partition(zk_win* win, const zk_span_cols* in, uint32_t flags, const zk_span_cols* out,
                             uint64_t* offsets, zk_win_counts* counts);
/* Device time of the passes of the last zk_win_partition, from HIP events, in ms: the time pass, the
   resolve, the histogram, the scan, the scatter, the final gather. Needs zk_win_config.timing (without it
   no event is recorded); ZK_ERR_INVALID_ARG without it or before the first partition. */
zk_status   zk_win_phase_ms(zk_win* win, double out[6]);
/* The window rule above on the host (no HIP): *w = the window of trace time t, or num_windows when t is
   before or after. ZK_ERR_INVALID_ARG for window_us <= 0, num_windows 0 or > ZK_WIN_MAX_WINDOWS. */
zk_status   zk_win_index(int64_t t, int64_t origin_us, int64_t window_us, uint32_t num_windows, uint32_t* w);

#ifdef __cplusplus
}
#endif
#endif /* ZKWINDOW_H */
