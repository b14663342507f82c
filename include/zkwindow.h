/*
 * zkwindow.h -- dependencies per time window: the device trace-time partition.
 *
 * ZipkinAggregateJob turns its whole input into ONE record, Dependencies(0, now, links). To store one
 * record per hour or day (the Cassandra store keys its rows by day, getDependencies(start, end) sums
 * records over a window) a batch of span fragments has to be split by time first. This pass does that
 * split in HBM: it gives every trace a time and moves the records of a trace-clustered batch into
 * window order, so that every window's slice is again a trace-clustered batch of whole traces that
 * zk_deps_accumulate (zkagg.h) takes with ZK_BATCH_DEVICE_PTRS | ZK_BATCH_TRACE_CLUSTERED. With the
 * trace-time table (below) it also takes records in any order and traces cut at a batch edge.
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
 * The rule above takes a trace's time from ONE run of ONE batch: it needs batches of whole,
 * trace-clustered traces. For records in any order, and for row-order batches cut wherever a reader's
 * buffer filled, the handle owns a TRACE-TIME TABLE that holds across batches:
 *  - zk_win_observe(batch) folds a batch into the table: traceId -> the minimum first_ts over the timed
 *    fragments of every batch observed since the last zk_win_table_reset.
 *  - MEMBERSHIP: only timed fragments enter. A traceId is in the table exactly when some observed
 *    fragment of it was timed, so a stored time of INT64_MAX is a real time and never "none".
 *  - IDEMPOTENCE: the fold is a minimum; observing a batch again leaves every word of the table as it
 *    was, and batches may be observed in any order.
 *  - Layout: open addressing with linear probing in HBM, 16 B per slot {uint64 key, uint64 time}; key =
 *    traceId, 0 = empty; time = first_ts with the sign bit flipped (unsigned order = signed order), all
 *    ones in a fresh slot. `slots` is a power of two and the home slot of a traceId is
 *        zk_mix64(trace_id ^ ZK_WIN_TABLE_SALT) & (slots - 1)
 *    (zk_mix64: the splitmix64 finalizer, z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) *
 *    0x94D049BB133111EB, z ^ z >> 31); a probe walks upwards and wraps to slot 0. TraceId 0, a legal id,
 *    lives in one extra slot at index `slots`, whose key word is a presence flag.
 *  - SIZING: before anything of a batch is inserted the call counts the batch's trace runs and makes
 *    sure that slots >= 2 * (traces in the table + runs in the batch), rounded up to a power of two
 *    (at least 1024). The load so never exceeds 1/2. A trace-clustered batch pays for its traces,
 *    not its records; an any-order batch, where every record is a run, for its records. The table only
 *    grows (the old content is rehashed into the new table); a refused allocation is ZK_ERR_CAPACITY
 *    and changes nothing.
 *  - zk_win_partition with ZK_WIN_TRACE_TABLE classes every RECORD by its trace's time in the table
 *    and then partitions exactly as above. The output is the same stable partition, over per-record
 *    classes, and its bytes are a function of (input, table) alone. For a trace-clustered batch every
 *    part is again trace-clustered; a trace cut at the end of batch k is the last run of its window's
 *    part of batch k and its continuation the first run of the same window's part of batch k + 1,
 *    which is what ZK_BATCH_CONTINUES (zkagg.h) joins. For an any-order batch a part is in any order,
 *    but every fragment of a trace, from every observed batch, lies in the same window.
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
/* batch flag of zk_win_partition: trace times come from the handle's trace-time table (see above), so
   the batch need not hold whole traces. ZK_BATCH_TRACE_CLUSTERED is then optional; ZK_WIN_HOLD_LAST
   together with it is ZK_ERR_INVALID_ARG (nothing needs holding). Observe every batch first: a timed
   record whose traceId is not in the table goes to the rest as untimed and is counted in
   zk_win_counts.unobserved_records. */
#define ZK_WIN_TRACE_TABLE (1u << 9)
/* the salt of the table's slot function */
#define ZK_WIN_TABLE_SALT 0xA0761D6478BD642Full

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
    uint64_t unobserved_records;                      /* ZK_WIN_TRACE_TABLE: timed records whose traceId the
                                                         table does not hold (else 0) */
    uint64_t reserved[4];
} zk_win_counts;
/* With ZK_WIN_TRACE_TABLE the *_records keep their meaning, the *_runs count runs (adjacent equal
   traceIds) by the class the table gives them, held_runs = held_records = 0 and held_from = n. */

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
 *   flags    ZK_BATCH_TRACE_CLUSTERED is required unless ZK_WIN_TRACE_TABLE is given (else
 *            ZK_ERR_UNSUPPORTED: without the table any-order input is not taken).
 *            ZK_BATCH_DEVICE_PTRS: `in` holds device pointers; without it `in` is host memory,
 *            staged, and the call waits for the staging copy. ZK_WIN_HOLD_LAST, ZK_WIN_TRACE_TABLE:
 *            see above.
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
   resolve, the histogram, the scan, the scatter, the final gather. With ZK_WIN_TRACE_TABLE slot 0 is the
   table lookup and slot 1 is 0. Needs zk_win_config.timing (without it no event is recorded);
   ZK_ERR_INVALID_ARG without it or before the first partition. */
zk_status   zk_win_phase_ms(zk_win* win, double out[6]);

/* ---- the trace-time table. Every call refuses a NULL handle or argument with ZK_ERR_INVALID_ARG
   before any device is touched; errors go to zk_win_last_error. ---- */
/* Fold a batch into the table. Only trace_id, first_ts and flags of `in` are read. flags:
   ZK_BATCH_DEVICE_PTRS as in zk_win_partition (a host batch is staged, 20 B per record, and the call
   waits for its staging copy); ZK_BATCH_TRACE_CLUSTERED is accepted and changes nothing (runs are
   found either way: one table update per run and row of 64 records). The call synchronises once, to
   read the run count it sizes the table by (see SIZING; growing synchronises once more). The inserts are
   queued on the handle's stream behind that: DEVICE columns must stay as they are until the handle's
   next synchronising call (zk_win_table_info, zk_win_table_lookup, zk_win_partition, zk_win_observe).
   n == 0 is ZK_OK. */
zk_status   zk_win_observe(zk_win* win, const zk_span_cols* in, uint32_t flags);
/* Empty the table; the allocation (slots) is kept. */
zk_status   zk_win_table_reset(zk_win* win);
/* Grow the table to at least 2 * traces slots now. A hint: it never shrinks the table and the content
   is kept. */
zk_status   zk_win_table_reserve(zk_win* win, uint64_t traces);
/* slots (0 before the first allocation), traceIds in the table, bytes of HBM the table holds. Any of the
   three pointers may be NULL. Synchronises. */
zk_status   zk_win_table_info(zk_win* win, uint64_t* slots, uint64_t* traces, uint64_t* bytes);
/* The table's answer for n traceIds (host memory, or device with ZK_BATCH_DEVICE_PTRS): t and found are
   HOST arrays of n entries; found[i] = 1 and t[i] = the trace's time when trace_ids[i] is in the table,
   else found[i] = 0 and t[i] is unspecified. Synchronises. */
zk_status   zk_win_table_lookup(zk_win* win, const uint64_t* trace_ids, uint64_t n, uint32_t flags, int64_t* t,
                                uint8_t* found);
/* Device time in ms of the last zk_win_observe: the run count, the sizing step (the count's copy and,
   when the table grew, the rehash), the inserts. Needs zk_win_config.timing; waits for the inserts. */
zk_status   zk_win_observe_ms(zk_win* win, double out[3]);
/* The window rule above on the host (no HIP): *w = the window of trace time t, or num_windows when t is
   before or after. ZK_ERR_INVALID_ARG for window_us <= 0, num_windows 0 or > ZK_WIN_MAX_WINDOWS. */
zk_status   zk_win_index(int64_t t, int64_t origin_us, int64_t window_us, uint32_t num_windows, uint32_t* w);

#ifdef __cplusplus
}
#endif
#endif /* ZKWINDOW_H */
