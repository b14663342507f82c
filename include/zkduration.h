/*
 * zkduration.h -- the trace duration index: getTracesDuration and the k slowest, fastest, newest or
 * oldest traces of a time range, on the device.
 *
 * The reference's stores answer getTracesDuration(traceIds): Seq[TraceIdDuration(traceId, duration,
 * startTimestamp)] and its query service sorts trace ids by it (Order.DURATION_DESC/ASC,
 * TIMESTAMP_DESC/ASC). Every 48-B record already carries trace_id, first_ts, last_ts and
 * ZK_F_HAS_ANNOTATIONS; this handle folds them into one table in HBM, traceId -> (start, end), and
 * selects over that table.
 *
 * Semantics (InMemorySpanStore.getTracesDuration)
 *  - A fragment is TIMED when flags & ZK_F_HAS_ANNOTATIONS. The first_ts and last_ts of any other
 *    fragment are ignored (the reference's firstAnnotation / lastAnnotation are None).
 *  - A trace's entry holds start = the minimum first_ts and end = the maximum last_ts over all its timed
 *    fragments, over every batch observed since the last zk_td_reset, and
 *        duration = (int64)((uint64)end - (uint64)start)
 *    which is the reference's wrapping Long subtraction: a trace from INT64_MIN to INT64_MAX has
 *    duration -1, and the orders below use that signed value.
 *  - MEMBERSHIP: a traceId is in the index exactly when some observed fragment of it was timed.
 *    TraceIds 0 and 2^64 - 1 are legal. An id that is not in the index has no entry.
 *  - The fold is a minimum and a maximum: observing a batch again changes no word of the table;
 *    batches and records may come in any order; a trace may be spread over any number of batches.
 *
 * The table
 *  - Open addressing with linear probing in HBM, 24 B per slot {uint64 key, uint64 start, uint64 end};
 *    key = traceId, 0 = empty; start = the start time with the sign bit flipped (unsigned order = signed
 *    order), end likewise. A fresh slot holds start = all ones and end = 0.
 *  - `slots` is a power of two and the home slot of a traceId is
 *        zk_mix64(trace_id ^ ZK_TD_TABLE_SALT) & (slots - 1)
 *    (zk_mix64: the splitmix64 finalizer, z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) *
 *    0x94D049BB133111EB, z ^ z >> 31); a probe walks upwards and wraps to slot 0. TraceId 0 lives in one
 *    extra slot at index `slots`, whose key word is a presence flag.
 *  - SIZING (the rule of zkwindow.h): before anything of a batch is inserted the call counts the batch's
 *    trace runs (maximal stretches of adjacent records with equal trace_id) and makes sure that
 *    slots >= 2 * (traces in the table + runs in the batch), rounded up to a power of two, at least
 *    1024. The load so never exceeds 1/2. An observe or a reserve only grows the table (the old content
 *    is rehashed into the new table); a refused allocation is ZK_ERR_CAPACITY and changes nothing.
 *    zk_td_expire is the ONE operation that may shrink it (see Expiry).
 *  - bytes = (slots + 1) * 24.
 *
 * Expiry (the reference's indexTtl: every index column Cassandra writes expires, CassieSpanStore.scala:48)
 *  - zk_td_expire(min_end) removes every trace whose end < min_end as signed values; a trace with
 *    end == min_end stays. `end` is used, not `start`, so that a trace still receiving fragments stays.
 *    TraceId 0, which lives in the extra slot, follows the same rule. EXPIRY IS BY THE TRACE'S OWN END
 *    TIME, NOT BY THE WALL-CLOCK TIME IT WAS WRITTEN: a stated departure from Cassandra's column TTL,
 *    which counts from the write. Every answer so stays a function of the observed fragments and the
 *    cutoffs applied, and stays exactly testable; for spans indexed near the time they end the two rules
 *    agree.
 *  - After the call the handle is indistinguishable, through zk_td_lookup, zk_td_top and the trace count
 *    of zk_td_info, from a fresh handle whose table holds only the survivors, each with the start and
 *    end it had. It is a one-time cut, not a filter on future input: a later observe of fragments of a
 *    removed trace enters the trace again, with the times of those fragments alone.
 *  - INT64_MIN removes nothing; INT64_MAX keeps only the traces whose end is exactly INT64_MAX.
 *  - WHY A REBUILD: open addressing with linear probing has no delete in place. Emptying a slot cuts the
 *    probe chain of every key that was displaced past it, and a lookup of such a key would end at the
 *    hole. So the call counts the survivors (one pass over the table) and, ONLY WHEN SOMETHING EXPIRES,
 *    inserts them into a fresh table sized by the SIZING rule applied to the survivors: slots = the
 *    power of two at or above 2 * survivors, at least 1024. The old table is freed after the rebuild is
 *    complete. The table may so shrink, and a zk_td_reserve hint does not survive the call. With
 *    nothing to remove the table stays where and as it is: the same slots, the same bytes.
 *  - A refused allocation is ZK_ERR_CAPACITY and leaves the handle exactly as it was.
 *  - CONSISTENCY with zkindex.h and zkannindex.h: an indexed fragment is timed, and its entry's
 *    ts <= last_ts <= the trace's end. With one cutoff c on the three handles, ts >= c implies
 *    end >= c: every (trace_id, ts) the two trace-id indices still return has its trace here.
 *
 * Top
 *  - zk_td_top takes the traces whose start lies in [start_lo, start_hi], both ends inclusive, and
 *    returns the first k of them in the chosen order:
 *        ZK_TD_DURATION_DESC   a.duration > b.duration      ZK_TD_DURATION_ASC   a.duration < b.duration
 *        ZK_TD_TIMESTAMP_DESC  a.start > b.start            ZK_TD_TIMESTAMP_ASC  a.start < b.start
 *    (the comparisons of QueryService.sortTraceIds). Equal keys are ordered by traceId ascending as
 *    unsigned, in all four orders, so the answer is a function of the table's content alone.
 *  - It is an exact radix select, not a sort: the order key (64 bits, smallest first) and the traceId
 *    form a 128-bit key; the table is read at most THREE times (the range filter with the count and
 *    the bits in which the matching keys differ; a 4096-bin histogram of the 12 highest differing
 *    bits; the append of the entries below the bin where the count crosses k and of the entries in
 *    it), further rounds run over the shrinking list of that bin's entries only, and at most
 *    ZK_TD_MAX_TOP entries reach the host, which sorts them and emits k.
 *
 * Conventions are those of zkagg.h: every entry point returns zk_status; a handle is not thread-safe;
 * all device work of a handle is ordered on one HIP stream. Every call refuses a NULL handle or argument
 * with ZK_ERR_INVALID_ARG before any device is touched; errors go to zk_td_last_error.
 */
#ifndef ZKDURATION_H
#define ZKDURATION_H

#include "zkagg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the salt of the table's slot function (not the one of zkwindow.h: the two tables hash apart) */
#define ZK_TD_TABLE_SALT 0xE7037ED1A0B428DBull
/* the largest k of zk_td_top */
#define ZK_TD_MAX_TOP 4096u
/* the orders of zk_td_top: the ordinals of the query service's Order enum */
#define ZK_TD_TIMESTAMP_DESC 0u
#define ZK_TD_TIMESTAMP_ASC  1u
#define ZK_TD_DURATION_ASC   2u
#define ZK_TD_DURATION_DESC  3u

typedef struct zk_td_config {
    int32_t  device;        /* HIP device ordinal */
    uint32_t timing;        /* 1: record HIP events (zk_td_observe_ms, zk_td_top_ms) */
    void*    stream;        /* hipStream_t to run on, or NULL for a private stream */
    uint32_t reserved[8];
} zk_td_config;

typedef struct zk_td zk_td;

/* Nothing is allocated until the first observe, reserve or top. */
zk_status   zk_td_create(const zk_td_config* cfg, zk_td** out);
zk_status   zk_td_destroy(zk_td* td);
const char* zk_td_last_error(const zk_td* td);

/* Fold a batch into the table. Only trace_id, first_ts, last_ts and flags of `in` are read (28 B per
   record). flags: ZK_BATCH_DEVICE_PTRS: `in` holds device pointers; without it `in` is host memory,
   staged (28 B per record), and the call waits for its staging copy. ZK_BATCH_TRACE_CLUSTERED is
   accepted and changes nothing (runs are found either way: one table update per run and row of 64
   records). The call synchronises once, to read the run count it sizes the table by (see SIZING;
   growing synchronises once more). The inserts are queued on the handle's stream behind that: DEVICE
   columns must stay as they are until the handle's next synchronising call (zk_td_info, zk_td_lookup,
   zk_td_top, zk_td_expire, zk_td_observe). n == 0 is ZK_OK. */
zk_status   zk_td_observe(zk_td* td, const zk_span_cols* in, uint32_t flags);
/* Empty the table; the allocation (slots) is kept. */
zk_status   zk_td_reset(zk_td* td);
/* Grow the table to at least 2 * traces slots now. A hint: it never shrinks the table and the content
   is kept. It does not survive a zk_td_expire that removes something. */
zk_status   zk_td_reserve(zk_td* td, uint64_t traces);
/* Remove every trace whose end < min_end (see Expiry). *removed = the traces removed; may be NULL. One
   pass over the table counts the survivors (16 B read per slot), one synchronisation reads the count,
   and when something expires a fresh table is cleared (24 B per slot) and filled from the old one (24 B
   read per slot, 24 B written per survivor). An empty handle is ZK_OK with *removed = 0. Synchronises. */
zk_status   zk_td_expire(zk_td* td, int64_t min_end, uint64_t* removed);
/* slots (0 before the first allocation), traceIds in the table, bytes of HBM the table holds. Any of the
   three pointers may be NULL. Synchronises. */
zk_status   zk_td_info(zk_td* td, uint64_t* slots, uint64_t* traces, uint64_t* bytes);
/* The table's answer for n traceIds (host memory, or device with ZK_BATCH_DEVICE_PTRS), in the order
   asked, duplicates as often as asked: start, duration and found are HOST arrays of n entries;
   found[i] = 1 with start[i] and duration[i] the trace's when trace_ids[i] is in the table, else
   found[i] = 0 and the two are unspecified. n == 0 is ZK_OK. Synchronises. */
zk_status   zk_td_lookup(zk_td* td, const uint64_t* trace_ids, uint64_t n, uint32_t flags, int64_t* start,
                         int64_t* duration, uint8_t* found);
/* The first k traces, in `order`, of those whose start lies in [start_lo, start_hi] (see Top).
 *   k          1..ZK_TD_MAX_TOP; anything else, an unknown order or start_lo > start_hi is
 *              ZK_ERR_INVALID_ARG and writes nothing.
 *   trace_id, start, duration   HOST arrays of k entries; the first *n_out are written.
 *   n_out      min(k, matched).
 *   matched    the number of traces in the range; may be NULL.
 * An empty table is ZK_OK with *n_out = 0. Scratch (112 KB, and 24 B for every entry of the bin the
 * select has to split) is allocated on first use and grown; a refused allocation is ZK_ERR_CAPACITY.
 * Synchronises. */
zk_status   zk_td_top(zk_td* td, uint32_t order, int64_t start_lo, int64_t start_hi, uint32_t k,
                      uint64_t* trace_id, int64_t* start, int64_t* duration, uint32_t* n_out, uint64_t* matched);
/* Device time in ms of the last zk_td_observe: the run count, the sizing step (the count's copy and,
   when the table grew, the rehash), the inserts. Needs zk_td_config.timing; waits for the inserts. */
zk_status   zk_td_observe_ms(zk_td* td, double out[3]);
/* Device time in ms of the last zk_td_expire that ran its count: the count, the sizing step (the
   count's copy and the synchronisation), the rebuild (0 when nothing expired). Needs
   zk_td_config.timing. */
zk_status   zk_td_expire_ms(zk_td* td, double out[3]);
/* Time in ms on the handle's stream of the last zk_td_top that ran a pass, from its first pass to its
   last copy (the host's bin choices between the passes included). Needs zk_td_config.timing. */
zk_status   zk_td_top_ms(zk_td* td, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* ZKDURATION_H */
