/*
 * zkannindex.h -- the trace-id index by annotation: getTraceIdsByAnnotation on the device.
 *
 * The third trace-id query of the reference's Index trait (after getTracesDuration, zkduration.h, and
 * getTraceIdsByName, zkindex.h): index.getTraceIdsByAnnotation(serviceName, annotation, value, endTs,
 * limit), the newest `limit` trace ids of a service that carry a time annotation of that value or a
 * binary annotation of that key (and, when a value is given, of that value), at or before endTs
 * (QueryService.getTraceIdsByAnnotation, both AnnotationSliceQuery forms of QueryService.getTraceIds;
 * SpanStore.scala:193-219; CassieSpanStore.scala:214-244, 383-393: the rows of AnnotationsIndex are
 * service:annotation[:value], their columns a timestamp, read in reversed order).
 *
 * Semantics
 *  - An ENTRY is (service u32, key u64, val u64, ts i64, trace_id u64):
 *      a time annotation:    key = zk_hash_string(value),  val = 0,  ts = the annotation's own timestamp;
 *      a binary annotation:  key = zk_hash_string(key),    val = zk_index_value_hash(value) (never 0),
 *                            ts = the span's last annotation timestamp.
 *    The reference writes two rows per binary annotation, (service, key, Some(value)) and
 *    (service, key, None); here it is ONE entry and the query rule reproduces the second row. Which
 *    annotations of which spans give entries is the item source's business (zkingest.h,
 *    zk_ingest_spans_indexed): zk_ax_observe enters every entry it is given.
 *  - SERVICE RANGE: an entry with service >= num_services makes the whole observe call
 *    ZK_ERR_SERVICE_RANGE; nothing of the batch is added.
 *  - The index is a MULTISET of entries: observing a batch again adds its entries again. Batches and
 *    entries may come in any order.
 *  - A query (service, key, val, end_ts, limit) matches the entries with entry.service == service,
 *    entry.key == key, val == ZK_AX_ANY_VALUE or entry.val == val, and entry.ts <= end_ts as signed
 *    values, inclusive. With ZK_AX_ANY_VALUE it so finds time annotations by value and binary
 *    annotations by key: both live in one row space, as in the reference. It returns (trace_id, ts)
 *    pairs in zkindex.h's order: ts descending, equal ts by traceId ascending as unsigned, equal pairs
 *    each as often as they were entered: the first `limit` of them, and `matched`, the number of
 *    matching entries.
 *  - Legal: key 0 and 2^64 - 1, traceIds 0 and 2^64 - 1, ts and end_ts at INT64_MIN / INT64_MAX. An even
 *    non-zero val can match nothing (a stored val is 0 or odd); it is accepted and returns no rows.
 *
 * Departures from the reference
 *  - HASH EQUALITY: equality of the 64-bit hashes stands for equality of the strings (for values: of
 *    63 bits). Two different strings with one hash share a row.
 *  - ts <= end_ts is the in-memory store's filter (SpanStore.scala:206, 212) and the one the store
 *    validator's vectors need. Cassandra's call passes endTs as the slice's END in reversed order
 *    (CassieSpanStore.scala:392), which read literally is the other side; that is not reproduced.
 *  - Cassandra's column name is the timestamp alone, so equal timestamps in one row clobber each other
 *    there. Here the index is a multiset, as in zkindex.h. In particular a span with two binary
 *    annotations of one key gives two entries that both match val = ZK_AX_ANY_VALUE.
 *  - The in-memory store's take(limit) in insertion order is not reproduced: the order is Cassandra's.
 *  - The rule that a core annotation (cs, cr, sr, ss) is never found (SpanStore.scala:201) is the
 *    caller's: the item source emits no time entry for them, but a binary annotation whose KEY is "cs"
 *    has an entry, and this handle returns it when asked.
 *
 * Layout
 *  - One zk_ax_observe makes one SEGMENT: the batch's entries grouped by service in four columns,
 *    tkey[u64] = ts with the sign bit flipped, tid[u64], key[u64], val[u64]: 32 B per entry (each column
 *    256-B aligned). The host keeps each segment's offsets[num_services + 1]. The order inside a
 *    service's slice is not reproducible; every answer is a function of the multiset alone.
 *  - At most ZK_AX_MAX_SEGMENTS segments exist: an observe that would make one more first merges all
 *    segments into one; zk_ax_compact does the same on request. A refused allocation is
 *    ZK_ERR_CAPACITY and leaves the index as it was.
 *  - At most 2^32 - 1 entries per handle: a batch that would exceed it is ZK_ERR_CAPACITY and changes
 *    nothing.
 *
 * The select is zkindex.h's: at most three reads of the asked service's slices, then rounds over the
 * shrinking list of 16-B candidates. A read of the slices looks at key (8 B) for every entry, at val
 * (8 B) only where the key matched and a value was asked, and at tkey / tid (16 B) only where both
 * matched.
 *
 * Expiry is zkindex.h's, on the entry's ts: zk_ax_expire(min_ts) removes every entry with ts < min_ts
 * as signed values (an entry with ts == min_ts stays), by the entry's own timestamp, not by the
 * wall-clock time it was written (the stated departure from Cassandra's column TTL). For a time
 * annotation ts is the annotation's own timestamp, for a binary annotation the span's last annotation
 * timestamp. After the call the handle is indistinguishable, through zk_ax_trace_ids (with matched),
 * zk_ax_service_counts and the entry count of zk_ax_info, from a fresh handle that observed only the
 * survivors; a service whose entries all expired has count 0. Equal entries go or stay together. A later
 * observe of older data enters it again. INT64_MIN removes nothing, INT64_MAX keeps only the entries at
 * exactly INT64_MAX. The segment rule is zkindex.h's: untouched segments are kept as they are, fully
 * expired ones are freed, the survivors of all mixed ones go into one new segment; the segment count
 * never grows; with nothing to remove nothing is rewritten or reallocated. A refused allocation is
 * ZK_ERR_CAPACITY and leaves the handle exactly as it was. The consistency invariant of zkindex.h holds
 * here too: an entry's ts is at most its span's last annotation timestamp, which is at most its trace's
 * end, so with one cutoff on this handle and on the duration index every (trace_id, ts) still returned
 * has its trace in the duration index.
 *
 * Conventions are those of zkindex.h: every entry point returns zk_status; a handle is not thread-safe;
 * all device work of a handle is ordered on one HIP stream; nothing is allocated before the first
 * observe. Every call refuses a NULL handle or argument with ZK_ERR_INVALID_ARG before any device is
 * touched; errors go to zk_ax_last_error.
 */
#ifndef ZKANNINDEX_H
#define ZKANNINDEX_H

#include "zkagg.h"
#include "zkingest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* zk_ax_trace_ids' val: every entry of the key, time or binary, whatever its value */
#define ZK_AX_ANY_VALUE 0ull
/* the largest limit of zk_ax_trace_ids */
#define ZK_AX_MAX_LIMIT 4096u
/* the most segments a handle holds */
#define ZK_AX_MAX_SEGMENTS 64u
/* the most services (the counting pass keeps one LDS bin per service) */
#define ZK_AX_MAX_SERVICES 4096u

typedef struct zk_ax_config {
    int32_t  device;          /* HIP device ordinal */
    uint32_t num_services;    /* S, 1..ZK_AX_MAX_SERVICES: service ids are 0..S-1 */
    uint32_t timing;          /* 1: record HIP events (zk_ax_observe_ms, zk_ax_query_ms) */
    void*    stream;          /* hipStream_t to run on, or NULL for a private stream */
    uint32_t reserved[8];
} zk_ax_config;

typedef struct zk_ax zk_ax;

/* num_services outside 1..ZK_AX_MAX_SERVICES is ZK_ERR_INVALID_ARG (before any device is touched). */
zk_status   zk_ax_create(const zk_ax_config* cfg, zk_ax** out);
zk_status   zk_ax_destroy(zk_ax* ax);
const char* zk_ax_last_error(const zk_ax* ax);

/* Add the items->n entries as one segment (cap is not read). flags: ZK_BATCH_DEVICE_PTRS: the five
   arrays are device pointers; without it they are host memory, staged (36 B per entry), and the call
   waits for its staging copy. The call synchronises once, to read the per-service counts it sizes the
   segment by (a merge, see Layout, synchronises once more). The scatter is queued on the handle's
   stream behind that: DEVICE columns must stay as they are until the handle's next synchronising call
   (zk_ax_info, zk_ax_trace_ids, zk_ax_compact, zk_ax_expire, zk_ax_observe). n == 0 is ZK_OK;
   n >= 2^32 is ZK_ERR_UNSUPPORTED. */
zk_status   zk_ax_observe(zk_ax* ax, const zk_ingest_index_items* items, uint32_t flags);
/* Empty the index: every segment is freed. */
zk_status   zk_ax_reset(zk_ax* ax);
/* Merge all segments into one (see Layout). Fewer than two segments: nothing to do. Synchronises. */
zk_status   zk_ax_compact(zk_ax* ax);
/* Remove every entry with ts < min_ts (see Expiry). *removed = the entries removed; may be NULL. Two
   passes: a count over every segment's tkey column (8 B per entry), one synchronisation to read the
   survivors per (segment, service), then the rewrite of the mixed segments' survivors (tkey again, and
   32 B read and 32 B written per survivor). An empty handle is ZK_OK with *removed = 0. Synchronises. */
zk_status   zk_ax_expire(zk_ax* ax, int64_t min_ts, uint64_t* removed);
/* entries in the index, segments, bytes of HBM the segments hold. Any of the three pointers may be
   NULL. Synchronises. */
zk_status   zk_ax_info(zk_ax* ax, uint64_t* entries, uint64_t* segments, uint64_t* bytes);
/* counts: a HOST array of num_services entries: the entries of each service. Host bookkeeping: no
   kernel runs and nothing is waited for. */
zk_status   zk_ax_service_counts(zk_ax* ax, uint64_t* counts);
/* The first `limit` (trace_id, ts) pairs of `service` and `key`, of value hash `val` or
 * ZK_AX_ANY_VALUE, with ts <= end_ts (see Semantics).
 *   service    >= num_services is ZK_ERR_INVALID_ARG.
 *   limit      1..ZK_AX_MAX_LIMIT, else ZK_ERR_INVALID_ARG.
 *   trace_id, ts   HOST arrays of `limit` entries; the first *n_out are written. A refused call writes
 *              nothing.
 *   n_out      min(limit, matched).
 *   matched    the number of matching entries; may be NULL.
 * An empty index or an empty service is ZK_OK with *n_out = 0. Scratch (83 KB, and 16 B for every entry
 * of the bin the select has to split) is allocated on first use and grown; a refused allocation is
 * ZK_ERR_CAPACITY. Synchronises. */
zk_status   zk_ax_trace_ids(zk_ax* ax, uint32_t service, uint64_t key, uint64_t val, int64_t end_ts, uint32_t limit,
                            uint64_t* trace_id, int64_t* ts, uint32_t* n_out, uint64_t* matched);
/* Device time in ms of the last zk_ax_observe that added a segment: the count, the sizing step (the
   counts' copy and, when the segment bound was met, the merge), the scatter. Needs zk_ax_config.timing;
   waits for the scatter. */
zk_status   zk_ax_observe_ms(zk_ax* ax, double out[3]);
/* Device time in ms of the last zk_ax_expire that ran its count: the count, the sizing step (the
   counts' copy and the synchronisation), the rewrite (0 when no segment was mixed). Needs
   zk_ax_config.timing. */
zk_status   zk_ax_expire_ms(zk_ax* ax, double out[3]);
/* Time in ms on the handle's stream of the last zk_ax_trace_ids that ran a pass, from its first pass
   to its last copy (the host's bin choices between the passes included). Needs zk_ax_config.timing. */
zk_status   zk_ax_query_ms(zk_ax* ax, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* ZKANNINDEX_H */
