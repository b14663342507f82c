/*
 * zkindex.h -- the trace-id index by service and span name: getTraceIdsByName, getSpanNames and
 * getAllServiceNames on the device.
 *
 * Every query of the reference's query service begins with index.getTraceIdsByName(serviceName,
 * spanName, endTs, limit): the newest `limit` trace ids of a service, optionally of one span name, at
 * or before endTs (QueryService.getTraceIdsByServiceName / getTraceIdsBySpanName and the no-slice case
 * of getTraceIds; SpanStore.scala:91-96, 172-191; CassieSpanStore.scala:188-212, 366-381: the rows of
 * ServiceNameIndex / ServiceSpanNameIndex are service[.span], their columns the last annotation's
 * timestamp, read with getRowSlice(key, Some(endTs), None, limit, Order.Reversed)). Every 48-B record
 * already carries service_id and, in bits 16..31 of flags, its span-name id; this handle keeps them in
 * HBM grouped by service and selects over one service's entries.
 *
 * Semantics
 *  - A fragment is INDEXED when all of these hold:
 *      flags & ZK_F_HAS_ANNOTATIONS               (the reference skips a span without a last annotation);
 *      flags & (ZK_F_SVC_CLIENT | ZK_F_SVC_SERVER) (else it has no service name, and the reference does
 *                                                  not index the empty service name);
 *      not (service_id == cfg.client_service and its cs or cr count, bits 8..11 of flags, is non-zero)
 *                                                  (shouldIndex, SpanStore.scala:67-68: a client-side span
 *                                                  of the service literally called "client").
 *    cfg.client_service is that service's dictionary id; ZK_IX_NO_CLIENT switches the rule off.
 *  - SERVICE RANGE: an indexed record with service_id >= num_services makes the whole observe call
 *    ZK_ERR_SERVICE_RANGE; nothing of the batch is added (the counting pass sees the record before
 *    anything is written). A record that is not indexed may carry any service_id.
 *  - An indexed fragment contributes ONE entry (service_id, name_id = flags >> 16, ts = last_ts, trace_id).
 *  - The index is a MULTISET of entries, like InMemorySpanStore's `spans ++= newSpans`: observing a
 *    batch again adds its entries again. Batches and records may come in any order.
 *  - A query (service, name, end_ts, limit) matches the entries with entry.service == service, with
 *    name == ZK_IX_ANY_NAME or entry.name_id == name, and with entry.ts <= end_ts as signed values,
 *    inclusive (Cassandra's slice start). It returns (trace_id, ts) pairs by ts descending
 *    (Order.Reversed), equal ts by traceId ascending as unsigned, equal pairs each as often as they
 *    were entered: the first `limit` of them, and `matched`, the number of matching entries.
 *  - Legal: traceIds 0 and 2^64 - 1, ts and end_ts at INT64_MIN / INT64_MAX, name id 65535.
 *
 * Departures from the reference
 *  - A record carries one service (Span.serviceName's choice), not Span.serviceNames: a fragment is
 *    indexed under that one service and shouldIndex sees only that one.
 *  - Name id 0 folds "", "Unknown" and an absent name together; the reference indexes "Unknown". Id 0
 *    is never a span name here: it matches ZK_IX_ANY_NAME only and zk_ix_span_names leaves it out.
 *  - Cassandra's column name is the timestamp alone, so two traces of one row with equal timestamps
 *    clobber each other there. Here both are kept, as in the in-memory and Anorm stores.
 *  - The in-memory store's take(limit) in insertion order is not reproduced: the order is Cassandra's.
 *
 * Layout
 *  - One zk_ix_observe makes one SEGMENT (none when no record of the batch is indexed): the batch's
 *    entries grouped by service in three columns, tkey[u64] = ts with the sign bit flipped (unsigned
 *    order = signed order), tid[u64], name[u16]: 18 B per entry (each column 256-B aligned). The host
 *    keeps each segment's offsets[num_services + 1]. The order inside a service's slice is not
 *    reproducible; every answer is a function of the multiset alone.
 *  - At most ZK_IX_MAX_SEGMENTS segments exist: an observe that would make one more first merges all
 *    segments into one (each service's slices concatenated in segment order into a freshly sized
 *    segment, then the old ones freed). zk_ix_compact does the same on request. A refused allocation
 *    is ZK_ERR_CAPACITY and leaves the index as it was.
 *  - At most 2^32 - 1 entries per handle: a batch that would exceed it is ZK_ERR_CAPACITY and changes
 *    nothing.
 *
 * The select
 *  - zk_ix_trace_ids reads only the asked service's slices (at most ZK_IX_MAX_SEGMENTS of them, planned
 *    on the host from the kept offsets), AT MOST THREE TIMES: the filter with the count and the bits in
 *    which the matching keys differ; a 4096-bin histogram of the 12 highest differing bits; the append
 *    of the entries below the bin where the count crosses `limit` and of the entries in it. Further
 *    rounds run over the shrinking list of that bin's 16-B entries only; at most ZK_IX_MAX_LIMIT entries
 *    reach the host, which sorts them and emits `limit`. It is the exact radix select of zkduration.h
 *    over the 128-bit key (~tkey, traceId), with one case more: entries may be EQUAL in all 128 bits.
 *    When the candidates differ in no bit they are all the same pair, and the call takes as many of
 *    them as are still wanted and stops.
 *
 * Expiry (the reference's indexTtl: every index column Cassandra writes expires, CassieSpanStore.scala:48)
 *  - zk_ix_expire(min_ts) removes every entry with ts < min_ts as signed values; an entry with
 *    ts == min_ts stays. EXPIRY IS BY THE ENTRY'S OWN TIMESTAMP, NOT BY THE WALL-CLOCK TIME IT WAS
 *    WRITTEN: a stated departure from Cassandra's column TTL, which counts from the write. Every answer
 *    so stays a function of the observed multiset and the cutoffs applied, and every query stays exactly
 *    testable; for spans indexed near the time they end the two rules agree.
 *  - After the call the handle is indistinguishable, through zk_ix_trace_ids (with matched),
 *    zk_ix_span_names, zk_ix_service_counts and the entry count of zk_ix_info, from a fresh handle that
 *    observed only the survivors. NAMES DISAPPEAR WITH THEIR ENTRIES: a span name whose entries all
 *    expired is no longer a span name of its service, a service whose entries all expired has count 0
 *    (Cassandra's behaviour too). Equal entries all have one ts: all copies go or all stay.
 *  - It is a one-time cut, not a filter on future input: a later observe of older data enters it again.
 *  - INT64_MIN removes nothing; INT64_MAX keeps only the entries at exactly INT64_MAX.
 *  - Segments: a segment none of whose entries goes is kept UNTOUCHED (not read again, not copied); a
 *    segment all of whose entries go is freed; the others are MIXED, and the survivors of all mixed
 *    segments are written, grouped by service, into ONE new segment sized for them, after which the
 *    mixed segments are freed. The segment count never grows. With nothing to remove nothing is
 *    rewritten or reallocated: the same segments, the same bytes.
 *  - A refused allocation is ZK_ERR_CAPACITY and leaves the handle exactly as it was: nothing is freed
 *    before its replacement is complete.
 *  - CONSISTENCY with zkduration.h and zkannindex.h: with one cutoff c applied to the three handles fed
 *    from the same spans, every (trace_id, ts) this index still returns has its trace in the duration
 *    index: an indexed fragment is timed, its ts = last_ts <= the trace's end, so ts >= c implies
 *    end >= c, and zk_td_expire goes by end. Sorting trace ids by duration so never loses an id a
 *    trace-id query returned.
 *
 * Conventions are those of zkduration.h: every entry point returns zk_status; a handle is not
 * thread-safe; all device work of a handle is ordered on one HIP stream; nothing is allocated before
 * the first observe. Every call refuses a NULL handle or argument with ZK_ERR_INVALID_ARG before any
 * device is touched; errors go to zk_ix_last_error.
 */
#ifndef ZKINDEX_H
#define ZKINDEX_H

#include "zkagg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* zk_ix_config.client_service: no service is called "client" (the shouldIndex rule is off) */
#define ZK_IX_NO_CLIENT 0xFFFFFFFFu
/* zk_ix_trace_ids' name: every entry of the service, whatever its name id (0 included) */
#define ZK_IX_ANY_NAME 0xFFFFFFFFu
/* the largest limit of zk_ix_trace_ids */
#define ZK_IX_MAX_LIMIT 4096u
/* the most segments a handle holds */
#define ZK_IX_MAX_SEGMENTS 64u
/* the most services (the counting pass keeps one LDS bin per service) */
#define ZK_IX_MAX_SERVICES 4096u

typedef struct zk_ix_config {
    int32_t  device;          /* HIP device ordinal */
    uint32_t num_services;    /* S, 1..ZK_IX_MAX_SERVICES: service ids are 0..S-1 */
    uint32_t client_service;  /* the id of the service called "client", or ZK_IX_NO_CLIENT */
    uint32_t timing;          /* 1: record HIP events (zk_ix_observe_ms, zk_ix_query_ms) */
    void*    stream;          /* hipStream_t to run on, or NULL for a private stream */
    uint32_t reserved[8];
} zk_ix_config;

typedef struct zk_ix zk_ix;

/* num_services outside 1..ZK_IX_MAX_SERVICES is ZK_ERR_INVALID_ARG (before any device is touched). */
zk_status   zk_ix_create(const zk_ix_config* cfg, zk_ix** out);
zk_status   zk_ix_destroy(zk_ix* ix);
const char* zk_ix_last_error(const zk_ix* ix);

/* Add a batch's entries as one segment. Only trace_id, last_ts, service_id and flags of `in` are read.
   flags: ZK_BATCH_DEVICE_PTRS: `in` holds device pointers; without it `in` is host memory, staged (24 B
   per record), and the call waits for its staging copy. ZK_BATCH_TRACE_CLUSTERED is accepted and
   changes nothing. The call synchronises once, to read the per-service counts it sizes the segment by
   (a merge, see Layout, synchronises once more). The scatter is queued on the handle's stream behind
   that: DEVICE columns must stay as they are until the handle's next synchronising call (zk_ix_info,
   zk_ix_trace_ids, zk_ix_span_names, zk_ix_compact, zk_ix_expire, zk_ix_observe). n == 0 is ZK_OK;
   n >= 2^32 is ZK_ERR_UNSUPPORTED. */
zk_status   zk_ix_observe(zk_ix* ix, const zk_span_cols* in, uint32_t flags);
/* Empty the index: every segment is freed. */
zk_status   zk_ix_reset(zk_ix* ix);
/* Merge all segments into one (see Layout). Fewer than two segments: nothing to do. Synchronises. */
zk_status   zk_ix_compact(zk_ix* ix);
/* Remove every entry with ts < min_ts (see Expiry). *removed = the entries removed; may be NULL. Two
   passes: a count over every segment's tkey column (8 B per entry), one synchronisation to read the
   survivors per (segment, service), then the rewrite of the mixed segments' survivors (tkey again, and
   18 B read and 18 B written per survivor). Scratch for the plan (4 B per segment and service, twice) is
   allocated on first use and grown. An empty handle is ZK_OK with *removed = 0. Synchronises. */
zk_status   zk_ix_expire(zk_ix* ix, int64_t min_ts, uint64_t* removed);
/* entries in the index, segments, bytes of HBM the segments hold. Any of the three pointers may be
   NULL. Synchronises. */
zk_status   zk_ix_info(zk_ix* ix, uint64_t* entries, uint64_t* segments, uint64_t* bytes);
/* counts: a HOST array of num_services entries: the entries of each service. Host bookkeeping: no
   kernel runs and nothing is waited for. */
zk_status   zk_ix_service_counts(zk_ix* ix, uint64_t* counts);
/* The first `limit` (trace_id, ts) pairs of `service`, of span-name id `name` or ZK_IX_ANY_NAME, with
 * ts <= end_ts (see Semantics).
 *   service    >= num_services is ZK_ERR_INVALID_ARG.
 *   name       1..65535 or ZK_IX_ANY_NAME; 0 ("no name", never in the reference's span-name index) and
 *              anything above 65535 are ZK_ERR_INVALID_ARG.
 *   limit      1..ZK_IX_MAX_LIMIT, else ZK_ERR_INVALID_ARG.
 *   trace_id, ts   HOST arrays of `limit` entries; the first *n_out are written. A refused call writes
 *              nothing.
 *   n_out      min(limit, matched).
 *   matched    the number of matching entries; may be NULL.
 * An empty index or an empty service is ZK_OK with *n_out = 0. Scratch (91 KB, and 16 B for every entry
 * of the bin the select has to split) is allocated on first use and grown; a refused allocation is
 * ZK_ERR_CAPACITY. Synchronises. */
zk_status   zk_ix_trace_ids(zk_ix* ix, uint32_t service, uint32_t name, int64_t end_ts, uint32_t limit,
                            uint64_t* trace_id, int64_t* ts, uint32_t* n_out, uint64_t* matched);
/* The distinct non-zero name ids of the service's entries, ascending, into name_ids (a HOST array of
   `cap` entries; may be NULL when cap == 0). *n_out = their number; cap too small is ZK_ERR_CAPACITY
   with *n_out set to the needed count and nothing written. One pass over the service's name slices
   (2 B per entry). Synchronises. */
zk_status   zk_ix_span_names(zk_ix* ix, uint32_t service, uint16_t* name_ids, uint32_t cap, uint32_t* n_out);
/* Device time in ms of the last zk_ix_observe that added a segment: the count, the sizing step (the
   counts' copy and, when the segment bound was met, the merge), the scatter. Needs zk_ix_config.timing;
   waits for the scatter. */
zk_status   zk_ix_observe_ms(zk_ix* ix, double out[3]);
/* Device time in ms of the last zk_ix_expire that ran its count: the count, the sizing step (the
   counts' copy and the synchronisation), the rewrite (0 when no segment was mixed). Needs
   zk_ix_config.timing. */
zk_status   zk_ix_expire_ms(zk_ix* ix, double out[3]);
/* Time in ms on the handle's stream of the last zk_ix_trace_ids that ran a pass, from its first pass
   to its last copy (the host's bin choices between the passes included). Needs zk_ix_config.timing. */
zk_status   zk_ix_query_ms(zk_ix* ix, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* ZKINDEX_H */
