/*
 * zkspans.h -- the span store by trace id: tracesExist and getSpansByTraceIds on the device.
 *
 * Everything the reference's query service returns about a trace starts from
 * storage.getSpansByTraceIds(traceIds) (QueryService.scala:286-355: tracesExist, getTracesByIds,
 * getTraceSummariesByIds; SpanStore.scala:76-84), and a Trace is built from those spans (Trace.scala,
 * TraceSummary.scala). The trace-id indices (zkindex.h, zkannindex.h) and the duration index
 * (zkduration.h) hand out trace ids; this handle keeps the 48-B records themselves in HBM, findable by
 * trace id, and hands the fragments of the asked traces back, or their TraceSummary alone, merged on the
 * device (zk_sp_summaries).
 *
 * Semantics
 *  - EVERY observed fragment is kept, whole, until its trace expires (see Expiry): trace_id, span_id,
 *    parent_id, first_ts, last_ts, service_id, flags. No fragment is filtered (the reference's
 *    shouldIndex governs its indices, not its span data) and no service-range rule applies: the config
 *    has no num_services and service_id may be any 32-bit value.
 *  - The store is a MULTISET of fragments, like InMemorySpanStore's `spans ++= newSpans`: observing a
 *    batch again adds it again. Batches and records may come in any order; a trace may be spread over
 *    any number of batches.
 *  - Legal: traceIds 0 and 2^64 - 1, timestamps at INT64_MIN / INT64_MAX.
 *  - MEMBERSHIP: a traceId exists exactly when some observed fragment carries it, TIMED OR NOT
 *    (tracesExist's rule: a row of the trace is there). This is WIDER than zkduration.h's rule, which
 *    admits a trace only through a timed fragment: a trace of untimed fragments alone exists here, is
 *    absent there, and has no TraceSummary (TraceSummary.apply yields None).
 *  - CANONICAL ORDER: the fragments of one trace are returned ascending lexicographically by
 *    (span_id unsigned, parent_id unsigned, first_ts signed, last_ts signed, service_id, flags); equal
 *    fragments appear as often as they were entered. Every answer is so a function of the multiset alone.
 *
 * Departures from the reference
 *  - A record carries no endpoint (ip, port): a TraceSummary built from this store has no endpoints.
 *  - A record carries one service (Span.serviceName's choice), not Span.serviceNames.
 *  - Expiry is by the data's own time, not by the wall-clock time of the write (see Expiry): the
 *    reference's column TTL counts from the write. Every answer so stays a function of the observed
 *    multiset and the cutoffs applied. This is zkindex.h's stated departure.
 *  - A pin (the reference's setTimeToLive) covers the whole trace, fragments observed later included;
 *    Cassandra gives later columns spanTtl again and getTimeToLive answers the minimum.
 *
 * Expiry (zk_sp_expire; the reference writes every span column with spanTtl, 7 days, and lets one trace's
 * ttl be set and read: CassieSpanStore.scala:47,295,317-339)
 *  - A trace goes or stays WHOLE. end(trace) = the maximum last_ts over the trace's TIMED fragments in
 *    the whole store, over all segments (timed: flags & ZK_F_HAS_ANNOTATIONS, zkduration.h's rule). A
 *    trace survives exactly when end(trace) >= cutoff(trace); end == cutoff stays. The untimed fragments
 *    of a surviving trace stay with it.
 *  - The first_ts / last_ts of an untimed fragment are never read as times: an untimed fragment with
 *    last_ts = INT64_MAX keeps no trace alive.
 *  - A trace with no timed fragment has end = INT64_MIN: it goes at any cutoff above INT64_MIN. The
 *    duration index does not hold such a trace and it has no TraceSummary.
 *  - cutoff(trace) = min_end, unless the call carries a pin for the trace id: then the pin's own min_end,
 *    which may be lower or higher than the default.
 *  - min_end == INT64_MIN with no pins removes nothing and rewrites nothing (segments, bytes and
 *    allocations stay); INT64_MAX keeps only the traces whose end is INT64_MAX.
 *  - After a call the store is indistinguishable, through zk_sp_exist, zk_sp_gather and zk_sp_info's
 *    entries, from a fresh store that observed only the surviving fragments. The cut is made once: a
 *    later observe of older data enters the store again.
 *  - INVARIANT: a zk_td (zkduration.h) and this store fed the same batches and cut at the same value
 *    hold the same trace ids: the store's surviving traces with a timed fragment are exactly the ids the
 *    duration index still finds. With the span cutoff at or below the indices' cutoff (7 days against 3)
 *    every id an index returns has its whole trace here.
 *  - Legal as before: trace ids 0 and 2^64 - 1, times at the int64 bounds, a trace of any length spread
 *    over any number of segments.
 *
 * Layout
 *  - One zk_sp_observe makes one SEGMENT: the batch's records grouped by BUCKET,
 *        bucket = zk_mix64(trace_id ^ ZK_SP_SALT) >> 52          (ZK_SP_BUCKETS = 4096 buckets)
 *    (zk_mix64: the splitmix64 finalizer, z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) *
 *    0x94D049BB133111EB, z ^ z >> 31), in seven columns, 48 B per entry, each column 256-B aligned. The
 *    host keeps each segment's offsets[4097]; a copy of them (4 B each) lies behind the segment's columns
 *    for the lookups. The order inside a bucket's slice is not reproducible.
 *  - At most ZK_SP_MAX_SEGMENTS segments exist: an observe that would make one more first merges all
 *    segments into one (each bucket's slices concatenated in segment order into a freshly sized segment,
 *    then the old ones freed). zk_sp_compact does the same on request.
 *  - At most 2^32 - 1 entries per handle: a batch that would exceed it is ZK_ERR_CAPACITY and changes
 *    nothing.
 *  - A refused allocation is ZK_ERR_CAPACITY and leaves the handle exactly as it was: nothing is freed
 *    before its replacement is complete.
 *
 * Conventions are those of zkduration.h: every entry point returns zk_status; a handle is not
 * thread-safe; all device work of a handle is ordered on one HIP stream; nothing is allocated before the
 * first observe. Every call refuses a NULL handle or argument with ZK_ERR_INVALID_ARG before any device
 * is touched; errors go to zk_sp_last_error.
 */
#ifndef ZKSPANS_H
#define ZKSPANS_H

#include "zkagg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the salt of the bucket function (not the ones of zkwindow.h and zkduration.h: the three hash apart) */
#define ZK_SP_SALT 0x8CB92BA72F3D8DD7ull
/* buckets of a segment: the 12 highest bits of the salted hash */
#define ZK_SP_BUCKETS 4096u
/* the most segments a handle holds */
#define ZK_SP_MAX_SEGMENTS 64u
/* the most ids one zk_sp_exist or zk_sp_gather asks */
#define ZK_SP_MAX_IDS 4096u
/* the most pins one zk_sp_expire carries */
#define ZK_SP_MAX_PINS 4096u
/* the salt of the expiry's scratch table, home slot = zk_mix64(trace_id ^ ZK_SP_END_SALT) & (slots - 1)
   (apart from ZK_SP_SALT: a range of buckets shares the bucket hash's high bits) */
#define ZK_SP_END_SALT 0x3C79AC492BA7B653ull

/* the longest trace (in rows) whose spans zk_sp_summaries merges on the device; a power of two */
#define ZK_SP_SUM_MAX_ROWS 2048u
/* zk_sp_summaries' plan: a trace of up to this many rows is summarized by one wave, a longer one by a workgroup */
#define ZK_SP_SUM_WAVE_ROWS 64u
/* zk_sp_summary.state */
#define ZK_SP_SUM_FOUND    1u  /* some fragment carries the id */
#define ZK_SP_SUM_TIMED    2u  /* some fragment of the trace is timed; clear: start = end = 0, the trace for
                                  which TraceSummary.apply yields None */
#define ZK_SP_SUM_OVERFLOW 4u  /* more than ZK_SP_SUM_MAX_ROWS rows: spans = span_ts = 0 and no entries */

/* the longest trace (in rows) that zk_sp_traces merges on the device: zk_sp_summaries' bound, so that both
   device paths overflow at the same length */
#define ZK_SP_TRACE_MAX_ROWS 2048u
/* zk_sp_trace.state: the ZK_SP_SUM_* bits, value for value */
#define ZK_SP_TR_FOUND    1u
#define ZK_SP_TR_TIMED    2u
#define ZK_SP_TR_OVERFLOW 4u  /* more than ZK_SP_TRACE_MAX_ROWS rows: spans = services = 0, nothing emitted */
/* zk_sp_span.bits */
#define ZK_SP_SPAN_HAS_PARENT   1u  /* some fragment of the span carries ZK_F_HAS_PARENT */
#define ZK_SP_SPAN_TIMED        2u  /* some fragment of the span is timed */
#define ZK_SP_SPAN_PARENT_FOUND 4u  /* the parent id is a span of this trace */
#define ZK_SP_SPAN_ROOT_MOST    8u  /* the trace's root-most span */

typedef struct zk_sp_config {
    int32_t  device;   /* HIP device ordinal */
    uint32_t timing;   /* 1: record HIP events (zk_sp_observe_ms, zk_sp_query_ms, zk_sp_expire_ms) */
    void*    stream;   /* hipStream_t to run on, or NULL for a private stream */
    uint32_t expire_chunk; /* zk_sp_expire: entries per range of buckets at most; 0: the default, 2^24 */
    uint32_t reserved[7];
} zk_sp_config;

/* zk_sp_gather's output: seven HOST columns of `cap` entries each */
typedef struct zk_sp_rows {
    uint64_t* trace_id;
    uint64_t* span_id;
    uint64_t* parent_id;
    int64_t*  first_ts;
    int64_t*  last_ts;
    uint32_t* service_id;
    uint32_t* flags;
} zk_sp_rows;

/* zk_sp_summaries' head of one asked id, 40 bytes */
typedef struct zk_sp_summary {
    uint64_t trace_id;   /* the asked id; 0 when it is not found (the whole head is zeros then) */
    int64_t  start;      /* the minimum first_ts over the trace's timed fragments */
    int64_t  end;        /* the maximum last_ts over them */
    uint32_t fragments;  /* the trace's rows */
    uint32_t spans;      /* its merged spans, timed or not */
    uint32_t span_ts;    /* its entries in zk_sp_span_ts */
    uint32_t state;      /* ZK_SP_SUM_* */
} zk_sp_summary;

/* zk_sp_summaries' entries: three HOST columns of `cap` entries each */
typedef struct zk_sp_span_ts {
    uint32_t* service_id;
    int64_t*  first;
    int64_t*  last;
} zk_sp_span_ts;

/* zk_sp_traces' head of one asked id, 48 bytes */
typedef struct zk_sp_trace {
    uint64_t trace_id;   /* the asked id; 0 when it is not found (the whole head is zeros then) */
    int64_t  start;      /* as in zk_sp_summary */
    int64_t  end;
    uint64_t root_most;  /* the span id of getRootMostSpan; 0 when spans == 0 */
    uint32_t fragments;  /* the trace's rows */
    uint32_t spans;      /* its merged spans: its entries in the span column */
    uint32_t services;   /* its (span, service) pairs: its entries in the services column */
    uint32_t state;      /* ZK_SP_TR_* */
} zk_sp_trace;

/* one merged span of zk_sp_traces, 48 bytes */
typedef struct zk_sp_span {
    uint64_t span_id;
    uint64_t parent_id;  /* 0 without ZK_SP_SPAN_HAS_PARENT (0 and 2^64 - 1 are legal parents: the bit decides) */
    int64_t  first;      /* 0 when untimed */
    int64_t  last;
    uint32_t name;       /* the 16-bit span-name id, 0 for none */
    uint32_t depth;      /* 1 for the root-most span; 0: the span is not under it */
    uint32_t services;   /* its entries in the services column */
    uint32_t bits;       /* ZK_SP_SPAN_* */
} zk_sp_span;

typedef struct zk_sp zk_sp;

zk_status   zk_sp_create(const zk_sp_config* cfg, zk_sp** out);
zk_status   zk_sp_destroy(zk_sp* sp);
const char* zk_sp_last_error(const zk_sp* sp);

/* Add a batch's records as one segment. All seven columns of `in` are read. flags:
   ZK_BATCH_DEVICE_PTRS: `in` holds device pointers; without it `in` is host memory, staged (48 B per
   record), and the call waits for its staging copy. ZK_BATCH_TRACE_CLUSTERED is accepted and changes
   nothing. A count kernel over trace_id (8 B per record) builds the 4096-bin histogram; the call
   synchronises once, to read the counts it sizes the segment by (a merge, see Layout, synchronises once
   more). The scatter of the seven columns (48 B read and 48 B written per record, trace_id read once
   more) is queued on the handle's stream behind that: DEVICE columns must stay as they are until the
   handle's next synchronising call (zk_sp_info, zk_sp_exist, zk_sp_gather, zk_sp_summaries, zk_sp_traces, zk_sp_compact,
   zk_sp_expire, zk_sp_observe). A record whose place falls outside its bucket's slice (it cannot while the columns
   stay as they were) is dropped, never written elsewhere. n == 0 is ZK_OK; n >= 2^32 is
   ZK_ERR_UNSUPPORTED. */
zk_status   zk_sp_observe(zk_sp* sp, const zk_span_cols* in, uint32_t flags);
/* Empty the store: every segment is freed. */
zk_status   zk_sp_reset(zk_sp* sp);
/* Merge all segments into one (see Layout): 48 B read and 48 B written per entry. Fewer than two
   segments: nothing to do. Synchronises. */
zk_status   zk_sp_compact(zk_sp* sp);
/* entries in the store, segments, bytes of HBM the segments hold. Any of the three pointers may be
   NULL. Synchronises. */
zk_status   zk_sp_info(zk_sp* sp, uint64_t* entries, uint64_t* segments, uint64_t* bytes);
/* found[i] = 1 when ids[i] is a member, else 0: answers in the order asked, a duplicated id answered as
   often as asked.
     ids     n trace ids: device memory under ZK_BATCH_DEVICE_PTRS (no other flag is accepted), else host.
     n       1..ZK_SP_MAX_IDS; more is ZK_ERR_INVALID_ARG; 0 is ZK_OK and writes nothing.
     found   a HOST array of n bytes.
   One work item per (asked id, segment) reads the trace_id slice of the id's bucket in that segment and
   nothing else (a slice longer than 4096 entries is split over several workgroups). An empty store
   answers without a device pass. Synchronises. */
zk_status   zk_sp_exist(zk_sp* sp, const uint64_t* ids, uint32_t n, uint32_t flags, uint8_t* found);
/* The fragments of the asked traces.
     ids, n, flags   as for zk_sp_exist; n == 0 is ZK_OK with *n_out = 0.
     counts  a HOST array of n entries: counts[i] = the fragments of ids[i] (0: not a member).
     out     seven HOST columns of `cap` entries each. The rows of ids[0] come first, then those of
             ids[1], and so on; a duplicated id gets its rows again; inside one trace the rows are in
             CANONICAL ORDER (the host sorts them). out, or any of its columns, may be NULL only when
             cap == 0.
     n_out   the total number of rows, the sum of counts.
   When cap is below the total the call returns ZK_ERR_CAPACITY with *n_out set to the needed total and
   counts written; no row is written. cap == 0 with NULL columns is the sizing call.
   Two device passes: the count pass of zk_sp_exist, one synchronisation and the host's prefix sum, then
   the write pass, which reads the same slices again and appends every matching row (all seven columns,
   48 B) behind its asked id's offset, a wave's matches with one atomic. A trace may be of any length:
   no pass keeps a trace's rows in LDS. Staging for the rows (48 B each) is allocated on first use and
   grown; a refused allocation is ZK_ERR_CAPACITY. Synchronises. */
zk_status   zk_sp_gather(zk_sp* sp, const uint64_t* ids, uint32_t n, uint32_t flags, uint32_t* counts,
                         zk_sp_rows* out, uint64_t cap, uint64_t* n_out);
/* The reference's TraceSummary (TraceSummary.scala, Trace.scala) of the asked traces, at record granularity:
   only summaries cross to the host. For one asked id, over all its fragments in all segments:
     merged spans  the fragments grouped by span_id. A span is timed when any of its fragments has
                   ZK_F_HAS_ANNOTATIONS; first = the minimum first_ts and last = the maximum last_ts over its
                   TIMED fragments (an untimed fragment's times are never read).
     services      of a span: the set of service_id over its fragments with ZK_F_SVC_CLIENT |
                   ZK_F_SVC_SERVER; a fragment with neither bit gives no service and is still a fragment
                   of the span.
     span order    by first ascending (signed), ties by span_id ascending as unsigned; an untimed span counts
                   in `spans` and has no entry.
     entries       in span order, per timed span one (service_id, first, last) for each of its services,
                   ascending by id; a timed span without a service has none.
     start, end    the minimum first_ts and the maximum last_ts over the trace's timed fragments.
   The answer is a function of the store's multiset of fragments and the asked ids alone.
     ids, n, flags   as for zk_sp_gather; n == 0 is ZK_OK with *n_out = 0.
     heads   n HOST structs, in the order asked; a duplicated id is answered as often as asked; an id that is
             not found gets a head of zeros.
     out     three HOST columns of `cap` entries each: the entries of ids[0] first, then those of ids[1], and
             so on. out, or any of its columns, may be NULL only when cap == 0.
     n_out   the total number of entries, the sum of span_ts.
   When cap is below the total the call returns ZK_ERR_CAPACITY with *n_out set to the needed total and the
   heads written; no entry is written. cap == 0 with NULL columns is the sizing call. An empty store
   answers without a device pass.
   fragments, start, end, FOUND and TIMED are plain reductions, exact for a trace of any length. The merge
   by span id sorts the trace's rows in LDS, for traces of up to ZK_SP_SUM_MAX_ROWS rows; a longer trace gets
   ZK_SP_SUM_OVERFLOW, spans = span_ts = 0 and no entries (the caller merges it from zk_sp_gather's rows).
   The passes: zk_sp_gather's count pass, synchronisation and prefix sum, its write pass into the handle's
   staging (the rows stay in HBM), then k_sp_summarize over the staged rows, a trace of up to 64 rows per
   wave and a longer one per workgroup of 256 (31 B of LDS per row: sort by (span_id, service), fold, mark
   one entry per (span, service), sort by (first, span_id, service)). Entries are staged at their rows' own
   bases (a trace has at most as many entries as rows). The heads (40 B per id) are copied and the call
   synchronises; if the entries fit, the staged entry columns (20 B per row) follow in one copy and are
   packed per trace on the host. Staging is grown on use; a refused allocation is ZK_ERR_CAPACITY and leaves
   the handle as it was. */
zk_status   zk_sp_summaries(zk_sp* sp, const uint64_t* ids, uint32_t n, uint32_t flags, zk_sp_summary* heads,
                            zk_sp_span_ts* out, uint64_t cap, uint64_t* n_out);
/* The asked traces MERGED: per trace a head, its merged spans with parent, name, times and DEPTH, and the
   spans' services: what QueryService.getTraceCombosByIds needs of a trace (Trace.scala's mergeBySpanId,
   getRootMostSpan and toSpanDepths, TraceSummary.scala), at record granularity, without a fragment crossing
   to the host. For one asked id, as a function of the store's multiset of fragments alone:
     merged spans  the fragments grouped by span_id; timed, first, last and the services of a span as in
                   zk_sp_summaries.
     parent        of a span: the parent_id of its first fragment in CANONICAL ORDER that carries
                   ZK_F_HAS_PARENT, which is the minimum unsigned parent_id over those fragments. A span
                   without such a fragment has NO parent: that is a bit (ZK_SP_SPAN_HAS_PARENT), never a
                   value; parent ids 0 and 2^64 - 1 are legal.
     name          of a span: the name id (flags >> ZK_F_NAME_SHIFT) of its first fragment in canonical order
                   (parent_id, first_ts, last_ts, service_id, flags) whose name id is non-zero, else 0. This
                   order reads the RAW first_ts / last_ts of untimed fragments too (nowhere else are they read).
     SPAN ORDER    by first ascending (signed), an untimed span as INT64_MAX; ties by span_id ascending as
                   unsigned (a timed span with first == INT64_MAX and an untimed one tie and go by id).
     root-most     the first span in span order without a parent. When every span has one: from the first
                   span in span order upwards through the parents that are spans of this trace, to the span
                   whose parent is not one; on a parent chain that closes on itself, the first span the walk
                   meets twice (the reference does not terminate on such a chain: a stated choice).
     depth         of span s: 1 + the fewest parent hops from s to the root-most span; 0 when the chain from
                   s (every span has at most one parent, so there is one chain) never reaches it. The
                   root-most span is at depth 1 whatever its own parent is.
     ids, n, flags   as for zk_sp_gather; n == 0 is ZK_OK with n_out[0] = n_out[1] = 0.
     heads     n HOST structs, in the order asked; a duplicated id is answered as often as asked; an id that is
               not found gets a head of zeros. fragments, start, end, FOUND and TIMED are plain reductions,
               exact for a trace of any length; a trace of more than ZK_SP_TRACE_MAX_ROWS rows gets
               ZK_SP_TR_OVERFLOW, spans = services = 0 and root_most = 0, and emits nothing (the caller merges
               it from zk_sp_gather's rows).
     spans     cap_spans HOST structs: the spans of ids[0] in span order, then those of ids[1], and so on.
     services  cap_services HOST entries: one service_id per (span, service) pair, the spans in the order of
               `spans`, each span's ids ascending (zk_sp_span.services of them).
               spans and services may be NULL only with their cap at 0.
     n_out     n_out[0] = the total of merged spans, n_out[1] = the total of (span, service) pairs.
   When either cap is below its total the call returns ZK_ERR_CAPACITY with both totals and the heads
   written; no span and no service is written. Both caps 0 with NULL buffers is the sizing call. An empty
   store answers without a device pass.
   The passes are zk_sp_summaries' (count pass, synchronisation and prefix sum, write pass into the handle's
   staging, the same two work lists: a trace of up to ZK_SP_SUM_WAVE_ROWS rows per wave, a longer one per
   workgroup of 256), with k_sp_trace in k_sp_summarize's place: 66 B of LDS per row; a sort of the rows by
   the full canonical key, the fold per span onto its first row (times, the first fragment with a parent,
   the first named fragment), every span's parent by binary search, a second sort into span order that also
   brings equal (span, service) pairs together, the root-most span, the depths by pointer doubling
   (ceil(log2(spans)) rounds), a prefix sum over the sorted rows that places every span and every pair. Both
   are staged at their trace's own row base (spans <= rows, pairs <= rows). The heads (48 B per id) are
   copied and the call synchronises; if both outputs fit, the staged spans and services (52 B per row)
   follow in one copy and are packed per trace on the host. Staging is grown on use; a refused allocation
   is ZK_ERR_CAPACITY and leaves the handle as it was. */
zk_status   zk_sp_traces(zk_sp* sp, const uint64_t* ids, uint32_t n, uint32_t flags, zk_sp_trace* heads,
                         zk_sp_span* spans, uint64_t cap_spans, uint32_t* services, uint64_t cap_services,
                         uint64_t n_out[2]);
/* Device time in ms of the last zk_sp_observe that added a segment: the count, the sizing step (the
   counts' copy and, when the segment bound was met, the merge), the scatter. Needs zk_sp_config.timing;
   waits for the scatter. */
zk_status   zk_sp_observe_ms(zk_sp* sp, double out[3]);
/* Time in ms on the handle's stream of the last zk_sp_exist, zk_sp_gather, zk_sp_summaries or zk_sp_traces
   that ran a pass, from its first pass to its last copy (the host's prefix sum included, the host's sort not). Needs
   zk_sp_config.timing. */
zk_status   zk_sp_query_ms(zk_sp* sp, double* ms);

/* Expire whole traces by their end (see Expiry).
     min_end       the default cutoff.
     pin_ids, pin_min_end   n_pins HOST entries: trace pin_ids[i] is judged by pin_min_end[i]. n_pins == 0
                   allows NULL arrays; more than ZK_SP_MAX_PINS, or an id given twice, is
                   ZK_ERR_INVALID_ARG and changes nothing. A pin for an id that is not in the store is
                   ignored.
     removed       the entries (fragments) removed.
   An empty store, and min_end == INT64_MIN without pins, are ZK_OK with *removed = 0 and no device pass.
   A trace's fragments share one bucket but may lie in every segment, so its end is folded over the store
   before a fragment is judged. The 4096 buckets are cut into consecutive RANGES of at most
   zk_sp_config.expire_chunk entries over all segments (one bucket above that is a range of its own); a
   range is one contiguous slice of every segment. Per range a scratch table {key, end} (16 B per slot;
   slots a power of two >= 2 x the range's entries; trace id 0 apart) is cleared, then
     k_sp_end_fold   reads trace_id, last_ts, flags of the range's slices (20 B per entry): claims the key,
                     folds the end with a 64-bit atomic max; an untimed fragment only claims the key; a
                     wave folds the runs of equal ids among its 64 entries first, one table update each;
     k_sp_end_pins   keeps, beside the table, the verdict of every pinned id it finds there, and replaces
                     the id's end by all ones, which sends the mark pass to the verdicts;
     k_sp_end_mark   reads trace_id again (8 B per entry), probes, writes one bit per entry (a wave's ballot
                     as one 64-bit word) and adds the survivors per (segment, bucket).
   The scratch is bounded by the range, not by the store; the marks take entries / 8 bytes. One copy of
   the survivor counts and ONE synchronisation follow. Segments where nothing goes are untouched and not
   read again; segments where everything goes are freed; the survivors of all other segments are written
   (k_sp_expire_rewrite: the mark bits, and the seven columns of survivors only), grouped by bucket, into
   ONE new segment that takes the first of their places: the segment count never grows. When nothing goes
   nothing is rewritten, reallocated or freed. A refused allocation is ZK_ERR_CAPACITY and leaves the
   handle exactly as it was: nothing is freed or swapped in before every replacement is complete.
   Synchronises. */
zk_status   zk_sp_expire(zk_sp* sp, int64_t min_end, const uint64_t* pin_ids, const int64_t* pin_min_end,
                         uint32_t n_pins, uint64_t* removed);
/* Device time in ms of the last zk_sp_expire that ran a pass: the end-table passes of all ranges, the
   sizing step (the counts' copy and the synchronisation), the rewrite. Needs zk_sp_config.timing. */
zk_status   zk_sp_expire_ms(zk_sp* sp, double out[3]);

#ifdef __cplusplus
}
#endif
#endif /* ZKSPANS_H */
