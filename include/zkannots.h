/*
 * zkannots.h -- the annotation store by trace id: a span's time annotations in HBM, next to the span store.
 *
 * The reference's query service folds its adjusters over a trace before it answers (QueryService.scala:
 * 295-355; the web front end asks for Adjust.TimeSkew on every trace call), and builds a TraceTimeline from
 * every span's annotations. Both need what the 48-B record of zkagg.h drops: each annotation's own
 * timestamp, the kind of its value and its host. This handle keeps one 44-B ROW per time annotation of an
 * accepted span, findable by trace id, and hands the rows of the asked traces back; the adjuster and the
 * timeline are built on the host over them (zipkin_amd/annotstore.py, spanstore.py). Binary annotations are
 * kept by a store of their own over this one's core: zkbinannots.h.
 *
 * A row, seven columns, 44 bytes:
 *   trace_id    u64
 *   span_id     u64
 *   ts          i64   the annotation's timestamp
 *   value       u64   zk_hash_string of the value (the decoder keeps the string: zk_ingest_string)
 *   ipv4        u32   the host's ipv4, as the thrift i32's bits; 0 without a host
 *   service_id  u32   the host's service (dictionary id); 0 without a host
 *   bits        u32   bits 0..2 the KIND (0 other, 1 cs, 2 cr, 3 sr, 4 ss); bit 3 ZK_AN_HAS_HOST;
 *                     bits 16..31 the host's port (the thrift i16's bits)
 *
 * Semantics
 *  - EVERY observed row is kept. The store is a MULTISET of rows, like the span store: observing a batch
 *    again adds it again. Batches and rows may come in any order; a trace may be spread over any number of
 *    batches.
 *  - Legal: traceIds 0 and 2^64 - 1, ts at INT64_MIN / INT64_MAX, any 32-bit ipv4, service_id and bits.
 *  - CANONICAL ORDER: the rows of one trace are returned ascending lexicographically by
 *    (span_id unsigned, ts signed, kind, value, ipv4, port, service_id, HAS_HOST), and last by the
 *    whole `bits` word (its bits 4..15 are reserved: kept and returned as given). Every answer is so a
 *    function of the multiset alone.
 *
 * Layout
 *  - One zk_an_observe makes one SEGMENT: the batch's rows grouped by BUCKET. The bucket function is THE
 *    SPAN STORE'S,
 *        bucket = zk_mix64(trace_id ^ ZK_SP_SALT) >> 52          (ZK_AN_BUCKETS = ZK_SP_BUCKETS = 4096)
 *    so a trace's spans and annotations carry the same bucket number in both stores, and a later joint
 *    kernel can rely on that. Seven columns, 44 B per entry, each column 256-B aligned. The host keeps each
 *    segment's offsets[4097]; a copy of them (4 B each) lies behind the segment's columns for the lookups.
 *    The order inside a bucket's slice is not reproducible.
 *  - At most ZK_AN_MAX_SEGMENTS segments exist: an observe that would make one more first merges all
 *    segments into one (each bucket's slices concatenated in segment order into a freshly sized segment,
 *    then the old ones freed). zk_an_compact does the same on request.
 *  - At most 2^32 - 1 entries per handle: a batch that would exceed it is ZK_ERR_CAPACITY and changes
 *    nothing.
 *  - A refused allocation is ZK_ERR_CAPACITY and leaves the handle exactly as it was: nothing is freed
 *    before its replacement is complete.
 *
 * Expiry (zk_an_expire; the span store's rule, zkspans.h "Expiry", applied from this store's own rows)
 *  - A trace goes or stays WHOLE. end(trace) = the maximum ts over all the trace's rows in the whole
 *    store, over all segments. Every row is timed: there is no untimed case here. A trace survives exactly
 *    when end(trace) >= cutoff(trace); end == cutoff stays.
 *  - A trace whose rows all have ts == INT64_MIN has end = INT64_MIN: it goes at any cutoff above INT64_MIN.
 *  - cutoff(trace) = min_end, unless the call carries a pin for the trace id: then the pin's own min_end,
 *    which may be lower or higher than the default.
 *  - min_end == INT64_MIN with no pins removes nothing and rewrites nothing (segments, bytes and
 *    allocations stay); INT64_MAX keeps only the traces whose end is INT64_MAX.
 *  - After a call the store is indistinguishable, through zk_an_gather and zk_an_info's entries, from a
 *    fresh store that observed only the surviving rows. The cut is made once: a later observe of older
 *    rows enters the store again.
 *  - INVARIANT: a zk_sp (zkspans.h) and this store fed from the same zk_ingest_spans_annotated batches
 *    (every record into the one, every row into the other) and cut with the same min_end and the same pins
 *    hold the same traces: the ids with rows here are exactly the span store's surviving traces that have a
 *    timed fragment with at least one annotation. The decoder's last_ts of a record is the maximum ts of
 *    its annotations, and a record is timed exactly when it has annotations, so both stores compute the
 *    same end for such a trace.
 *  - Legal as before: trace ids 0 and 2^64 - 1, ts at the int64 bounds, a trace of any length spread over
 *    any number of segments.
 *
 * Conventions are those of zkspans.h: every entry point returns zk_status; a handle is not thread-safe; all
 * device work of a handle is ordered on one HIP stream; nothing is allocated before the first observe. Every
 * call refuses a NULL handle or argument with ZK_ERR_INVALID_ARG before any device is touched; errors go to
 * zk_an_last_error. ONE DIFFERENCE: zk_an_create touches no device either. The device is opened (and must
 * be a gfx950: ZK_ERR_NO_DEVICE otherwise) by the first observe that carries rows, so an empty store answers
 * zk_an_info and zk_an_gather on a machine without a device.
 */
#ifndef ZKANNOTS_H
#define ZKANNOTS_H

#include "zkagg.h"
#include "zkspans.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZK_AN_BUCKETS 4096u
#define ZK_AN_MAX_SEGMENTS 64u
/* the most ids one zk_an_gather asks */
#define ZK_AN_MAX_IDS 4096u
/* bytes of one row */
#define ZK_AN_ROW_BYTES 44u
/* the most pins one zk_an_expire carries */
#define ZK_AN_MAX_PINS 4096u

/* zk_an_cols.bits */
#define ZK_AN_KIND_MASK  7u
#define ZK_AN_KIND_OTHER 0u
#define ZK_AN_KIND_CS    1u
#define ZK_AN_KIND_CR    2u
#define ZK_AN_KIND_SR    3u
#define ZK_AN_KIND_SS    4u
#define ZK_AN_HAS_HOST   8u
#define ZK_AN_PORT_SHIFT 16u

typedef struct zk_an_config {
    int32_t  device;   /* HIP device ordinal */
    uint32_t timing;   /* 1: record HIP events (zk_an_observe_ms, zk_an_query_ms, zk_an_expire_ms) */
    void*    stream;   /* hipStream_t to run on, or NULL for a private stream */
    uint32_t expire_chunk; /* zk_an_expire: entries per range of buckets at most; 0: the default, 2^24 */
    uint32_t reserved[7];
} zk_an_config;

/* seven parallel columns: zk_an_observe's input (host or device), zk_an_gather's output (host) */
typedef struct zk_an_cols {
    uint64_t* trace_id;
    uint64_t* span_id;
    int64_t*  ts;
    uint64_t* value;
    uint32_t* ipv4;
    uint32_t* service_id;
    uint32_t* bits;
} zk_an_cols;

typedef struct zk_an zk_an;

zk_status   zk_an_create(const zk_an_config* cfg, zk_an** out);
zk_status   zk_an_destroy(zk_an* an);
const char* zk_an_last_error(const zk_an* an);

/* Add a batch of n rows as one segment. All seven columns of `in` are read. flags: ZK_BATCH_DEVICE_PTRS:
   `in` holds device pointers; without it `in` is host memory, staged (44 B per row), and the call waits for
   its staging copy. No other flag is accepted. A count kernel over trace_id (8 B per row) builds the
   4096-bin histogram; the call synchronises once, to read the counts it sizes the segment by (a merge, see
   Layout, synchronises once more). The scatter of the seven columns (44 B read and 44 B written per row,
   trace_id read once more) is queued on the handle's stream behind that: DEVICE columns must stay as they
   are until the handle's next synchronising call (zk_an_info, zk_an_gather, zk_an_compact, zk_an_expire,
   zk_an_observe).
   A row whose place falls outside its bucket's slice (it cannot while the columns stay as they were) is
   dropped, never written elsewhere. n == 0 is ZK_OK; n >= 2^32 is ZK_ERR_UNSUPPORTED. */
zk_status   zk_an_observe(zk_an* an, const zk_an_cols* in, uint64_t n, uint32_t flags);
/* Empty the store: every segment is freed. */
zk_status   zk_an_reset(zk_an* an);
/* Merge all segments into one (see Layout): 44 B read and 44 B written per entry. Fewer than two segments:
   nothing to do. Synchronises. */
zk_status   zk_an_compact(zk_an* an);
/* entries in the store, segments, bytes of HBM the segments hold. Any of the three pointers may be NULL.
   Synchronises. */
zk_status   zk_an_info(zk_an* an, uint64_t* entries, uint64_t* segments, uint64_t* bytes);
/* The rows of the asked traces: zk_sp_gather's contract.
     ids     n trace ids: device memory under ZK_BATCH_DEVICE_PTRS (no other flag is accepted), else host.
     n       1..ZK_AN_MAX_IDS; more is ZK_ERR_INVALID_ARG; 0 is ZK_OK with *n_out = 0.
     counts  a HOST array of n entries: counts[i] = the rows of ids[i] (0: none).
     out     seven HOST columns of `cap` entries each. The rows of ids[0] come first, then those of ids[1],
             and so on; a duplicated id gets its rows again; inside one trace the rows are in CANONICAL
             ORDER (the host sorts them). out, or any of its columns, may be NULL only when cap == 0.
     n_out   the total number of rows, the sum of counts.
   When cap is below the total the call returns ZK_ERR_CAPACITY with *n_out set to the needed total and
   counts written; no row is written. cap == 0 with NULL columns is the sizing call. An empty store answers
   without a device pass.
   Two device passes: the count pass (a workgroup per asked id, segment and part of the slice reads the
   trace_id slice of the id's bucket; a slice longer than 4096 entries is split over several workgroups),
   one synchronisation and the host's prefix sum, then the write pass, which reads the same slices again
   and appends every matching row (all seven columns, 44 B) behind its asked id's offset, a wave's matches
   with one atomic. A trace may be of any length: no pass keeps a trace's rows in LDS. Staging for the rows
   (44 B each) is allocated on first use and grown; a refused allocation is ZK_ERR_CAPACITY. Synchronises. */
zk_status   zk_an_gather(zk_an* an, const uint64_t* ids, uint32_t n, uint32_t flags, uint32_t* counts,
                         zk_an_cols* out, uint64_t cap, uint64_t* n_out);
/* Device time in ms of the last zk_an_observe that added a segment: the count, the sizing step (the counts'
   copy and, when the segment bound was met, the merge), the scatter. Needs zk_an_config.timing; waits for
   the scatter. */
zk_status   zk_an_observe_ms(zk_an* an, double out[3]);
/* Time in ms on the handle's stream of the last zk_an_gather that ran a pass, from its first pass to its
   last copy (the host's prefix sum included, the host's sort not). Needs zk_an_config.timing. */
zk_status   zk_an_query_ms(zk_an* an, double* ms);

/* Expire whole traces by their end (see Expiry).
     min_end       the default cutoff.
     pin_ids, pin_min_end   n_pins HOST entries: trace pin_ids[i] is judged by pin_min_end[i]. n_pins == 0
                   allows NULL arrays; n_pins > 0 with a NULL array, more than ZK_AN_MAX_PINS, or an id
                   given twice, is ZK_ERR_INVALID_ARG and changes nothing. A pin for an id that is not in
                   the store is ignored.
     removed       the entries (rows) removed.
   An empty store, and min_end == INT64_MIN without pins, are ZK_OK with *removed = 0 and no device pass:
   nothing is reallocated or freed, and a handle that never opened a device answers without one.
   A trace's rows share one bucket but may lie in every segment, so its end is folded over the store
   before a row is judged. The 4096 buckets are cut into consecutive RANGES of at most
   zk_an_config.expire_chunk entries over all segments (one bucket above that is a range of its own); a
   range is one contiguous slice of every segment. Per range a scratch table {key, end} (16 B per slot;
   slots a power of two >= 2 x the range's entries and >= 1024; trace id 0 apart, in a slot behind the
   table; home slot = zk_mix64(trace_id ^ ZK_SP_END_SALT) & (slots - 1), apart from the bucket salt: a
   range of buckets shares the bucket hash's high bits) is cleared, then
     k_an_end_fold   reads trace_id and ts of the range's slices (16 B per entry; there is no flags column
                     to read): claims the key, folds the end with a 64-bit atomic max; a wave folds the
                     runs of equal ids among its 64 entries first, one table update each;
     k_an_end_pins   keeps, beside the table, the verdict of every pinned id it finds there, and replaces
                     the id's end by all ones, which sends the mark pass to the verdicts;
     k_an_end_mark   reads trace_id again (8 B per entry), probes, writes one bit per entry (a wave's ballot
                     as one 64-bit word) and adds the survivors per (segment, bucket).
   The scratch is bounded by the range, not by the store; the marks take entries / 8 bytes. One copy of
   the survivor counts and ONE synchronisation follow. Segments where nothing goes are untouched and not
   read again; segments where everything goes are freed; the survivors of all other segments are written
   (k_an_expire_rewrite: the mark bits, and the seven columns of survivors only), grouped by bucket, into
   ONE new segment that takes the first of their places: the segment count never grows. When nothing goes
   nothing is rewritten, reallocated or freed. A refused allocation is ZK_ERR_CAPACITY and leaves the
   handle exactly as it was: nothing is freed or swapped in before every replacement is complete.
   Synchronises. */
zk_status   zk_an_expire(zk_an* an, int64_t min_end, const uint64_t* pin_ids, const int64_t* pin_min_end,
                         uint32_t n_pins, uint64_t* removed);
/* Device time in ms of the last zk_an_expire that ran a pass: the end-table passes of all ranges, the
   sizing step (the counts' copy and the synchronisation), the rewrite. Needs zk_an_config.timing; an error
   without it, or before an expiry that ran a pass. */
zk_status   zk_an_expire_ms(zk_an* an, double out[3]);

/* ---- time-skew-adjusted trace summaries (the joint call over a zk_an and a zk_sp) ------------------------ */

/* the most annotation rows of a trace that zk_an_adjusted_summaries adjusts on the device; a power of two.
   How it is chosen: one workgroup holds one trace in the 160 KiB of LDS of a CU. A merged span takes 52 B
   there and a trace has at most ZK_SP_TRACE_MAX_ROWS = 2048 of them (104 KiB); a row takes 26 B (its span id
   and ts [8 B], ipv4 and bits [4 B], a 16-bit sort index; value and service_id are read from HBM only to break
   the ties of the sort). 64 B + 2048 x 52 B + 2048 x 26 B = 159,808 B fits; 4096 rows would not. */
#define ZK_AN_ADJ_MAX_ROWS 2048u
/* the plan: a trace of up to this many annotation rows AND merged spans is adjusted by one wave, any other
   by a workgroup of 256 */
#define ZK_AN_ADJ_WAVE_ROWS 64u
/* zk_sp_summary.state of zk_an_adjusted_summaries: the ZK_SP_SUM_* bits, and */
#define ZK_AN_ADJ_ANNOTATED 8u   /* the trace has rows in the annotation store */
#define ZK_AN_ADJ_OVERFLOW  16u  /* more than ZK_SP_TRACE_MAX_ROWS fragments, or more than ZK_AN_ADJ_MAX_ROWS
                                    annotation rows: spans = span_ts = 0 and no entries */

/* getTraceSummariesByIds with Adjust.TimeSkew, on the device: zk_sp_summaries' answer for the traces as the
   reference's TimeSkewAdjuster leaves them. Only summaries cross to the host. For one asked id, as a function
   of both stores' multisets alone (DESIGN.md 5l states the rules; zipkin_amd/spanstore.py is their host form):
     merged spans  the span store's (zk_sp_traces): fragments grouped by span id, the parent of a span from its
                   first fragment in canonical order with ZK_F_HAS_PARENT, its services ascending.
     span times    a span that has annotation rows takes first and last from the minimum and maximum ts of its
                   rows, and is timed even when no fragment of it is; a span without rows keeps its record
                   times. Rows whose span_id is not a span of the trace are ignored.
     SPAN ORDER    (first, span_id unsigned), an untimed span as INT64_MAX, computed from THESE times.
     not annotated a trace without rows in the annotation store is answered exactly as zk_sp_summaries answers
                   it: nothing is adjusted and nothing pruned.
     root          the first span in span order without a parent. Without one nothing is shifted and nothing
                   pruned (the annotation-derived times hold). With one, only the spans whose parent chain
                   reaches the root stay.
     the walk      from the root down. A span's list is its rows in CANONICAL ORDER; a shift changes a row's ts
                   and never the list's order. The children of a span are the spans whose parent is its id,
                   in the span order from before the walk. At a span, in this order:
                   1. the skew its parent handed down is taken out of its list;
                   2. if the list has exactly one cs and one cr, at most one sr and one ss and not both, and
                      the span has children (a CLIENT-ONLY span): the endpoint is the host of the first cs or
                      cr in the first child's list (none: no endpoint); every child that has a cs and a cr
                      (the first of each) gets skew(cs, cr, child cs, child cr) taken out of its list. The
                      reference also injects sr = cs and ss = cr here; they never move the span's minimum or
                      maximum and make its own skew 0, so no row is materialised;
                   3. else, if the list has all of cs, cr, sr, ss (the LAST of each): skew(cs, cr, sr, ss) with
                      the sr's host as the endpoint is taken out of its list and handed to its children.
     skew          cd = cr - cs, sd = ss - sr; none when sd > cd or (cs < sr and cr > ss); latency = (cd - sd)
                   / 2, skew = sr - latency - cs; none when it is 0 or there is no endpoint. The arithmetic is
                   the JVM's: 64-bit wrap, / 2 truncated toward zero.
     a shift       of a list by (endpoint, skew): ts -= skew for every row that has a host and whose ipv4 is the
                   endpoint's, or that is a cs or cr on 127.0.0.1.
     the answer    the surviving spans, their times taken again from their lists, in span order again.
   The head and the entries are zk_sp_summaries': start and end are the minimum first and maximum last over
   the timed spans of the adjusted trace, fragments counts the span store's rows, spans the adjusted trace's
   spans, span_ts its entries: per timed span, in span order, one (service_id, first, last) per service of
   the span, ascending. state: ZK_SP_SUM_FOUND, ZK_SP_SUM_TIMED, ZK_AN_ADJ_ANNOTATED, ZK_AN_ADJ_OVERFLOW.
   An overflowed trace has spans = span_ts = 0 and no entries; fragments, FOUND and ANNOTATED are exact for
   it, and the caller completes it on the host. An annotated one has start = end = 0 and TIMED clear; one
   without rows keeps zk_sp_summaries' head (start, end, TIMED, ZK_SP_SUM_OVERFLOW) beside the new bit.
     an, sp  the two handles, on the same device (else ZK_ERR_INVALID_ARG). Errors go to zk_an_last_error.
     ids, n, flags   as for zk_sp_summaries; n > ZK_AN_MAX_IDS is ZK_ERR_INVALID_ARG; n == 0 is ZK_OK.
     heads   n HOST structs in the order asked; a duplicated id is answered as often as asked; an id the span
             store does not hold gets a head of zeros (whatever the annotation store holds of it).
     out, cap, n_out   as for zk_sp_summaries: when cap is below the total the call returns ZK_ERR_CAPACITY
             with *n_out set and the heads written; no entry is written. cap == 0 with NULL columns is the
             sizing call.
   NULL handles or arguments are refused before any device is touched. An empty annotation store hands the
   call to zk_sp_summaries. Otherwise the passes are: zk_sp_traces' on the span store's stream, which leave
   every asked trace's merged spans and services in its staging and end synchronised; then on THIS handle's
   stream zk_an_gather's count pass, synchronisation and prefix sum, its write pass into this handle's staging,
   and k_an_adjust over both stagings on two work lists (a wave or a workgroup per trace, above). In LDS: the
   span ids sorted once (every span's parent by binary search, and the rank that breaks the span order's
   ties), the rows sorted by the full canonical key, every span's run of rows by binary search, the span
   order, the root, the walk LEVEL BY LEVEL (all shifts a span hands to its children happen during its own
   visit, so the spans of a level are visited at once; a span's level is found as the walk arrives, one
   round per level), the times again, the span order again, a prefix sum that places the entries. Entries are
   staged at the trace's row base in the span store's numbering (entries <= fragments). The heads (40 B per
   id) are copied and the call synchronises; if the entries fit, the staged columns follow in one copy and are
   packed per trace on the host. zk_an_query_ms covers this handle's passes, zk_sp_query_ms the span store's.
   A call with n > 0 that ran no k_an_adjust (the annotation store is empty, no asked id is in the span store,
   or every found trace overflowed) leaves no timed lookup behind: zk_an_query_ms is then an error until the next
   lookup, never an earlier call's time.
   Staging is grown on use; a refused allocation is ZK_ERR_CAPACITY. Synchronises. */
zk_status   zk_an_adjusted_summaries(zk_an* an, zk_sp* sp, const uint64_t* ids, uint32_t n, uint32_t flags,
                                     zk_sp_summary* heads, zk_sp_span_ts* out, uint64_t cap, uint64_t* n_out);

/* ---- time-skew-adjusted traces (the second joint call) --------------------------------------------------- */

/* zk_an_adjusted_traces' head of one asked id, 56 bytes: zk_sp_trace's fields with the same meaning, over the
   ADJUSTED trace, and the trace's entries in the row columns */
typedef struct zk_an_trace {
    uint64_t trace_id;   /* the asked id; 0 when the span store lacks it (the whole head is zeros then) */
    int64_t  start;      /* the minimum first and the maximum last over the timed spans of the adjusted trace */
    int64_t  end;
    uint64_t root_most;  /* the span id of getRootMostSpan over the adjusted trace; 0 when spans == 0 */
    uint32_t fragments;  /* the span store's rows of the trace */
    uint32_t spans;      /* its entries in the span column */
    uint32_t services;   /* its entries in the services column */
    uint32_t state;      /* ZK_SP_TR_FOUND, ZK_SP_TR_TIMED, ZK_SP_TR_OVERFLOW, ZK_AN_ADJ_ANNOTATED, ZK_AN_ADJ_OVERFLOW */
    uint32_t rows;       /* its entries in the row columns, injected ones included */
    uint32_t reserved;   /* 0 */
} zk_an_trace;

/* one span of an adjusted trace, 56 bytes: zk_sp_span's fields under the same names, then */
typedef struct zk_an_span {
    uint64_t span_id;
    uint64_t parent_id;
    int64_t  first;      /* 0 when untimed */
    int64_t  last;
    uint32_t name;
    uint32_t depth;
    uint32_t services;
    uint32_t bits;       /* ZK_SP_SPAN_* */
    uint32_t rows;       /* the span's entries in the row columns, injected ones included */
    uint32_t injected;   /* 0, or 2: the sr and ss of a client-only span, its last two rows */
} zk_an_span;

/* getTraceCombosByIds / getTraceTimelinesByIds / getTracesByIds with Adjust.TimeSkew, on the device: the asked
   traces as the reference's TimeSkewAdjuster leaves them, with every span's annotations. The adjuster's rules
   are zk_an_adjusted_summaries' above (merged spans, span times, SPAN ORDER, root, the walk, skew, a shift);
   this call emits what that one drops. Per asked id, as a function of both stores' multisets alone:
     spans     the surviving spans in the adjusted span order. first and last from their lists again (a span
               without rows keeps its record times; 0 when untimed); name and services are zk_sp_traces';
               ZK_SP_SPAN_TIMED when the span has rows or a timed fragment; ZK_SP_SPAN_HAS_PARENT unchanged;
               ZK_SP_SPAN_PARENT_FOUND when the parent is a span of the ADJUSTED trace. The services column
               holds the survivors' service ids in the same order, ascending per span.
     rows      per span in that order its rows in CANONICAL ORDER (a shift never reorders a list): ts is the
               adjusted value, every other column as stored. Rows of pruned spans, and rows whose span_id is no
               span of the trace, are not emitted.
     injected  a CLIENT-ONLY span (the walk, 2.) gets the reference's two injected annotations behind its own
               rows, sr then ss: ts = the span's first cs (sr) / first cr (ss) after the handed-down shift,
               value = zk_hash_string("sr") / ("ss"), the kind SR / SS, and the host the whole endpoint of the
               first cs or cr in the first child's list (ipv4, port, service_id, ZK_AN_HAS_HOST); without such
               a host ipv4 = service_id = 0 and bits = the kind alone. They never move the span's first or last.
     annotated, with a root      root_most is the root, depth the walk's level (the root 1), and the root
               carries ZK_SP_SPAN_ROOT_MOST.
     annotated, every span with a parent   nothing is shifted, pruned or injected: all spans in the
               annotation-derived span order with all rows of known spans. root_most and depth are zk_sp_traces'
               rules (root-most, depth) over THAT order: from the first span up through the parents the trace
               holds, ending where the chain would repeat; then level by level down the children, a span
               reached twice keeping its first depth.
     not annotated   zk_sp_traces' answer span for span, rows = 0; ZK_SP_TR_OVERFLOW stays beside
               ZK_AN_ADJ_OVERFLOW if it was set.
     overflow  more than ZK_SP_TRACE_MAX_ROWS fragments or more than ZK_AN_ADJ_MAX_ROWS rows: ZK_AN_ADJ_OVERFLOW,
               spans = services = rows = 0 and nothing emitted; fragments, FOUND and ANNOTATED are exact (an
               annotated one has start = end = 0 and TIMED clear, as above).
   Arguments:
     an, sp, ids, n, flags   as for zk_an_adjusted_summaries.
     heads     n HOST structs in the order asked; a duplicated id is answered as often as asked; an id the span
               store lacks gets a head of zeros.
     spans, services, rows   HOST outputs of cap_spans, cap_services, cap_rows entries: the traces one after
               another in the order asked. All seven row columns are written (trace_id is the asked id). Each
               may be NULL (rows: or any of its columns) only with its cap at 0.
     totals    the totals of spans, services and rows.
   When any capacity is short the call returns ZK_ERR_CAPACITY with totals set and the heads written; no span,
   service or row is written. All caps 0 with NULL outputs is the sizing call. NULL handles or arguments and
   n > ZK_AN_MAX_IDS are refused before any device is touched; n == 0 is ZK_OK. An empty annotation store hands
   the call to zk_sp_traces (rows = 0 in every head).
   The passes are zk_an_adjusted_summaries', with k_an_adjust's emitting instantiation: behind the second span
   order a prefix sum over the sorted positions of (rows + injected) and of services places every survivor's
   rows and pairs; the spans are written a thread per position; the rows are written with all threads of the
   workgroup striding over the OUTPUT rows, each finding its span by binary search over the spans' row
   offsets (kept in LDS fields that are dead behind the walk: the budget stays 159,808 B at both bounds);
   value and service_id come from the staged rows in HBM. A trace emits at most A + 2 S rows (A its rows, S
   its spans): the row staging holds the sum of that over the asked traces, and a trace's rows lie at its row
   base plus twice its span base; spans and pairs lie at its base in the span store's numbering. The heads
   (56 B per id) are copied and the call synchronises; if all three outputs fit, one copy per output follows
   and each is packed per trace on the host. zk_an_query_ms / zk_sp_query_ms as for the summaries call.
   Staging is grown on use; a refused allocation is ZK_ERR_CAPACITY. Synchronises. */
zk_status   zk_an_adjusted_traces(zk_an* an, zk_sp* sp, const uint64_t* ids, uint32_t n, uint32_t flags,
                                  zk_an_trace* heads, zk_an_span* spans, uint64_t cap_spans,
                                  uint32_t* services, uint64_t cap_services, zk_an_cols* rows, uint64_t cap_rows,
                                  uint64_t totals[3] /* spans, services, rows */);

#ifdef __cplusplus
}
#endif
#endif /* ZKANNOTS_H */
