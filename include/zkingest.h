/*
 * zkingest.h — C ABI of the span ingest decoders of libzkagg (host, and device: zk_ingest_dev).
 *
 * Turns stored span fragments into the 48-B columnar records of zkagg.h, replacing the job's
 * input decode: the Cassandra column value of one span fragment is
 *   Snappy(TBinaryProtocol(thrift Span))      CassieSpanStoreDefaults.SpanCodec
 *                                             (zipkin-cassandra/.../storage/cassandra/CassieSpanStore.scala:52;
 *                                             SnappyCodec.scala:32-51, ScroogeThriftCodec.scala:23-40)
 * with the Span / Annotation / BinaryAnnotation / Endpoint structs of
 *   zipkin-thrift/src/main/thrift/com/twitter/zipkin/zipkinCore.thrift:27-58.
 * The reference decodes each fragment twice (StorageRecordReader.scala:58 for the key, then
 * SpanSource.scala:20-22); this decodes once, straight into columns.
 *
 * Validation is the reference's thrift -> Span conversion (zipkin-scrooge/.../conversions/
 * thrift.scala): a null span name throws IncompleteTraceDataException (:101-104); an annotation
 * with timestamp <= 0 or an empty value throws IllegalArgumentException (:66-71); a null or empty
 * endpoint service name becomes "Unknown service name" (:36-43). ZK_INGEST_STRICT mirrors the
 * throw (the batch fails with ZK_ERR_INVALID_SPAN at the first bad span); otherwise bad spans are
 * skipped and counted. Bytes that do not decode are always ZK_ERR_INVALID_SPAN in strict mode.
 *
 * Record derivation (Span.scala:72-74,125-131,174-191,216-240): first/last
 * = min/max annotation timestamp; service = host of the first sr/ss annotation with a host, else
 * of the first cs/cr; 2-bit saturating counts of cs/cr/sr/ss; parentId presence.
 *
 * Side outputs for the sketches (zksketch.h), following the span indexer
 * (CassieSpanStore.scala:214-242; only spans with >= 1 annotation are indexed):
 *   key-value items   one per binary annotation with a host: (host service id, key hash)
 *   annotation items  one per distinct non-core annotation value with a host: (service id, value hash)
 * Hashes are zk_hash_string (64-bit FNV-1a, then the splitmix64 finalizer); the decoder keeps the
 * strings so hashes map back to names (zk_ingest_string).
 *
 * A zk_ingest owns the service-name dictionary (ids in order of first appearance, names
 * case-sensitive as Service(name) compares them, Dependencies.scala:25). It is not thread-safe.
 */
#ifndef ZKINGEST_H
#define ZKINGEST_H

#include <stddef.h>
#include <stdint.h>

#include "zkagg.h"
#include "zkstore.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZK_CODEC_THRIFT        0u  /* TBinaryProtocol-encoded Span */
#define ZK_CODEC_SNAPPY_THRIFT 1u  /* raw Snappy block of the above (the stored Cassandra value) */

#define ZK_INGEST_STRICT 1u        /* fail the batch on the first span the reference rejects */
#define ZK_INGEST_ONE_THREAD 2u    /* host decoder: decode on the calling thread only (by default up to
                                      16 threads decode contiguous ranges; records, items, service ids
                                      and errors are the same either way) */
#define ZK_INGEST_SPAN_NAMES 4u     /* keep a span-name dictionary (names compared byte for byte, any
                                      bytes) and write id + 1 into bits 16..31 of every record's flags
                                      (zkagg.h ZK_F_NAME_SHIFT); "" and "Unknown" (exactly these bytes) get
                                      0 and are never in the dictionary. A batch that would take the
                                      dictionary past its limit fails as a whole with ZK_ERR_CAPACITY.
                                      Without the flag those bits are 0 and the dictionary is untouched.
                                      Host decoder: ids in order of first appearance, the same for any
                                      thread count; at most 65535 names.
                                      Device decoder: only one made by zk_ingest_dev_create_names keeps a
                                      span-name dictionary (at most max_span_names names); one made by
                                      zk_ingest_dev_create returns ZK_ERR_UNSUPPORTED for this flag. Its
                                      ids are NOT the host decoder's: see zk_ingest_dev_create_names. */
#define ZK_INGEST_NO_CLIENT_RULE 8u /* zk_ingest_spans_indexed: emit the entries of a client-side span of the
                                      service called "client" too (shouldIndex off) */
#define ZK_INGEST_NO_ROW_STRINGS 16u /* zk_ingest_dev_spans_annotated: do not capture the rows' value strings
                                      (the rows are the same; zk_ingest_dev_string is untouched by them) */
/* Both decoders (host zk_ingest_spans, device zk_ingest_dev_spans) reject a Snappy fragment whose
 * header announces more than ZK_INGEST_MAX_FRAGMENT bytes, or more than the format can expand its
 * payload to (a 3-byte copy emits at most 64 bytes: < ZK_SNAPPY_MAX_EXPANSION x), before any
 * allocation -- a 5-byte hostile header cannot make either decoder allocate gigabytes. */
#define ZK_INGEST_MAX_FRAGMENT   (1u << 24)
#define ZK_SNAPPY_MAX_EXPANSION  22u

typedef struct zk_ingest zk_ingest;

/* caller buffers for the sketch items (any may be NULL / cap 0: not produced) */
typedef struct zk_ingest_items {
    uint32_t* kv_service;     /* binary annotations: host service id */
    uint64_t* kv_key;         /* zk_hash_string(key) */
    uint64_t  kv_cap;
    uint64_t  kv_n;           /* out: items written */
    uint32_t* ann_service;    /* non-core annotation values */
    uint64_t* ann_value;      /* zk_hash_string(value) */
    uint64_t  ann_cap;
    uint64_t  ann_n;          /* out */
} zk_ingest_items;

zk_status   zk_ingest_create(zk_ingest** out);
zk_status   zk_ingest_destroy(zk_ingest* ing);
const char* zk_ingest_last_error(const zk_ingest* ing);

/* Decode n stored fragments: fragment i is buf[offsets[i] .. offsets[i+1]) (offsets has n+1
 * entries). Records go to the host columns of `out` (capacity >= n); *n_out = records written
 * (in input order), *n_rejected = spans skipped (lenient mode). items may be NULL.
 * ZK_ERR_CAPACITY when an item buffer is too small (the records are still written). */
zk_status zk_ingest_spans(zk_ingest* ing, const uint8_t* buf, const uint64_t* offsets, uint64_t n, uint32_t codec,
                          uint32_t flags, const zk_span_cols* out, uint64_t* n_out, uint64_t* n_rejected,
                          zk_ingest_items* items);

/* caller buffers for the entries of the annotation index (zkannindex.h): five parallel columns */
typedef struct zk_ingest_index_items {
    uint32_t* service;   /* the item's own host: its service id */
    uint64_t* key;       /* zk_hash_string of a time annotation's value / a binary annotation's key */
    uint64_t* val;       /* 0 for a time annotation; zk_index_value_hash(value) for a binary annotation */
    int64_t*  ts;        /* the annotation's own timestamp / the span's last timestamp */
    uint64_t* trace_id;
    uint64_t  cap;       /* entries the arrays hold */
    uint64_t  n;         /* out (decoder) / in (zk_ax_observe): entries */
} zk_ingest_index_items;

/* zk_ingest_spans (records, rejection and dictionaries as that call's, for the same flags; like its items,
 * the entries' hosts enter the service dictionary: ids in order of first appearance, a record's own
 * service before its entries' hosts) that also writes the span indexer's annotation entries
 * (CassieSpanStore.scala:214-244) to the HOST columns of `ix`. A span gives entries when it is accepted, has at least one annotation and passes shouldIndex
 * (SpanStore.scala:67-68, evaluated exactly: its entries are dropped when some annotation's value is
 * "cs" or "cr" AND some annotation's host service name, ASCII-lowercased, is "client";
 * ZK_INGEST_NO_CLIENT_RULE switches that off):
 *   - time entries: the annotations whose value is not cs/cr/sr/ss, grouped by value; each group's
 *     minimum by Annotation.compare (the difference of the timestamps truncated to 32 bits; the first of
 *     equals), if it has a host: (host service, hash(value), 0, its own timestamp, traceId);
 *   - binary entries: every binary annotation with a host: (host service, hash(key),
 *     zk_index_value_hash(value), the span's last timestamp, traceId). An absent value hashes as "".
 * Entries are in record order; within a record the time entries come first, by first occurrence of
 * their value, then the binary entries in order; the same for any thread count. `service` is the
 * dictionary id of the item's own host ("Unknown service name" when absent or empty).
 * ix->cap too small: ZK_ERR_CAPACITY; the records and the first cap entries are written and ix->n = cap.
 * ix and its five columns must not be NULL (ZK_ERR_INVALID_ARG). */
zk_status zk_ingest_spans_indexed(zk_ingest* ing, const uint8_t* buf, const uint64_t* offsets, uint64_t n, uint32_t codec,
                                  uint32_t flags, const zk_span_cols* out, uint64_t* n_out, uint64_t* n_rejected,
                                  zk_ingest_index_items* ix);
/* caller buffers for the rows of the annotation store (zkannots.h): seven parallel columns (HOST memory for
 * zk_ingest_spans_annotated, DEVICE memory for zk_ingest_dev_spans_annotated), laid out as zk_an_cols, then
 * their capacity and count */
typedef struct zk_ingest_annotation_rows {
    uint64_t* trace_id;
    uint64_t* span_id;
    int64_t*  ts;          /* the annotation's timestamp */
    uint64_t* value;       /* zk_hash_string(value); the string is kept: zk_ingest_string */
    uint32_t* ipv4;        /* the host's ipv4 (Endpoint field 1, the i32's bits); 0 without a host */
    uint32_t* service_id;  /* the host's service id; 0 without a host */
    uint32_t* bits;        /* ZK_AN_* of zkannots.h: kind, HAS_HOST, the port (Endpoint field 2) in bits 16..31 */
    uint64_t  cap;         /* rows the arrays hold */
    uint64_t  n;           /* out (decoder): rows */
} zk_ingest_annotation_rows;

/* zk_ingest_spans (records, rejection, dictionaries, flags and `items`, which may be NULL, exactly as that
 * call's for the same arguments, ZK_INGEST_SPAN_NAMES and ZK_INGEST_ONE_THREAD included) that also writes
 * the annotation store's rows to the HOST columns of `an`: one row per time annotation of every ACCEPTED
 * span, binary annotations none.
 *   - Order: record order and, within a record, the annotation list's order (all field-6 lists appended,
 *     see Wire forms); the same for any thread count.
 *   - A row's host enters the service dictionary as an item's host does: after the record's own service
 *     and the record's items, in row order ("Unknown service name" when absent or empty). A row without a
 *     host has service_id = ipv4 = 0, no HAS_HOST bit and port 0.
 *   - The value's string is captured: zk_ingest_string(value) returns it. An annotation without a value
 *     field hashes as "".
 *   - Wire forms: the endpoint reader also reads field 1 (i32 -> ipv4) and field 2 (i16 -> port). The
 *     rules below extend to them: within an endpoint the last occurrence wins; a known id with another
 *     wire type is skipped by its type; within one annotation a later host struct keeps the earlier ipv4
 *     and port unless it carries its own. (The other decode calls read the two fields and ignore them:
 *     their outputs are what they were.)
 *   - an->cap too small: ZK_ERR_CAPACITY; the records and the first cap rows are written and an->n = cap.
 *   - an and its seven columns must not be NULL (ZK_ERR_INVALID_ARG).
 * The device decoder emits the same rows into device columns: zk_ingest_dev_spans_annotated. */
zk_status zk_ingest_spans_annotated(zk_ingest* ing, const uint8_t* buf, const uint64_t* offsets, uint64_t n, uint32_t codec,
                                    uint32_t flags, const zk_span_cols* out, uint64_t* n_out, uint64_t* n_rejected,
                                    zk_ingest_items* items, zk_ingest_annotation_rows* an);
/* caller buffers for the rows of the binary-annotation store (zkbinannots.h): seven parallel columns (HOST
 * memory for zk_ingest_spans_annotated_binary, DEVICE memory for zk_ingest_dev_spans_annotated_binary), laid
 * out as zk_bn_cols, then their capacity and count */
typedef struct zk_ingest_binary_rows {
    uint64_t* trace_id;
    uint64_t* span_id;
    uint64_t* key;         /* zk_hash_string(key); the bytes are kept: zk_ingest_string */
    uint64_t* value;       /* zk_hash_string(value bytes), without the index's `| 1`; the bytes are kept */
    uint32_t* ipv4;        /* the host's ipv4 (Endpoint field 1, the i32's bits); 0 without a host */
    uint32_t* service_id;  /* the host's service id; 0 without a host */
    uint32_t* bits;        /* ZK_BN_* of zkbinannots.h: type, HAS_HOST, the port (Endpoint field 2) in bits 16..31 */
    uint64_t  cap;         /* rows the arrays hold */
    uint64_t  n;           /* out (decoder): rows */
} zk_ingest_binary_rows;

/* zk_ingest_spans_annotated (records, rejection, `items`, ZK_INGEST_SPAN_NAMES and the time rows of `an`
 * exactly as that call's for the same arguments) that also writes the binary-annotation store's rows to the
 * HOST columns of `bn`: one row per binary annotation of every ACCEPTED span (with or without time
 * annotations).
 *   - Order: record order and, within a record, list order (all field-8 lists appended); the same for any
 *     thread count.
 *   - Wire forms of a BinaryAnnotation: field 1 string key, field 2 string value, field 3 i32 type, field 4
 *     struct host, the host read as for a time row (ipv4, port, name). The last occurrence of a scalar
 *     wins; a known id with another wire type is skipped by its type; within one binary annotation a later
 *     host struct keeps the earlier ipv4, port and name unless it carries its own; an absent or empty name
 *     is "Unknown service name". An absent key or value hashes as "". The type: an absent field 3 gives 0,
 *     a value outside 0..6 gives 7 (ZK_BN_TYPE_OTHER). Binary annotations are not validated.
 *   - A binary row's host enters the service dictionary after the record's own service, the record's items
 *     and the record's time rows, in row order. A row without a host has service_id = ipv4 = 0, no HAS_HOST
 *     bit and port 0.
 *   - The key's and the value's bytes are captured: zk_ingest_string(hash) answers for both, with their
 *     length (a value may hold NUL and bytes that are no UTF-8). One string is kept per distinct value:
 *     nothing bounds the host memory of high-cardinality values here.
 *   - bn->cap too small: ZK_ERR_CAPACITY; the records, all time rows that fit `an` and the first cap binary
 *     rows are written and bn->n = cap. The capacities of an and bn are judged independently.
 *   - an and bn and their columns must not be NULL (ZK_ERR_INVALID_ARG).
 * The device decoder emits the same rows into device columns: zk_ingest_dev_spans_annotated_binary. */
zk_status zk_ingest_spans_annotated_binary(zk_ingest* ing, const uint8_t* buf, const uint64_t* offsets, uint64_t n,
                                           uint32_t codec, uint32_t flags, const zk_span_cols* out, uint64_t* n_out,
                                           uint64_t* n_rejected, zk_ingest_items* items, zk_ingest_annotation_rows* an,
                                           zk_ingest_binary_rows* bn);
/* the value hash of the annotation index: zk_hash_string(s, len) | 1, so it is never 0 (0 asks for any
   value, and marks a time-annotation entry) */
uint64_t  zk_index_value_hash(const char* s, uint64_t len);

/* the service dictionary */
zk_status zk_ingest_num_services(const zk_ingest* ing, uint32_t* n);
zk_status zk_ingest_service_id(zk_ingest* ing, const char* name, uint64_t len, uint32_t* id);  /* adds if new */
zk_status zk_ingest_service_name(const zk_ingest* ing, uint32_t id, char* buf, uint64_t cap, uint64_t* len);
/* the span-name dictionary (ZK_INGEST_SPAN_NAMES); a record's flags carry id + 1 */
zk_status zk_ingest_num_span_names(const zk_ingest* ing, uint32_t* n);
zk_status zk_ingest_span_name_id(zk_ingest* ing, const char* name, uint64_t len, uint32_t* id);  /* adds if new */
zk_status zk_ingest_span_name(const zk_ingest* ing, uint32_t id, char* buf, uint64_t cap, uint64_t* len);
/* the string behind a key / value hash seen by this decoder (two-phase: buf NULL -> *len) */
zk_status zk_ingest_string(const zk_ingest* ing, uint64_t hash, char* buf, uint64_t cap, uint64_t* len);

/* ---- the same decoder on the device -------------------------------------------------------
 * zk_ingest_dev decodes fragments that are already in HBM (buf and offsets are device pointers)
 * into device columns, one lane per fragment (Snappy block, thrift walk, validation and record as
 * above; the indexer items through zk_ingest_dev_spans_items). Its service dictionary lives on the device: a batch's new names get ids
 * in the order of their hash-table slots (not in order of first appearance; names whose hashes
 * collide in the table may swap ids between runs), names are compared byte for byte. At most `max_services` distinct names
 * (ZK_ERR_SERVICE_RANGE past that). Results are synchronous with respect to the host (the call waits).
 *
 * Wire forms (both decoders, every path and build of the device decoder; tests/thriftref.py restates
 * them). A known field is a (field id, wire type) pair; a known id with another type is skipped by
 * its wire type like an unknown one. The last occurrence of a scalar field wins; parent_id stays set
 * once seen. Every field-6 / field-8 list of structs is appended to what earlier such lists gave
 * (Scrooge would keep the last list only); one with another element type is skipped element by
 * element. Within an annotation every host struct marks the host present, and a later one keeps the
 * earlier service name unless it carries its own; within an endpoint the last service_name wins, and
 * an absent or empty one is "Unknown service name". An annotation without a value field is valid
 * (its item string is ""), one without a timestamp has timestamp 0. Bytes after the Span's STOP are
 * ignored. A negative string length or container count, a value of an unknown type code (a container
 * of zero elements reads none) and a short read make the fragment undecodable. Validation applies to
 * decodable bytes only, in this order: no name; then per annotation in order, timestamp <= 0, then a
 * present, empty value.
 * Nesting inside one skipped value is the one point where the decoders differ: the device decoder
 * allows at most 16 containers (struct, map, set, list) open at once and treats a 17th as undecodable;
 * the host decoder allows a value inside at most 64 containers (so 64 containers around a scalar, and
 * a 65th only if it is empty) and treats anything deeper as undecodable. */
typedef struct zk_ingest_dev zk_ingest_dev;
zk_status   zk_ingest_dev_create(int32_t device, void* stream, uint32_t max_services, zk_ingest_dev** out);
zk_status   zk_ingest_dev_destroy(zk_ingest_dev* ing);
const char* zk_ingest_dev_last_error(const zk_ingest_dev* ing);
zk_status   zk_ingest_dev_spans(zk_ingest_dev* ing, const uint8_t* buf, const uint64_t* offsets, uint64_t n,
                                uint32_t codec, uint32_t flags, const zk_span_cols* out, uint64_t* n_out,
                                uint64_t* n_rejected);
/* The same decode with the span indexer's items (as zk_ingest_spans: CassieSpanStore.scala:214-242),
 * written to DEVICE buffers: kv_service / kv_key and ann_service / ann_value are device pointers
 * (either pair NULL or cap 0: not produced). Service ids are this decoder's; within a batch the items
 * come in no particular order (the sketches take a batch as a set), the multiset per batch equals the
 * host decoder's. ZK_ERR_CAPACITY when a buffer is too small (records and the first cap items are
 * still written; kv_n / ann_n are the items written). n < 2^30. The strings behind key / value hashes
 * are kept on the host side of the decoder: zk_ingest_dev_string. Slower than zk_ingest_dev_spans
 * (a second build of the decoder: a captured-string set probe per item, no copy-in prefetch). */
zk_status   zk_ingest_dev_spans_items(zk_ingest_dev* ing, const uint8_t* buf, const uint64_t* offsets, uint64_t n,
                                      uint32_t codec, uint32_t flags, const zk_span_cols* out, uint64_t* n_out,
                                      uint64_t* n_rejected, zk_ingest_items* items);
/* Several stored batches in one decode: batch b is bufs[b] + offsets[b][0..ns[b]] (device pointers;
 * host arrays of nb entries; ns[b] == 0 allowed). Records, rejected count and items (items may be
 * NULL: none) are those of zk_ingest_dev_spans(_items) over the batches joined in order; fragment
 * numbers in errors count across the batches. One set of launches and one host round trip for all
 * of them: a job reading many small stored batches (StorageRecordReader.scala:49-54, one row batch
 * per read) decodes them at the large-batch rate. */
zk_status   zk_ingest_dev_spans_multi(zk_ingest_dev* ing, uint32_t nb, const uint8_t* const* bufs,
                                      const uint64_t* const* offsets, const uint64_t* ns, uint32_t codec,
                                      uint32_t flags, const zk_span_cols* out, uint64_t* n_out,
                                      uint64_t* n_rejected, zk_ingest_items* items);
/* zk_ingest_dev_spans(_items) / zk_ingest_dev_spans_multi that also write the annotation index's entries
 * (zkannindex.h) to the five DEVICE columns of `ix`: zk_ingest_spans_indexed on the device, so stored
 * bytes reach zk_ax_observe (ZK_BATCH_DEVICE_PTRS) without leaving HBM. Records, rejection, dictionaries,
 * `items` (may be NULL: none) and ZK_INGEST_SPAN_NAMES behave exactly as in those calls for the same
 * arguments. ix, or any of its five columns, NULL: ZK_ERR_INVALID_ARG before any device is touched.
 *   - Which spans give which entries is zk_ingest_spans_indexed's rule, word for word (accepted, at least
 *     one annotation, shouldIndex evaluated exactly unless ZK_INGEST_NO_CLIENT_RULE; time entries from
 *     the non-core annotations grouped by value, the group's minimum under the 32-bit truncated compare,
 *     the first of equals, only if it has a host; binary entries from every binary annotation with a
 *     host, an absent key or value hashing as ""; an absent or empty host name is "Unknown service
 *     name"), on the wire forms documented above.
 *   - Order: the host decoder's. Record order; within a record the time entries first, by first
 *     occurrence of their value, then the binary entries in order. (Stronger than the items' "no
 *     particular order": the output is reproducible, and ZK_ERR_CAPACITY leaves a defined prefix.)
 *   - ix->cap too small: ZK_ERR_CAPACITY; the records and the first cap entries are written, ix->n = cap.
 *   - `service` is this decoder's id of the entry's own host. An entry's host enters the service
 *     dictionary like an item's host does (ids in slot order: compare through names). More names than
 *     max_services: ZK_ERR_SERVICE_RANGE; two names with one hash: ZK_ERR_INVALID_SPAN; both with
 *     ix->n = 0. A strict-mode failure or a span-name overflow returns before any entry is written
 *     (ix->n = 0).
 *   - The entries capture no strings (a query hashes its own): zk_ingest_dev_string is untouched by them.
 * The entries come from an index pass of its own after the batch's decode (count -> scan -> write over
 * slices of fragments whose decompressed Spans fit the Snappy scratch, which grows only for a fragment
 * larger than all of it); the decode kernels are those of the calls above. */
zk_status   zk_ingest_dev_spans_indexed(zk_ingest_dev* ing, const uint8_t* buf, const uint64_t* offsets, uint64_t n,
                                        uint32_t codec, uint32_t flags, const zk_span_cols* out, uint64_t* n_out,
                                        uint64_t* n_rejected, zk_ingest_items* items /* may be NULL */,
                                        zk_ingest_index_items* ix);
zk_status   zk_ingest_dev_spans_multi_indexed(zk_ingest_dev* ing, uint32_t nb, const uint8_t* const* bufs,
                                              const uint64_t* const* offsets, const uint64_t* ns, uint32_t codec,
                                              uint32_t flags, const zk_span_cols* out, uint64_t* n_out,
                                              uint64_t* n_rejected, zk_ingest_items* items, zk_ingest_index_items* ix);
/* the last index pass of this decoder: the device time between its first and last launch (ms), and the
   slices it ran in (0 / 0 before the first indexed call) */
zk_status   zk_ingest_dev_index_stats(const zk_ingest_dev* ing, double* pass_ms, uint64_t* slices);
/* zk_ingest_dev_spans(_items) / zk_ingest_dev_spans_multi that also write the annotation store's rows
 * (zkannots.h) to the seven DEVICE columns of `an` (laid out as zk_an_cols): zk_ingest_spans_annotated on
 * the device, so stored bytes reach zk_an_observe (ZK_BATCH_DEVICE_PTRS) without leaving HBM and without a
 * copy. Records, rejection, dictionaries, `items` (may be NULL: none) and ZK_INGEST_SPAN_NAMES behave exactly
 * as in those calls for the same arguments. an, or any of its seven columns, NULL: ZK_ERR_INVALID_ARG before
 * any device is touched. an->n = 0 on entry.
 *   - Rows: one per time annotation of every ACCEPTED span, none for binary annotations; all field-6 lists
 *     appended. value = zk_hash_string(value), an annotation without a value field hashing as ""; the kind
 *     from cs / cr / sr / ss; ipv4 from Endpoint field 1 (the i32's bits), the port from field 2 (the
 *     i16's bits, in bits 16..31); ZK_AN_HAS_HOST when the annotation carries a host struct (field 3), as
 *     the host decoder sets it; a row without a host has service_id = ipv4 = 0, no HAS_HOST bit and port 0;
 *     trace_id and span_id are the record's.
 *   - Endpoint wire forms: the host decoder's, word for word ("Wire forms" above and the extension in
 *     zk_ingest_spans_annotated's comment): within an endpoint the last occurrence wins; a known id with
 *     another wire type is skipped by its type; within one annotation a later host struct keeps the earlier
 *     ipv4, port and name unless it carries its own; an absent or empty name is "Unknown service name".
 *   - Order: the host decoder's. Record order and, within a record, the annotation list's order. The output
 *     is reproducible, so ZK_ERR_CAPACITY leaves a defined prefix:
 *   - an->cap too small: ZK_ERR_CAPACITY; the records and the first cap rows are written, an->n = cap.
 *   - `service_id` is THIS decoder's id of the row's host (ids in slot order: compare through names). A row's
 *     host enters the service dictionary as an entry's host does in the indexed call. More names than
 *     max_services: ZK_ERR_SERVICE_RANGE; two names with one hash: ZK_ERR_INVALID_SPAN; a strict-mode failure
 *     or a span-name overflow returns before any row is written. In all these cases an->n = 0.
 *   - Strings: after the call zk_ingest_dev_string(hash) answers for the value of every row the call wrote,
 *     as zk_ingest_string does on the host (a timeline needs the text). New values go through the captured-
 *     string set of the items path, which the pass sizes and regrows itself (with items == NULL too); the
 *     four core values are answered from the host side without a probe. ZK_INGEST_NO_ROW_STRINGS switches
 *     the capture off: the rows are identical and zk_ingest_dev_string is untouched by them (the time-skew
 *     adjuster and the summaries need no text).
 *   - Bounded stores: a row at or past cap is dropped, never written elsewhere.
 * The rows come from a pass of their own after the batch's decode, shaped like the index pass (count -> scan
 * -> write over slices of fragments whose decompressed Spans fit the Snappy scratch, honouring
 * zk_ingest_dev_set_scratch), but ONE linear walk of a fragment's field-6 lists per kernel: no grouping by
 * value and no field-8 walk. The decode kernels are those of the calls above. No call runs the index pass
 * and the rows pass together. */
zk_status   zk_ingest_dev_spans_annotated(zk_ingest_dev* ing, const uint8_t* buf, const uint64_t* offsets, uint64_t n,
                                          uint32_t codec, uint32_t flags, const zk_span_cols* out, uint64_t* n_out,
                                          uint64_t* n_rejected, zk_ingest_items* items /* may be NULL */,
                                          zk_ingest_annotation_rows* an);
zk_status   zk_ingest_dev_spans_multi_annotated(zk_ingest_dev* ing, uint32_t nb, const uint8_t* const* bufs,
                                                const uint64_t* const* offsets, const uint64_t* ns, uint32_t codec,
                                                uint32_t flags, const zk_span_cols* out, uint64_t* n_out,
                                                uint64_t* n_rejected, zk_ingest_items* items,
                                                zk_ingest_annotation_rows* an);
/* zk_ingest_dev_spans_annotated / zk_ingest_dev_spans_multi_annotated that also write the binary-annotation
 * store's rows (zkbinannots.h) to the seven DEVICE columns of `bn` (laid out as zk_bn_cols), which
 * zk_bn_observe (ZK_BATCH_DEVICE_PTRS) takes without a copy: zk_ingest_spans_annotated_binary on the device.
 * Records, rejection, dictionaries, `items`, ZK_INGEST_SPAN_NAMES and the time rows of `an` are the annotated
 * call's for the same arguments. an, bn or any of their columns NULL: ZK_ERR_INVALID_ARG before any device is
 * touched. an->n = bn->n = 0 on entry.
 *   - Rows, wire forms, order, the capacity prefix (an and bn judged independently), errors and the
 *     dictionary rule are the host decoder's and the annotated call's, word for word; service_id is THIS
 *     decoder's id (compare through names).
 *   - Strings: without ZK_INGEST_NO_ROW_STRINGS every key and value goes through the captured-string set as
 *     row values do, and zk_ingest_dev_string(hash) answers for every key and value the call wrote, with its
 *     length. With the flag the rows are identical and the set is untouched. One string is kept per distinct
 *     value on the host side: high-cardinality values are what the flag is for.
 *   - Bounded stores: a row at or past bn->cap is dropped, never written elsewhere.
 * ONE rows pass serves both lists: the count kernel decompresses a fragment once and walks field 6 and then
 * field 8 over the same bytes; the write kernel walks both again over the slice's scratch. A fragment is
 * walked when it is accepted, with or without time annotations. */
zk_status   zk_ingest_dev_spans_annotated_binary(zk_ingest_dev* ing, const uint8_t* buf, const uint64_t* offsets, uint64_t n,
                                                 uint32_t codec, uint32_t flags, const zk_span_cols* out, uint64_t* n_out,
                                                 uint64_t* n_rejected, zk_ingest_items* items /* may be NULL */,
                                                 zk_ingest_annotation_rows* an, zk_ingest_binary_rows* bn);
zk_status   zk_ingest_dev_spans_multi_annotated_binary(zk_ingest_dev* ing, uint32_t nb, const uint8_t* const* bufs,
                                                       const uint64_t* const* offsets, const uint64_t* ns, uint32_t codec,
                                                       uint32_t flags, const zk_span_cols* out, uint64_t* n_out,
                                                       uint64_t* n_rejected, zk_ingest_items* items,
                                                       zk_ingest_annotation_rows* an, zk_ingest_binary_rows* bn);
/* the last rows pass of this decoder: the device time between its first and last launch (ms), and the
   slices it ran in (0 / 0 before the first annotated call); the combined pass of an annotated_binary call */
zk_status   zk_ingest_dev_rows_stats(const zk_ingest_dev* ing, double* pass_ms, uint64_t* slices);
/* the string behind a key / value hash an items batch of this decoder has seen, or behind the value of a
   row an annotated call wrote without ZK_INGEST_NO_ROW_STRINGS (two-phase) */
zk_status   zk_ingest_dev_string(const zk_ingest_dev* ing, uint64_t hash, char* buf, uint64_t cap, uint64_t* len);
zk_status   zk_ingest_dev_num_services(const zk_ingest_dev* ing, uint32_t* n);
/* Snappy scratch (deferred fragments' Spans, names not yet in the dictionary): bump-allocated per
 * batch and grown when a batch runs out (the fragments that missed out are decoded again). `bytes`
 * sets its size from the next batch on; 0 = automatic (max(64 MiB, 24 B per fragment)). The index pass of
 * the indexed calls lays the decompressed Spans of a slice of fragments out in the same scratch: with
 * `bytes` set, a slice stays within max(bytes, the batch's largest fragment) even where the decode has
 * grown the scratch past that. */
zk_status   zk_ingest_dev_set_scratch(zk_ingest_dev* ing, uint64_t bytes);
zk_status   zk_ingest_dev_service_name(const zk_ingest_dev* ing, uint32_t id, char* buf, uint64_t cap,
                                       uint64_t* len);
/* A device decoder that also keeps a span-name dictionary in HBM (a second table, a name arena and
 * a second publish list), so that ZK_INGEST_SPAN_NAMES works on all three decode calls and both
 * codecs. max_span_names: 1..65535 (ZK_F_NAME_MASK: id + 1 must fit 16 bits), else
 * ZK_ERR_INVALID_ARG before any device is touched. Without the flag such a decoder runs the same
 * kernels as one made by zk_ingest_dev_create.
 *   - The dictionary is separate from the service dictionary (the same string may be in both with
 *     unrelated ids) and persists across batches: a name keeps its id for the decoder's life.
 *   - A batch's new names get ids in the order of their hash-table slots, as the service dictionary
 *     does, not in order of first appearance: device ids are not the host decoder's ids, and any
 *     comparison between the two goes through the names (zk_ingest_dev_span_name).
 *   - A name enters the dictionary only through a record the batch accepts.
 *   - A batch that would take the dictionary past max_span_names fails as a whole with
 *     ZK_ERR_CAPACITY; the dictionary then holds exactly the names it held before, and a later batch
 *     whose names fit decodes normally.
 *   - Two different names with one 64-bit hash are an error (ZK_ERR_INVALID_SPAN), as for service names.
 *   - The merge rule downstream (K1 kModeLinks) takes the MAXIMUM id over a span's fragments. Only
 *     when the fragments of one span carry different names can a device-decoded and a host-decoded
 *     stream therefore select different names for it; each choice is deterministic for its
 *     dictionary (the reference's own pick depends on fragment order, Span.scala:153-158).
 * zk_ingest_dev_num_span_names is 0 on a decoder without the dictionary, and zk_ingest_dev_span_name
 * then returns ZK_ERR_INVALID_ARG, as for any id past the count; two-phase (buf NULL -> *len). */
zk_status   zk_ingest_dev_create_names(int32_t device, void* stream, uint32_t max_services, uint32_t max_span_names,
                                       zk_ingest_dev** out);
zk_status   zk_ingest_dev_num_span_names(const zk_ingest_dev* ing, uint32_t* n);
zk_status   zk_ingest_dev_span_name(const zk_ingest_dev* ing, uint32_t id, char* buf, uint64_t cap, uint64_t* len);

/* ---- the Dependencies record on the wire ----------------------------------------------------
 * TBinaryProtocol thriftscala.Dependencies (zipkinDependencies.thrift:24-43) as the Cassandra
 * store writes it: WrappedDependencies.toThrift (zipkin-scrooge/.../conversions/thrift.scala:
 * 330-333) through ScroogeThriftCodec (zipkin-cassandra/.../cassandra/AggregatesBuilder.scala:31),
 * one column per record (CassandraAggregates.scala:111-116). Fields in id order, all written.
 * encode: service ids resolve through names[id] (name_lens[id] bytes, case-sensitive);
 * two-phase (out == NULL -> *len). decode: names map to ids through the dictionary of `dict`
 * exactly as stored ("" stays ""; new names are added); two-phase on the link count; bytes that
 * do not decode -> ZK_ERR_INVALID_SPAN. */
zk_status zk_dependencies_encode(int64_t start_us, int64_t end_us, const zk_dep_link* links, uint64_t n_links,
                                 const char* const* names, const uint32_t* name_lens, uint32_t num_names,
                                 uint8_t* out, uint64_t cap, uint64_t* len);
zk_status zk_dependencies_decode(zk_ingest* dict, const uint8_t* buf, uint64_t len, int64_t* start_us,
                                 int64_t* end_us, zk_dep_link* out, uint64_t cap, uint64_t* n_links);
/* the record's Cassandra row key: deps.startTime.floor(1.day).inMicroseconds
 * (CassandraAggregates.scala:111-113), integer division toward zero */
int64_t   zk_dependencies_row_key(int64_t start_us);

uint64_t  zk_hash_string(const char* s, uint64_t len);
/* raw Snappy block decompression (exposed for tools/tests): *out_len = uncompressed size; with
 * out == NULL only the size is read from the header */
zk_status zk_snappy_uncompress(const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t cap, uint64_t* out_len);

#ifdef __cplusplus
}
#endif

#endif /* ZKINGEST_H */
