/*
 * zkbinannots.h -- the binary-annotation store by trace id: a span's key/value annotations (Span field 8) in
 * HBM, next to the span store and the annotation store.
 *
 * The reference's TraceTimeline(traceId, rootSpanId, annotations, trace.getBinaryAnnotations) carries a trace's
 * binary annotations, and Trace.getBinaryAnnotations / getBinaryAnnotationsByKey (Trace.scala:161-171) hand
 * them out: http.uri, status codes, SQL text. This handle keeps one 44-B ROW per binary annotation of an
 * accepted span, findable by trace id, and hands the rows of the asked traces back.
 *
 * A row has the annotation store's shape on purpose: seven columns, 44 bytes:
 *   trace_id    u64
 *   span_id     u64
 *   key         u64   zk_hash_string(key); an absent key hashes as ""
 *   value       u64   zk_hash_string(value bytes); an absent value hashes as "" (NOT zk_index_value_hash:
 *                     no `| 1`). The decoder keeps the bytes: zk_ingest_string
 *   ipv4        u32   the host's ipv4, as the thrift i32's bits; 0 without a host
 *   service_id  u32   the host's service (dictionary id); 0 without a host
 *   bits        u32   bits 0..2 the TYPE; bit 3 ZK_BN_HAS_HOST; bits 16..31 the host's port (the thrift
 *                     i16's bits); bits 4..15 reserved, 0
 * The TYPE is the reference's AnnotationType ordinal (BinaryAnnotation field 3, an i32): 0 BOOL, 1 BYTES,
 * 2 I16, 3 I32, 4 I64, 5 DOUBLE, 6 STRING. An absent field 3 gives 0; a value outside 0..6 gives 7
 * (ZK_BN_TYPE_OTHER); the last occurrence wins; a field 3 of another wire type is skipped by its type.
 *
 * zk_bn_cols has the layout of zk_an_cols with `key` in the place of `ts`, so the store IS the annotation
 * store's code (zkannots.h, zk_an.hip), not a copy of it: zk_bn is a typed facade over the same core. The
 * same segments, the span store's bucket function, the same bound of ZK_AN_MAX_SEGMENTS segments with the
 * merge, the same two gather passes; no kernel of its own. Every contract below is its zk_an_* twin's, word
 * for word (zkannots.h "Semantics", "Layout", "Conventions"): every observed row is kept (a MULTISET);
 * batches and rows in any order; trace ids 0 and 2^64 - 1 legal; at most 2^32 - 1 entries per handle; a
 * refused allocation is ZK_ERR_CAPACITY and leaves the handle exactly as it was; a NULL handle or argument
 * is refused with ZK_ERR_INVALID_ARG before any device is touched; zk_bn_create touches no device, so an
 * empty store answers zk_bn_info and zk_bn_gather on a machine without one.
 *
 * CANONICAL ORDER: the rows of one trace are returned ascending lexicographically by
 *   (span_id unsigned, key as the signed i64 its bits are, type, value, ipv4, port, service_id, HAS_HOST),
 * and last by the whole `bits` word: the core's order, with the key where the core has ts. Every answer is
 * so a function of the multiset alone.
 *
 * There is no zk_bn_expire and no adjusted call: a binary row carries no time of its own, and a trace's end
 * is the span store's to judge. The types keep a zk_bn out of zk_an_expire / zk_an_adjusted_*.
 * zk_bn_reset is the only removal.
 */
#ifndef ZKBINANNOTS_H
#define ZKBINANNOTS_H

#include "zkannots.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZK_BN_BUCKETS      ZK_AN_BUCKETS
#define ZK_BN_MAX_SEGMENTS ZK_AN_MAX_SEGMENTS
#define ZK_BN_MAX_IDS      ZK_AN_MAX_IDS
#define ZK_BN_ROW_BYTES    ZK_AN_ROW_BYTES

/* zk_bn_cols.bits */
#define ZK_BN_TYPE_MASK   7u
#define ZK_BN_TYPE_BOOL   0u
#define ZK_BN_TYPE_BYTES  1u
#define ZK_BN_TYPE_I16    2u
#define ZK_BN_TYPE_I32    3u
#define ZK_BN_TYPE_I64    4u
#define ZK_BN_TYPE_DOUBLE 5u
#define ZK_BN_TYPE_STRING 6u
#define ZK_BN_TYPE_OTHER  7u
#define ZK_BN_HAS_HOST    8u
#define ZK_BN_PORT_SHIFT  16u

/* seven parallel columns: zk_bn_observe's input (host or device), zk_bn_gather's output (host) */
typedef struct zk_bn_cols {
    uint64_t* trace_id;
    uint64_t* span_id;
    uint64_t* key;
    uint64_t* value;
    uint32_t* ipv4;
    uint32_t* service_id;
    uint32_t* bits;
} zk_bn_cols;

typedef struct zk_bn zk_bn;

/* cfg: a zk_an_config; expire_chunk is ignored (there is no expiry) */
zk_status   zk_bn_create(const zk_an_config* cfg, zk_bn** out);
zk_status   zk_bn_destroy(zk_bn* bn);
const char* zk_bn_last_error(const zk_bn* bn);

/* zk_an_observe: a batch of n rows as one segment; flags: ZK_BATCH_DEVICE_PTRS or 0. DEVICE columns must stay
   as they are until the handle's next synchronising call (zk_bn_info, zk_bn_gather, zk_bn_compact,
   zk_bn_observe). n == 0 is ZK_OK; n >= 2^32 is ZK_ERR_UNSUPPORTED. */
zk_status   zk_bn_observe(zk_bn* bn, const zk_bn_cols* in, uint64_t n, uint32_t flags);
/* zk_an_reset: every segment is freed */
zk_status   zk_bn_reset(zk_bn* bn);
/* zk_an_compact: all segments into one */
zk_status   zk_bn_compact(zk_bn* bn);
/* zk_an_info: entries, segments, bytes of HBM; any pointer may be NULL. Synchronises. */
zk_status   zk_bn_info(zk_bn* bn, uint64_t* entries, uint64_t* segments, uint64_t* bytes);
/* zk_an_gather: the rows of the asked traces in the order asked, a duplicated id answered again, inside one
   trace in CANONICAL ORDER. n 1..ZK_BN_MAX_IDS (more: ZK_ERR_INVALID_ARG; 0: ZK_OK with *n_out = 0). cap below
   the total: ZK_ERR_CAPACITY with *n_out and counts set and no row written; cap == 0 with NULL columns is the
   sizing call. An empty store answers without a device pass. */
zk_status   zk_bn_gather(zk_bn* bn, const uint64_t* ids, uint32_t n, uint32_t flags, uint32_t* counts,
                         zk_bn_cols* out, uint64_t cap, uint64_t* n_out);
/* zk_an_observe_ms / zk_an_query_ms (zk_an_config.timing) */
zk_status   zk_bn_observe_ms(zk_bn* bn, double out[3]);
zk_status   zk_bn_query_ms(zk_bn* bn, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* ZKBINANNOTS_H */
