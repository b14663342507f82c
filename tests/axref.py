"""TEST INFRASTRUCTURE ONLY -- a plain-Python restatement of the annotation index (include/zkannindex.h):
the span indexer's entries (CassieSpanStore.scala:214-244 behind SpanStore.shouldIndex, :67-68), the query
with a full sort, and the query service's getTraceIds composition (QueryService.scala:97-207). It imports
nothing of the library: the hash is restated too."""
from __future__ import annotations

import json
from collections import OrderedDict
from pathlib import Path
from typing import Callable, List, Optional, Sequence, Tuple

from oracle.spans import CORE_ANNOTATIONS, UNKNOWN_SERVICE_NAME, Annotation, BinaryAnnotation, Endpoint, Span

U64 = 2 ** 64 - 1
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
ANY = 0                      # ZK_AX_ANY_VALUE
PADDING_US = 60_000_000      # Constants.TraceTimestampPadding
GOLDEN = Path(__file__).resolve().parent / "golden" / "trace_ids_by_annotation.json"


def _b(s) -> bytes:
    return s.encode() if isinstance(s, str) else bytes(s)


def hash_string(s) -> int:
    """zk_hash_string: 64-bit FNV-1a, then the splitmix64 finalizer."""
    h = 0xCBF29CE484222325
    for c in _b(s):
        h = ((h ^ c) * 0x100000001B3) & U64
    h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & U64
    h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & U64
    return h ^ (h >> 31)


def value_hash(s) -> int:
    """zk_index_value_hash: never 0."""
    return hash_string(s) | 1


def _to_int(v: int) -> int:
    """Scala's Long.toInt."""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def _host_name(e: Endpoint) -> str:
    return e.service_name if e.service_name else UNKNOWN_SERVICE_NAME  # thrift.scala:36-43


def should_index(span: Span) -> bool:
    """SpanStore.scala:67-68."""
    return not (span.is_client_side() and "client" in {_host_name(a.host).lower() for a in span.annotations if a.host is not None})


def entries_of_span(span: Span, client_rule: bool = True) -> List[tuple]:
    """[(service name, key, val, ts, trace_id)] in the decoder's order: time entries by first occurrence
    of the value, then binary entries."""
    last = span.last_annotation
    if last is None or (client_rule and not should_index(span)):
        return []
    tid = span.trace_id & U64
    out = []
    groups: "OrderedDict[str, List[Annotation]]" = OrderedDict()
    for a in span.annotations:  # :222-224
        if a.value not in CORE_ANNOTATIONS:
            groups.setdefault(a.value, []).append(a)
    for value, group in groups.items():
        m = group[0]  # :226 as.min: reduceLeft((x, y) => if (x.compare(y) <= 0) x else y), Annotation.compare
        for a in group[1:]:
            if _to_int(m.timestamp - a.timestamp) > 0:
                m = a
        if m.host is not None:  # :227-232
            out.append((_host_name(m.host), hash_string(value), 0, m.timestamp, tid))
    for b in span.binary_annotations:  # :235-241: (key, Some(value)) and (key, None) as one entry
        if b.host is not None:
            out.append((_host_name(b.host), hash_string(b.key), value_hash(b.value), last.timestamp, tid))
    return out


def entries_of_spans(spans: Sequence[Span], client_rule: bool = True) -> List[tuple]:
    return [e for s in spans for e in entries_of_span(s, client_rule)]


def trace_ids(entries, service, key: int, val: int, end_ts: int, limit: int) -> Tuple[List[tuple], int]:
    """([(trace_id, ts)] the first `limit` by ts descending then traceId ascending, matched)."""
    hit = [(e[4], e[3]) for e in entries if e[0] == service and e[1] == key and (val == ANY or e[2] == val) and e[3] <= end_ts]
    hit.sort(key=lambda t: (-t[1], t[0]))
    return hit[:limit], len(hit)


def by_annotation(entries, service, annotation, value, end_ts: int, limit: int) -> List[tuple]:
    """SpanStore.getTraceIdsByAnnotation over `entries`: a core annotation finds nothing (:201)."""
    if _b(annotation).decode("latin-1") in CORE_ANNOTATIONS:
        return []
    return trace_ids(entries, service, hash_string(annotation), ANY if value is None else value_hash(value), end_ts, limit)[0]


def intersect(id_lists: Sequence[Sequence[tuple]]) -> List[tuple]:
    """QueryService.traceIdsIntersect (:185-207), in the order of the first list's first occurrences."""
    common = [t for t, _ in id_lists[0]]
    common = [t for i, t in enumerate(common) if t not in common[:i]]
    for l in id_lists[1:]:
        common = [t for t in common if any(t == u for u, _ in l)]
    return [(t, max(ts for l in id_lists for u, ts in l if u == t)) for t in common]


def get_trace_ids(name_query: Callable, annotation_query: Callable, span_name, annotation_list, binary_annotations,
                  end_ts: int, limit: int) -> Tuple[List[tuple], int]:
    """QueryService.getTraceIds (:97-207) before constructQueryResponse. name_query(span_name, end_ts,
    limit) and annotation_query(annotation, value, end_ts, limit) return [(trace_id, ts)]. Where the
    reference throws on an empty list: all probes empty -> ([], end_ts); empty slices are left out of the
    maximum of the minima."""
    queries = []
    if span_name is not None:
        queries.append(lambda e, l: name_query(span_name, e, l))
    for a in annotation_list or ():
        queries.append(lambda e, l, a=a: annotation_query(a, None, e, l))
    for k, v in binary_annotations or ():
        queries.append(lambda e, l, k=k, v=v: annotation_query(k, v, e, l))
    if not queries:
        return list(name_query(None, end_ts, limit)), end_ts
    if len(queries) == 1:
        return list(queries[0](end_ts, limit)), end_ts
    probes = [ts for q in queries for _, ts in q(end_ts, 1)]
    if not probes:
        return [], end_ts
    padded = min(min(probes) + PADDING_US, INT64_MAX)
    ids = [list(q(padded, limit)) for q in queries]
    common = intersect(ids)
    if common:
        return common, padded
    minima = [min(ts for _, ts in l) for l in ids if l]
    return [], (max(minima) if minima else end_ts)


# ---- the validator's vectors ----------------------------------------------------------------------------
def golden() -> dict:
    return json.loads(GOLDEN.read_text())


def golden_spans(g: dict, names: Sequence[str]) -> List[Span]:
    ep = Endpoint(g["endpoint"]["ipv4"], g["endpoint"]["port"], g["endpoint"]["service"])
    out = []
    for n in names:
        s = g["spans"][n]
        out.append(Span(s["trace_id"], "methodcall", 456, None, tuple(Annotation(t, v, ep) for t, v in s["annotations"]),
                        tuple(BinaryAnnotation(k, v.encode(), "String", ep) for k, v in s["binary_annotations"])))
    return out
