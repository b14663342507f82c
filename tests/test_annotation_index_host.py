"""The annotation index without a device: the C ABI's refusals (include/zkannindex.h), the value hash,
the host decoder's entries (zk_ingest_spans_indexed) against tests/axref.py, and the query service's
getTraceIds composition over stub indices. Every comparison is exact equality."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from oracle.spans import Annotation, BinaryAnnotation, Endpoint, Span
from tests import axref, thriftenc
from zipkin_amd import AnnotationItems, IndexedTraceId, ZkError, _abi, get_trace_ids, trace_ids_intersect
from zipkin_amd.annindex import key_hash, value_hash
from zipkin_amd.ingest import SpanDecoder, hash_string

WEB, DB = Endpoint(1, 80, "web"), Endpoint(2, 5432, "db")
NONAME, CLIENT = Endpoint(3, 1, ""), Endpoint(4, 1, "Client")
T = 1_400_000_000_000_000


def ba(key, value, host=WEB):
    return BinaryAnnotation(key, value, "String", host)


def fragments():
    """The spans whose entries the decoder has to get right, one property each."""
    return [
        # no annotations: no last annotation, so no entries, whatever its binary annotations
        Span(1, "get", 10, None, (), (ba("k", b"v"),)),
        # a hostless annotation gives nothing; the one beside it does
        Span(2, "get", 11, None, (Annotation(T + 10, "foo", None), Annotation(T + 11, "bar", WEB))),
        # a repeated value whose later copy has the smaller timestamp: the later copy's host and time
        Span(3, "get", 12, 10, (Annotation(T + 50, "dup", WEB), Annotation(T + 40, "dup", DB), Annotation(T + 45, "dup", WEB))),
        # a pair whose timestamp difference wraps the 32-bit compare: the LATER one is the minimum
        Span(4, "get", 13, None, (Annotation(T, "wrap", WEB), Annotation(T + 2 ** 31 + 5, "wrap", DB))),
        # ... and one just below the wrap, where the earlier one stays
        Span(5, "get", 14, None, (Annotation(T, "wrap", WEB), Annotation(T + 2 ** 31 - 5, "wrap", DB))),
        # an empty host name is "Unknown service name"
        Span(6, "get", 15, None, (Annotation(T + 1, "note", NONAME),), (ba("k", b"v", NONAME),)),
        # core values give no time entry; binary entries carry the span's LAST timestamp
        Span(7, "get", 16, None, (Annotation(T + 1, "sr", WEB), Annotation(T + 9, "ss", WEB), Annotation(T + 3, "custom", DB)),
             (ba("http.uri", b"/a"), ba("http.uri", b"/b"), ba("sql", b"select", DB))),
        # a binary annotation without a host gives nothing; an empty value is a value
        Span(8, "get", 17, None, (Annotation(T + 2, "x", WEB),), (ba("nohost", b"v", None), ba("empty", b""))),
        # the client rule: cs, and the host "Client" on another annotation
        Span(9, "get", 18, None, (Annotation(T + 5, "cs", WEB), Annotation(T + 6, "note", CLIENT)), (ba("k", b"v"),)),
        # a server-side span of "client" is indexed
        Span(10, "get", 19, None, (Annotation(T + 5, "sr", CLIENT), Annotation(T + 6, "note", CLIENT)), (ba("k", b"v", CLIENT),)),
        # cr without a "client" host is indexed
        Span(2 ** 64 - 1, "get", 20, None, (Annotation(T + 5, "cr", WEB), Annotation(T + 7, "note", DB))),
    ]


def encode(spans, snappy):
    blobs = [thriftenc.span(s) for s in spans]
    return [thriftenc.snappy(b) for b in blobs] if snappy else blobs


def named_rows(dec, items):
    names = dec.service_names()
    return [(names[s], k, v, ts, tid) for s, k, v, ts, tid in items.rows()]


# ---- the C ABI -----------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    L = _abi.lib()
    h = C.c_void_p()
    cfg = _abi.zk_ax_config()
    assert L.zk_ax_create(None, C.byref(h)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ax_create(C.byref(cfg), None) == _abi.ZK_ERR_INVALID_ARG
    for s in (0, _abi.ZK_AX_MAX_SERVICES + 1):
        cfg.num_services = s
        assert L.zk_ax_create(C.byref(cfg), C.byref(h)) == _abi.ZK_ERR_INVALID_ARG
    it = _abi.zk_ingest_index_items()
    n32, n64, d = C.c_uint32(), C.c_uint64(), C.c_double()
    ids, ts = (C.c_uint64 * 1)(), (C.c_int64 * 1)()
    assert L.zk_ax_destroy(None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ax_observe(None, C.byref(it), 0) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ax_reset(None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ax_compact(None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ax_info(None, C.byref(n64), None, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ax_service_counts(None, C.byref(n64)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ax_trace_ids(None, 0, 1, 0, 0, 1, ids, ts, C.byref(n32), C.byref(n64)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ax_observe_ms(None, C.byref(d)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ax_query_ms(None, C.byref(d)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ax_last_error(None) == b"null handle"


def test_indexed_decode_refuses_null_arguments():
    L = _abi.lib()
    dec = SpanDecoder()
    n, r = C.c_uint64(), C.c_uint64()
    it = _abi.zk_ingest_index_items()  # null columns
    assert L.zk_ingest_spans_indexed(dec._h, None, None, 0, 0, 0, None, C.byref(n), C.byref(r), None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_spans_indexed(dec._h, None, None, 0, 0, 0, None, C.byref(n), C.byref(r), C.byref(it)) == _abi.ZK_ERR_INVALID_ARG
    ok = AnnotationItems.empty(4)
    ab = ok.abi(cap=4, n=0)
    assert L.zk_ingest_spans_indexed(None, None, None, 0, 0, 0, None, C.byref(n), C.byref(r), C.byref(ab)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_spans_indexed(dec._h, None, None, 0, 0, 0, None, C.byref(n), C.byref(r), C.byref(ab)) == _abi.ZK_OK  # n == 0


@pytest.mark.parametrize("s", (b"", b"BEH", b"\x00", "café".encode(), b"x" * 300))
def test_value_hash_is_the_string_hash_made_odd(s):
    L = _abi.lib()
    v = int(L.zk_index_value_hash(s, len(s)))
    assert v & 1 and v == hash_string(s) | 1 == value_hash(s) == axref.value_hash(s)
    assert hash_string(s) == key_hash(s) == axref.hash_string(s)


# ---- the decoder's entries -----------------------------------------------------------------------------
@pytest.mark.parametrize("snappy", (False, True), ids=("thrift", "snappy"))
@pytest.mark.parametrize("client_rule", (True, False), ids=("client_rule", "no_client_rule"))
def test_decode_indexed_against_the_restatement(snappy, client_rule):
    spans = fragments()
    blobs = encode(spans, snappy)
    blobs.insert(3, b"\xff\xff")  # an undecodable fragment between them: rejected, no entries
    dec = SpanDecoder()
    cols, rejected, items = dec.decode_indexed(blobs, snappy=snappy, strict=False, client_rule=client_rule)
    assert rejected == 1 and len(cols) == len(spans)
    want = axref.entries_of_spans(spans, client_rule)
    assert named_rows(dec, items) == want
    # the properties the fragments stand for, spelled out
    by_trace = {}
    for name, k, v, ts, tid in want:
        by_trace.setdefault(tid, []).append((name, k, v, ts))
    assert 1 not in by_trace
    assert by_trace[2] == [("web", hash_string("bar"), 0, T + 11)]
    assert by_trace[3] == [("db", hash_string("dup"), 0, T + 40)]
    assert by_trace[4] == [("db", hash_string("wrap"), 0, T + 2 ** 31 + 5)]
    assert by_trace[5] == [("web", hash_string("wrap"), 0, T)]
    assert [e[0] for e in by_trace[6]] == ["Unknown service name"] * 2
    assert [(e[0], e[3]) for e in by_trace[7]] == [("db", T + 3), ("web", T + 9), ("web", T + 9), ("db", T + 9)]
    assert [e[2] for e in by_trace[8]] == [0, value_hash(b"")]
    assert (9 in by_trace) == (not client_rule)
    assert 10 in by_trace and 2 ** 64 - 1 in by_trace
    # the records are zk_ingest_spans's
    dec2 = SpanDecoder()
    cols2, rejected2 = dec2.decode(blobs, snappy=snappy, strict=False)
    assert rejected2 == 1
    for k in ("trace_id", "span_id", "parent_id", "first_ts", "last_ts", "flags"):
        assert np.array_equal(getattr(cols, k), getattr(cols2, k)), k
    n1, n2 = dec.service_names(), dec2.service_names()
    has_svc = (cols.flags & (_abi.ZK_F_SVC_CLIENT | _abi.ZK_F_SVC_SERVER)) != 0
    assert [n1[i] for i in cols.service_id[has_svc]] == [n2[i] for i in cols2.service_id[has_svc]]


def test_strict_mode_and_span_names_pass_through():
    spans = fragments()
    dec = SpanDecoder()
    cols, rejected, items = dec.decode_indexed(encode(spans, False), snappy=False, strict=True, span_names=True)
    assert rejected == 0 and dec.span_names() == ["get"] and set(cols.name_ids().tolist()) == {1}
    with pytest.raises(ZkError) as e:
        SpanDecoder().decode_indexed([b"\xff\xff"], snappy=False, strict=True)
    assert e.value.status == _abi.ZK_ERR_INVALID_SPAN


def many(n):
    """n fragments: the cases above over and over, with their own trace ids."""
    base = fragments()
    return [Span(1000 + i, s.name, s.id, s.parent_id, s.annotations, s.binary_annotations) for i in range(n) for s in (base[i % len(base)],)]


def test_one_thread_and_many_threads_agree():
    blobs = encode(many(3 * 2048 + 7), False)  # enough for three decode threads, the last range uneven
    a, b = SpanDecoder(), SpanDecoder()
    ca, ra, ia = a.decode_indexed(blobs, snappy=False, one_thread=True)
    cb, rb, ib = b.decode_indexed(blobs, snappy=False)
    assert ra == rb == 0 and a.service_names() == b.service_names()
    assert ia.rows() == ib.rows() and len(ia) > len(blobs)
    for k in ("trace_id", "span_id", "parent_id", "first_ts", "last_ts", "service_id", "flags"):
        assert np.array_equal(getattr(ca, k), getattr(cb, k)), k


def test_rule_off_projection_equals_the_sketch_items():
    blobs = encode(fragments(), False)
    a, b = SpanDecoder(), SpanDecoder()
    _, _, items = a.decode_indexed(blobs, snappy=False, client_rule=False)
    _, _, kv, ann = b.decode(blobs, snappy=False, items=True)
    na, nb = a.service_names(), b.service_names()
    rows = items.rows()
    assert Counter((na[s], k) for s, k, v, _, _ in rows if v == 0) == Counter((nb[s], k) for s, k in zip(ann[0].tolist(), ann[1].tolist()))
    assert Counter((na[s], k) for s, k, v, _, _ in rows if v != 0) == Counter((nb[s], k) for s, k in zip(kv[0].tolist(), kv[1].tolist()))
    assert a.string(hash_string("http.uri")) == "http.uri" and a.string(hash_string("dup")) == "dup"


def test_item_cap_too_small_keeps_the_first_entries():
    blobs = encode(fragments(), False)
    _, _, full = SpanDecoder().decode_indexed(blobs, snappy=False)
    assert len(full) > 5
    with pytest.raises(ZkError) as e:
        SpanDecoder().decode_indexed(blobs, snappy=False, item_cap=5)
    assert e.value.status == _abi.ZK_ERR_CAPACITY
    assert e.value.items.rows() == full.rows()[:5]
    _, _, exact = SpanDecoder().decode_indexed(blobs, snappy=False, item_cap=len(full))
    assert exact.rows() == full.rows()


def test_golden_entries():
    g = axref.golden()
    spans = axref.golden_spans(g, ["span1", "span4", "span5"])
    dec = SpanDecoder()
    _, _, items = dec.decode_indexed(encode(spans, True))
    assert named_rows(dec, items) == axref.entries_of_spans(spans) == [
        ("service", hash_string("custom"), 0, 20, 123), ("service", hash_string("BAH"), value_hash(b"BEH"), 20, 123),
        ("service", hash_string("custom"), 0, 6, 999),
        ("service", hash_string("custom"), 0, 5, 999), ("service", hash_string("BAH2"), value_hash(b"BEH2"), 8, 999)]


# ---- the query service's composition -------------------------------------------------------------------
class StubNames:
    def __init__(self, entries):  # [(service, span name, ts, trace_id)]
        self.entries = entries

    def query(self, service, span_name, end_ts, limit):
        hit = [(t, ts) for s, n, ts, t in self.entries if s == service and (span_name is None or n == span_name) and ts <= end_ts]
        return sorted(hit, key=lambda x: (-x[1], x[0]))[:limit]

    def getTraceIdsByName(self, service, span_name, end_ts, limit):
        return [IndexedTraceId(*t) for t in self.query(service, span_name, end_ts, limit)]


class StubAnnotations:
    def __init__(self, entries):  # axref entries
        self.entries = entries

    def getTraceIdsByAnnotation(self, service, annotation, value, end_ts, limit):
        return [IndexedTraceId(*t) for t in axref.by_annotation(self.entries, service, annotation, value, end_ts, limit)]


def composition_world():
    rng = np.random.default_rng(7)
    names, anns = [], []
    for t in range(1, 41):
        ts = T + int(rng.integers(0, 50)) * 1_000_000
        names.append(("web", "get" if t % 2 else "put", ts, t))
        if t % 3 == 0:
            anns.append(("web", axref.hash_string("retry"), 0, ts - 5, t))
        if t % 4 == 0:
            anns.append(("web", axref.hash_string("http.uri"), axref.value_hash(b"/a"), ts, t))
        if t % 5 == 0:
            anns.append(("web", axref.hash_string("late"), 0, ts + 200_000_000, t))
    anns.append(("web", axref.hash_string("lonely"), 0, T, 1000))
    return names, anns


CASES = [
    dict(),                                                                      # no slice
    dict(span_name="get"),                                                       # one slice
    dict(annotation_list=["retry"]),
    dict(binary_annotations=[("http.uri", b"/a")]),
    dict(span_name="get", annotation_list=["retry"]),                            # two slices
    dict(annotation_list=["retry"], binary_annotations=[("http.uri", b"/a")]),
    dict(span_name="put", annotation_list=["retry"], binary_annotations=[("http.uri", b"/a")]),  # three
    dict(span_name="get", annotation_list=["lonely"]),                           # an empty intersection
    dict(span_name="get", annotation_list=["absent"]),                           # one slice empty
    dict(annotation_list=["absent", "nothing"]),                                 # every probe empty
    dict(annotation_list=["retry", "cs"]),                                       # a core annotation among them
    dict(annotation_list=["retry", "late"]),                                     # the padding decides
]


@pytest.mark.parametrize("case", CASES, ids=[",".join(c) or "none" for c in CASES])
@pytest.mark.parametrize("limit", (1, 3, 100))
def test_get_trace_ids_over_stubs(case, limit):
    names, anns = composition_world()
    sn, sa = StubNames(names), StubAnnotations(anns)
    end_ts = T + 40_000_000
    got, got_end = get_trace_ids(sn, sa, "web", end_ts=end_ts, limit=limit, **case)
    want, want_end = axref.get_trace_ids(
        lambda n, e, l: sn.query("web", n, e, l), lambda a, v, e, l: axref.by_annotation(anns, "web", a, v, e, l),
        case.get("span_name"), case.get("annotation_list"), case.get("binary_annotations"), end_ts, limit)
    assert [tuple(t) for t in got] == want and got_end == want_end
    assert all(isinstance(t, IndexedTraceId) for t in got)


def test_intersect_takes_the_maximum_timestamp():
    a = [IndexedTraceId(1, 10), IndexedTraceId(2, 20), IndexedTraceId(1, 12)]
    b = [IndexedTraceId(2, 25), IndexedTraceId(1, 5), IndexedTraceId(3, 1)]
    assert trace_ids_intersect([a, b]) == [(1, 12), (2, 25)] == axref.intersect([a, b])
    assert trace_ids_intersect([a, []]) == [] and trace_ids_intersect([]) == []
