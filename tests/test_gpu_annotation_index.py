"""The trace-id index by annotation on the device (include/zkannindex.h, zipkin_amd/annindex.py) against
tests/axref.py and the validator's vectors (tests/golden/trace_ids_by_annotation.json). Every comparison
is exact equality; nothing depends on the order inside a service's slice."""
import ctypes as C

import numpy as np
import pytest

from oracle.spans import Annotation, BinaryAnnotation, Endpoint, Span
from tests import axref, ixref, thriftenc
from tests.axref import ANY, INT64_MAX, INT64_MIN, U64
from zipkin_amd import (AnnotationItems, DeviceAnnotationItems, DeviceColumns, IndexedTraceId, TraceAnnotationIndex,
                        TraceDurationIndex, TraceNameIndex, ZkError, _abi, get_trace_ids)
from zipkin_amd.ingest import SpanDecoder

pytestmark = pytest.mark.gpu

T0 = 1_400_000_000_000_000
STRETCH = 16384  # k_ax_scatter: entries per workgroup at least


@pytest.fixture()
def make(gpu):
    made = []

    def factory(S, **kw):
        made.append(TraceAnnotationIndex(S, device=gpu, **kw))
        return made[-1]

    yield factory
    for idx in made:
        idx.close()


def items_of(service, key, val, ts, trace_id) -> AnnotationItems:
    n = len(service)
    full = lambda a, dt: np.full(n, a, dt) if np.isscalar(a) else np.asarray(a, dt)  # noqa: E731
    return AnnotationItems(np.asarray(service, np.uint32), full(key, np.uint64), full(val, np.uint64), full(ts, np.int64),
                           full(trace_id, np.uint64))


def observe(idx, items, device=True):
    idx.observe(DeviceAnnotationItems.from_host(items, idx.device) if device else items)


def ask(idx, entries, service, key, val, end_ts, limit):
    got, matched = idx.trace_ids(service, key, val, end_ts, limit)
    rows, want = axref.trace_ids(entries, service, key, val, end_ts, limit)
    assert all(isinstance(t, IndexedTraceId) for t in got)
    assert [tuple(t) for t in got] == rows, (service, key, val, end_ts, limit)
    assert matched == want, (service, key, val, end_ts, limit)
    return rows


def encode(spans):
    return [thriftenc.snappy(thriftenc.span(s)) for s in spans]


# ---- 1. the validator's vectors, from thrift bytes -----------------------------------------------------
@pytest.mark.parametrize("device", (True, False), ids=("device_items", "host_items"))
def test_golden_vectors(make, device):
    g = axref.golden()
    for case in g["cases"]:
        dec = SpanDecoder()
        _, rejected, items = dec.decode_indexed(encode(axref.golden_spans(g, case["load"])))
        assert rejected == 0
        idx = make(dec.num_services, services=dec.service_names())
        observe(idx, items, device)
        for q in case["queries"]:
            value = None if q["value"] is None else q["value"].encode()
            got = idx.getTraceIdsByAnnotation(q["service"], q["annotation"], value, q["end_ts"], q["limit"])
            if "trace_ids" in q:
                assert [t.trace_id for t in got] == q["trace_ids"]
            elif q["head_trace_id"] is None:
                assert got == []
            else:
                assert got[0].trace_id == q["head_trace_id"]
        assert idx.getTraceIdsByAnnotation("SERVICE", b"custom", None, 100, 1)[0] == (123, 20)  # service names fold case
        assert idx.getTraceIdsByAnnotation("service", "CUSTOM", None, 100, 1) == []             # annotations do not
        assert idx.getTraceIdsByAnnotation("badservice", "custom", None, 100, 1) == []


# ---- 2. empty index, empty service, one entry ----------------------------------------------------------
def test_empty_index_and_one_entry(make):
    idx = make(5)
    assert idx.info() == {"entries": 0, "segments": 0, "bytes": 0}
    assert idx.trace_ids(3, 7, ANY, INT64_MAX, 10) == ([], 0)
    assert idx.service_counts().tolist() == [0] * 5
    observe(idx, items_of([], 0, 0, 0, 0))  # n == 0
    assert idx.info()["segments"] == 0
    it = items_of([3], 7, 9, T0, 77)
    observe(idx, it)
    info = idx.info()
    assert (info["entries"], info["segments"]) == (1, 1) and info["bytes"] >= 32
    e = it.rows()
    assert ask(idx, e, 3, 7, ANY, INT64_MAX, 10) == [(77, T0)]
    assert ask(idx, e, 3, 7, 9, T0, 1) == [(77, T0)]
    assert ask(idx, e, 3, 7, 11, T0, 1) == [] and ask(idx, e, 3, 7, 8, T0, 1) == []  # an even value matches nothing
    assert ask(idx, e, 3, 6, ANY, T0, 1) == [] and ask(idx, e, 3, 7, 9, T0 - 1, 1) == []
    assert ask(idx, e, 2, 7, ANY, INT64_MAX, 10) == []  # an empty service beside a full one
    assert idx.service_counts().tolist() == [0, 0, 0, 1, 0]
    for bad in (dict(service_id=5), dict(limit=0), dict(limit=4097)):
        kw = dict(service_id=3, key_hash=7, val_hash=ANY, end_ts=T0, limit=1)
        kw.update(bad)
        with pytest.raises(ZkError) as err:
            idx.trace_ids(**kw)
        assert err.value.status == _abi.ZK_ERR_INVALID_ARG


def test_refusals_leave_the_outputs_as_they_were(make):
    """zk_ax_trace_ids' refusals at the C ABI, as tests/test_gpu_trace_index.py has them for zk_ix_trace_ids:
    the two calls share the select's driver behind these checks."""
    S = 2
    it = items_of(np.arange(6) % S, 7, 9, T0 + np.arange(6), 100 + np.arange(6))
    idx = make(S)
    observe(idx, it)
    L = _abi.lib()
    ids = (C.c_uint64 * 8)(*[0x5A5A5A5A5A5A5A5A] * 8)
    ts = (C.c_int64 * 8)(*[0x5A5A5A5A] * 8)
    n, m = C.c_uint32(99), C.c_uint64(99)
    #      service, limit
    bad = [(S, 8), (0xFFFFFFFF, 8), (0, 0), (0, _abi.ZK_AX_MAX_LIMIT + 1)]
    for service, limit in bad:
        assert L.zk_ax_trace_ids(idx._h, service, 7, ANY, INT64_MAX, limit, ids, ts, C.byref(n), C.byref(m)) == _abi.ZK_ERR_INVALID_ARG
        assert L.zk_ax_last_error(idx._h)
    assert L.zk_ax_trace_ids(idx._h, 0, 7, ANY, 0, 8, None, ts, C.byref(n), None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ax_trace_ids(idx._h, 0, 7, ANY, 0, 8, ids, None, C.byref(n), None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ax_trace_ids(idx._h, 0, 7, ANY, 0, 8, ids, ts, None, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ax_observe(idx._h, None, 0) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ax_service_counts(idx._h, None) == _abi.ZK_ERR_INVALID_ARG
    assert list(ids) == [0x5A5A5A5A5A5A5A5A] * 8 and list(ts) == [0x5A5A5A5A] * 8
    assert (n.value, m.value) == (99, 99)
    # matched may be NULL, and the handle still answers
    assert L.zk_ax_trace_ids(idx._h, 1, 7, ANY, INT64_MAX, 8, ids, ts, C.byref(n), None) == _abi.ZK_OK
    assert [(ids[i], ts[i]) for i in range(n.value)] == axref.trace_ids(it.rows(), 1, 7, ANY, INT64_MAX, 8)[0]


# ---- 3. the service bins' bounds -----------------------------------------------------------------------
@pytest.mark.parametrize("S", (1, 4096))
def test_service_bins(make, S):
    svc = [0, S - 1, 0, S - 1, S - 1]
    it = items_of(svc, [5, 5, 6, 5, 5], [0, 1, 0, 3, 1], T0 + np.arange(5), [10, 11, 12, 13, 14])
    idx = make(S)
    observe(idx, it)
    e = it.rows()
    for s in {0, S - 1, S // 2}:
        for k in (5, 6):
            for v in (ANY, 1):
                ask(idx, e, s, k, v, INT64_MAX, 10)
    counts = idx.service_counts()
    assert counts.sum() == 5 and counts[0] + counts[S - 1] == (10 if S == 1 else 5)


# ---- 4. a service id out of range ----------------------------------------------------------------------
@pytest.mark.parametrize("device", (True, False), ids=("device_items", "host_items"))
def test_service_out_of_range_refuses_the_batch(make, device):
    S, n = 8, 2 * STRETCH + 1000
    idx = make(S)
    good = items_of(np.arange(n) % S, 1, 0, T0, np.arange(n))
    observe(idx, good, device)
    before = idx.info()
    svc = np.arange(n) % S
    svc[n - 3] = S  # in the last workgroup's stretch of both passes
    with pytest.raises(ZkError) as err:
        observe(idx, items_of(svc, 1, 0, T0, np.arange(n)), device)
    assert err.value.status == _abi.ZK_ERR_SERVICE_RANGE
    assert idx.info() == before
    assert idx.trace_ids(1, 1, ANY, INT64_MAX, 1) == ([(1, T0)], n // S)


# ---- 5. the scatter across workgroups ------------------------------------------------------------------
@pytest.mark.parametrize("device", (True, False), ids=("device_items", "host_items"))
def test_scatter_across_workgroups(make, device):
    S, n = 7, 2 * STRETCH + 7000 + 13  # three scatter stretches, the last partial and no multiple of the workgroup
    rng = np.random.default_rng(11)
    svc = np.where(rng.random(n) < 0.9, 2, rng.integers(0, S, n))  # 90 % in one service
    keys = np.array([0, 1, 0x8000000000000000, U64, 0x1234], np.uint64)
    vals = np.array([0, 0, 1, 3, 0x8000000000000001], np.uint64)
    it = items_of(svc, keys[rng.integers(0, 5, n)], vals[rng.integers(0, 5, n)], T0 + rng.integers(0, 500, n),
                  rng.integers(0, 2 ** 63, n, dtype=np.uint64) * 2 + rng.integers(0, 2, n, dtype=np.uint64))
    idx = make(S)
    observe(idx, it, device)
    assert idx.info()["entries"] == n and idx.info()["bytes"] >= 32 * n
    assert idx.service_counts().tolist() == np.bincount(svc, minlength=S).tolist()
    e = it.rows()
    for s in range(S):
        by_service = [x for x in e if x[0] == s]
        for k in keys.tolist():
            ask(idx, by_service, s, k, ANY, INT64_MAX, 50)
            ask(idx, by_service, s, k, 3, T0 + 250, 4096)


# ---- 6. the filters ------------------------------------------------------------------------------------
def test_filters(make):
    K = 0x4000000000000002
    rows = [
        # (service, key, val, ts, trace id)
        (1, K, 0, T0 + 1, 1),                        # a time entry of K
        (1, K, 0x11, T0 + 2, 2),                     # binary entries of K
        (1, K, 0x13, T0 + 3, 3),                     # ... whose value differs in one bit
        (1, K, 0x8000000000000011, T0 + 4, 4),       # ... and in the top bit
        (1, K ^ (1 << 63), 0x11, T0 + 5, 5),         # keys that differ from K only in bit 63
        (1, K ^ 1, 0x11, T0 + 6, 6),                 # ... and only in bit 0
        (2, 0x77, 0, T0 + 7, 7),                     # a key present only in another service
        (1, K, 0x11, T0 + 8, 8),
    ]
    it = items_of(*[list(c) for c in zip(*rows)])
    idx = make(3)
    observe(idx, it)
    assert ask(idx, rows, 1, K, ANY, INT64_MAX, 10) == [(8, T0 + 8), (4, T0 + 4), (3, T0 + 3), (2, T0 + 2), (1, T0 + 1)]
    assert ask(idx, rows, 1, K, 0x11, INT64_MAX, 10) == [(8, T0 + 8), (2, T0 + 2)]
    assert ask(idx, rows, 1, K, 0x13, INT64_MAX, 10) == [(3, T0 + 3)]
    assert ask(idx, rows, 1, K, 0x8000000000000011, INT64_MAX, 10) == [(4, T0 + 4)]
    assert ask(idx, rows, 1, K ^ (1 << 63), ANY, INT64_MAX, 10) == [(5, T0 + 5)]
    assert ask(idx, rows, 1, K ^ 1, 0x11, INT64_MAX, 10) == [(6, T0 + 6)]
    assert ask(idx, rows, 1, 0x77, ANY, INT64_MAX, 10) == [] and ask(idx, rows, 2, 0x77, ANY, INT64_MAX, 10) == [(7, T0 + 7)]
    assert ask(idx, rows, 2, K, ANY, INT64_MAX, 10) == [] and ask(idx, rows, 0, K, ANY, INT64_MAX, 10) == []
    assert ask(idx, rows, 1, K, 0x10, INT64_MAX, 10) == []


# ---- 7. the select -------------------------------------------------------------------------------------
N_SEL = 20000


def select_entries(kind):
    """20,000 entries of (service 1, key 5, val 7) in three batches, with noise around them."""
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 2 ** 63, N_SEL, dtype=np.uint64) * 2 + rng.integers(0, 2, N_SEL, dtype=np.uint64)
    if kind == "distinct_ts":
        ts = T0 + rng.permutation(N_SEL)
    elif kind == "eight_ts":
        ts = T0 + rng.integers(0, 8, N_SEL) * 1000
    elif kind == "shared_ts":  # the 6,000 newest-but-2,000 share one timestamp: it straddles 4096 and 100 is inside the newer
        ts = T0 + rng.permutation(N_SEL)
        order = np.argsort(-ts)
        ts[order[2000:8000]] = ts[order[2000]]
    else:  # equal_pairs: 5,000 fully equal pairs as the newest
        ts = T0 + rng.permutation(N_SEL)
        order = np.argsort(-ts)
        ts[order[:5000]] = ts[order[0]]
        ids[order[:5000]] = ids[order[0]]
    noise = 3000
    svc = np.concatenate([np.ones(N_SEL, np.uint32), np.ones(noise, np.uint32), np.zeros(noise, np.uint32)])
    key = np.concatenate([np.full(N_SEL, 5, np.uint64), np.full(noise, 6, np.uint64), np.full(noise, 5, np.uint64)])
    val = np.concatenate([np.full(N_SEL, 7, np.uint64), np.full(2 * noise, 7, np.uint64)])
    val[N_SEL // 2:N_SEL:3] = 0  # some of the row are time entries: val ANY finds them, val 7 does not
    tsa = np.concatenate([ts, T0 + rng.integers(0, N_SEL, 2 * noise)])
    ida = np.concatenate([ids, rng.integers(0, 2 ** 63, 2 * noise, dtype=np.uint64)])
    perm = rng.permutation(len(svc))
    return items_of(svc[perm], key[perm], val[perm], tsa[perm], ida[perm])


@pytest.mark.parametrize("kind", ("distinct_ts", "eight_ts", "shared_ts", "equal_pairs"))
def test_select(make, kind):
    it = select_entries(kind)
    idx = make(2)
    third = len(it) // 3
    for a, b in ((0, third), (third, 2 * third), (2 * third, len(it))):  # three segments
        observe(idx, it.take(slice(a, b)))
    e = [x for x in it.rows() if x[0] == 1]
    for limit in (1, 100, 4096):
        for val in (ANY, 7):
            rows = ask(idx, e, 1, 5, val, INT64_MAX, limit)
            assert len(rows) == limit
    assert idx.trace_ids(1, 5, ANY, INT64_MAX, 1)[1] == N_SEL
    ask(idx, e, 1, 5, ANY, T0 + N_SEL // 2, 4096)
    ask(idx, e, 1, 6, 7, INT64_MAX, 4096)  # matched <= 4096: no histogram


# ---- 8. end_ts and the bounds of the domain ------------------------------------------------------------
def test_end_ts_and_bounds(make):
    ts = [INT64_MIN, INT64_MIN + 1, -1, 0, 1, T0, T0, T0 + 1, INT64_MAX - 1, INT64_MAX]
    tid = [0, U64, 5, 0, U64, U64, 0, 1 << 63, 0, U64]
    it = items_of([0] * len(ts), [0] * 5 + [U64] * 5, 0, ts, tid)
    idx = make(1)
    observe(idx, it)
    e = it.rows()
    for key in (0, U64):
        for end_ts in (INT64_MIN, INT64_MIN + 1, -2, 0, T0 - 1, T0, T0 + 1, INT64_MAX - 1, INT64_MAX):
            for limit in (1, 2, 10):
                ask(idx, e, 0, key, ANY, end_ts, limit)
    assert ask(idx, e, 0, U64, ANY, T0, 10) == [(0, T0), (U64, T0)]
    assert ask(idx, e, 0, 0, ANY, INT64_MIN, 10) == [(0, INT64_MIN)]
    assert ask(idx, e, 0, U64, ANY, INT64_MAX, 1) == [(U64, INT64_MAX)]


# ---- 9. segments: the merge, compact, reset, a batch twice ---------------------------------------------
def test_segments_merge_compact_reset(make):
    S, per = 5, 37
    rng = np.random.default_rng(3)
    idx = make(S)
    parts = []
    for b in range(65):
        parts.append(items_of(rng.integers(0, S, per), rng.integers(0, 3, per), rng.integers(0, 2, per) * 5,
                              T0 + rng.integers(0, 40, per), rng.integers(0, 50, per)))
        observe(idx, parts[-1], device=bool(b % 2))
        assert idx.info()["segments"] == (b + 1 if b < 64 else 2)  # the 65th first merges the 64
    e = AnnotationItems.concat(parts).rows()
    assert idx.info()["entries"] == 65 * per

    def answers():
        return [ask(idx, e, s, k, v, end, lim) for s in range(S) for k in range(3) for v in (ANY, 5)
                for end, lim in ((INT64_MAX, 4096), (T0 + 20, 7))]

    before = answers()
    idx.compact()
    assert idx.info()["segments"] == 1 and idx.info()["entries"] == 65 * per
    assert answers() == before
    idx.compact()  # fewer than two segments: nothing to do
    observe(idx, parts[0])
    observe(idx, parts[0])  # a batch observed twice is entered twice
    e2 = e + 2 * parts[0].rows()
    assert idx.info()["entries"] == 67 * per
    for s in range(S):
        ask(idx, e2, s, 1, ANY, INT64_MAX, 4096)
    idx.reset()
    assert idx.info() == {"entries": 0, "segments": 0, "bytes": 0} and idx.service_counts().sum() == 0
    assert idx.trace_ids(0, 1, ANY, INT64_MAX, 10) == ([], 0)
    observe(idx, parts[1])
    for s in range(S):
        ask(idx, parts[1].rows(), s, 1, ANY, INT64_MAX, 10)


# ---- 10. the query service's call ----------------------------------------------------------------------
def test_query_service_call(gpu, make):
    """QueryService.getTraceIdsByAnnotation over span1, span4 and span5: trace 123 runs 1..20 (duration 19),
    trace 999 runs 5..8 (duration 3); 'custom' at limit 2 finds [123, 999]."""
    g = axref.golden()
    dec = SpanDecoder()
    cols, _, items = dec.decode_indexed(encode(axref.golden_spans(g, ["span1", "span4", "span5"])))
    idx = make(dec.num_services, services=dec.service_names())
    observe(idx, items)
    with TraceDurationIndex(device=gpu) as durations:
        durations.observe(cols)
        call = lambda a, v, order, limit=2: idx.getTraceIdsByAnnotationOrdered("service", a, v, 100, limit, order, durations)  # noqa: E731
        assert call("custom", None, None) == [123, 999]
        assert call("custom", b"", None) == [123, 999]  # an empty value is no value
        assert call("custom", None, None, limit=3) == [123, 999, 999]
        assert call("custom", None, "duration-asc") == [999, 123] == call("custom", None, "timestamp-desc")
        assert call("custom", None, "duration-desc") == [123, 999] == call("custom", None, "timestamp-asc")
        assert call("BAH2", b"BEH2", "duration-desc") == [999] and call("BAH2", b"BEH", None) == []
        assert call("cs", None, None) == []
        for bad in ("", b"", None):
            with pytest.raises(ValueError, match="No annotation provided"):
                call(bad, None, None)


# ---- 11. the query service over both indices -----------------------------------------------------------
def test_get_trace_ids_over_both_indices(gpu, make):
    web = Endpoint(1, 80, "web")
    spans = []
    for t in range(1, 61):
        ts = T0 + (t * 7919 % 50) * 1_000_000
        anns = [Annotation(ts, "sr", web), Annotation(ts + 900, "ss", web)]
        if t % 3 == 0:
            anns.append(Annotation(ts + 10, "retry", web))
        if t % 5 == 0:
            anns.append(Annotation(ts + 200_000_000, "late", web))
        bas = (BinaryAnnotation("http.uri", b"/a" if t % 8 else b"/b", "String", web),) if t % 4 == 0 else ()
        spans.append(Span(t, "get" if t % 2 else "put", 100 + t, None, tuple(anns), bas))
    spans.append(Span(1000, "lonely", 7, None, (Annotation(T0, "sr", web), Annotation(T0 + 1, "alone", web))))
    dec = SpanDecoder()
    cols, rejected, items = dec.decode_indexed(encode(spans), span_names=True)
    assert rejected == 0
    services, span_names = dec.service_names(), dec.span_names()
    S = len(services)
    names = TraceNameIndex(S, device=gpu, services=services, span_names=span_names)
    try:
        names.observe(DeviceColumns.from_host(cols))
        anns_idx = make(S, services=services)
        observe(anns_idx, items)
        ne = ixref.entries_of(cols, S)
        ae = items.rows()
        w = services.index("web")
        name_query = lambda n, e, l: ixref.trace_ids(ne, w, ixref.ANY if n is None else span_names.index(n) + 1, e, l)[0]  # noqa: E731
        ann_query = lambda a, v, e, l: axref.by_annotation(ae, w, a, v, e, l)  # noqa: E731
        end_ts = T0 + 45_000_000
        cases = [
            dict(),
            dict(annotation_list=["retry"]),
            dict(span_name="get", annotation_list=["retry"]),                                             # two slices
            dict(span_name="put", annotation_list=["retry"], binary_annotations=[("http.uri", b"/a")]),   # three
            dict(annotation_list=["retry"], binary_annotations=[("http.uri", b"/b")]),
            dict(span_name="get", annotation_list=["alone"]),                                             # an empty intersection
            dict(annotation_list=["retry", "late"]),
            dict(annotation_list=["absent", "nothing"]),
        ]
        seen = set()
        for case in cases:
            for limit in (2, 100):
                got, got_end = get_trace_ids(names, anns_idx, "web", end_ts=end_ts, limit=limit, **case)
                want, want_end = axref.get_trace_ids(name_query, ann_query, case.get("span_name"), case.get("annotation_list"),
                                                     case.get("binary_annotations"), end_ts, limit)
                assert [tuple(t) for t in got] == want and got_end == want_end, (case, limit)
                seen.add((len(case), bool(want)))
        assert {(2, True), (3, True), (2, False)} <= seen  # both outcomes of an intersection were exercised
    finally:
        names.close()
