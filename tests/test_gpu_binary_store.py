"""The binary-annotation store (zkbinannots.h, TraceBinaryAnnotationStore) against a Python multiset reference, and
the three trace calls with binary= on the host path, on_device=True and adjust_on_device=True, fed from stored
bytes that never leave the device (observe_stored(spans=, binary=)). Every comparison is exact equality."""
import random

import numpy as np
import pytest

from oracle.spans import Annotation, BinaryAnnotation, Endpoint, Span
from tests import binref as B
from tests.test_gpu_ingest_rows import upload
from zipkin_amd import _abi
from zipkin_amd.binannotstore import (BinaryAnnotationRows, DeviceBinaryAnnotationRows, TraceBinaryAnnotationStore,
                                      binary_annotation_key, binary_row_bits)
from zipkin_amd.ingest import SpanDecoder, hash_string

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1


def random_rows(seed, n, tids):
    rnd = random.Random(seed)
    keys = [rnd.getrandbits(64) for _ in range(6)] + [0, U64, 1 << 63]
    return [(rnd.choice(tids), rnd.getrandbits(3), rnd.choice(keys), rnd.getrandbits(2), rnd.getrandbits(32) if rnd.random() < .5 else 0,
             rnd.getrandbits(4), binary_row_bits(rnd.randrange(8), rnd.random() < .5, rnd.getrandbits(16)) | (rnd.getrandbits(12) << 4 if rnd.random() < .1 else 0))
            for _ in range(n)]


def reference(rows, ids):
    return [sorted((r for r in rows if r[0] == i), key=binary_annotation_key) for i in ids]


def test_observe_gather_compact_against_a_multiset(gpu):
    tids = [0, U64, 5, 6, 1 << 63, 12345678901234567]
    batches = [random_rows(500 + k, n, tids) for k, n in enumerate((1, 257, 4097, 64))]
    ask = [U64, 0, 5, 404, 5, 1 << 63]  # an id twice, one the store lacks
    with TraceBinaryAnnotationStore(device=gpu, timing=True) as st:
        assert st.info() == {"entries": 0, "segments": 0, "bytes": 0}
        seen = []
        for k, rows in enumerate(batches):
            host = BinaryAnnotationRows.of_rows(rows)
            st.observe(DeviceBinaryAnnotationRows.from_host(host, gpu) if k % 2 else host)
            seen += rows
            assert st.getBinaryAnnotationsByTraceIds(ask) == reference(seen, ask)
        assert set(st.observe_ms()) == {"count", "size", "scatter"} and st.query_ms() >= 0.0
        assert st.info()["entries"] == len(seen) and st.info()["segments"] == 4
        st.observe(BinaryAnnotationRows.of_rows(batches[1]))  # a batch again is added again
        seen += batches[1]
        st.compact()
        assert st.info()["segments"] == 1 and st.info()["entries"] == len(seen)
        assert st.getBinaryAnnotationsByTraceIds(ask) == reference(seen, ask)
        counts, got = st.gather(np.array(ask, np.uint64))
        assert counts.tolist() == [len(r) for r in reference(seen, ask)] and len(got) == int(counts.sum())
        st.reset()
        assert st.info()["entries"] == 0 and st.getBinaryAnnotationsByTraceIds(ask) == [[] for _ in ask]


def test_sixty_five_tiny_observes_cross_the_segment_bound(gpu):
    tids = [0, U64, 9]
    with TraceBinaryAnnotationStore(device=gpu) as st:
        seen = []
        for k in range(_abi.ZK_BN_MAX_SEGMENTS + 1):
            rows = random_rows(600 + k, 3, tids)
            st.observe(BinaryAnnotationRows.of_rows(rows), sync=False)
            seen += rows
            if k == _abi.ZK_BN_MAX_SEGMENTS - 1:
                assert st.info()["segments"] == _abi.ZK_BN_MAX_SEGMENTS
        assert st.info() == dict(st.info(), entries=len(seen), segments=2)  # the 65th observe merged the 64 first
        assert st.getBinaryAnnotationsByTraceIds(tids) == reference(seen, tids)


# ---- end to end ---------------------------------------------------------------------------------------------
WEB, DB = Endpoint(0x0A000001, 80, "Web"), Endpoint(0x0A000002, 3306, "db")
T1 = 77


def hand_trace():
    """A root (1), its child (2, in two fragments, the second without time annotations), and a span (3) whose
    parent the trace lacks: the time-skew adjuster prunes it, and its binary annotations leave with it."""
    return [
        Span(T1, "get", 1, None, (Annotation(100, "sr", WEB), Annotation(200, "ss", WEB)),
             (BinaryAnnotation("http.uri", b"/x?y", "String", WEB), BinaryAnnotation("http.status", b"\x00\xc8", "I16", WEB))),
        Span(T1, "query", 2, 1, (Annotation(110, "cs", WEB), Annotation(190, "cr", WEB), Annotation(1120, "sr", DB), Annotation(1180, "ss", DB)),
             (BinaryAnnotation("sql.query", b"select\0\xff 1", "BYTES", DB),)),
        Span(T1, "query", 2, 1, (), (BinaryAnnotation("rows", b"\0\0\0\x07", "I32", None), BinaryAnnotation("sql.query", b"select 2", "String", DB))),
        Span(T1, "lost", 3, 999, (Annotation(150, "custom", DB),), (BinaryAnnotation("lost.key", b"gone", "String", DB),)),
    ]


def expect_binaries(spans, span_order):
    """[(key text, value bytes, type, (ipv4, port, name) or None, span_id)]: the spans in span_order, each span's rows
    in canonical order (here: by the key's hash as a signed value, then type, then the value's hash)."""
    rows = B.expected_binary_rows(spans)
    texts = B.strings_of(spans)
    out = []
    for sid in span_order:
        mine = sorted((r for r in rows if r[1] == sid), key=lambda r: (r[2] - (1 << 64) if r[2] >> 63 else r[2], r[6] & 7, r[3]))
        out += [(texts[r[2]].decode(), texts[r[3]], r[6] & 7, (r[4], r[6] >> 16, r[5]) if r[6] & 8 else None, sid) for r in mine]
    return out


def flat(binaries):
    return [(b.key, b.value, b.type, None if b.host is None else tuple(b.host), b.span_id) for b in binaries]


def test_trace_calls_with_binary_on_all_three_paths(gpu):
    from zipkin_amd import TraceAnnotationStore, TraceSpanStore
    from zipkin_amd.ingest import DeviceSpanDecoder
    from zipkin_amd.spanstore import resolve_binary

    hand = hand_trace()
    frags = [B.Frag(s) for s in hand] + B.gen_frags(700, 120, traces=10)
    blobs = B.encode_all(frags)
    ids = [T1] + sorted({f.span.trace_id & U64 for f in frags} - {T1}) + [T1, 31337]  # an id twice, one the stores lack
    dd = DeviceSpanDecoder(64)
    with TraceAnnotationStore(device=gpu) as an, TraceSpanStore(device=gpu) as sp, TraceBinaryAnnotationStore(device=gpu) as bn:
        total = 0
        for part in (blobs[:50], blobs[50:]):
            buf, off, n = upload(part)
            cols, rej, m = an.observe_stored(dd, buf, off, n, spans=sp, binary=bn)
            assert rej == 0 and cols.n == n and bn._held is not None and bn._held.key.is_cuda
            total += len(bn._held)
        assert bn.info()["entries"] == total == len(B.expected_binary_rows(frags)) and bn._held is None
        # a row of a span the trace has no record of is ignored by every call
        bn.observe(BinaryAnnotationRows.of_rows([(T1, 424242, hash_string("stray"), hash_string("v"), 0, 0, 6)]))
        sp.services = dd.service_names()
        names = dd.service_names()

        def resolved(trace):
            return flat(resolve_binary(trace.getBinaryAnnotations(), dd, names))

        # -- without an adjuster: host path and on_device=True, all three spans of the hand-built trace
        host = sp.getTracesByIds(ids, binary=bn)
        dev = [c.trace for c in sp.getTraceCombosByIds(ids, on_device=True, binary=bn)]
        plain = [c.trace for c in sp.getTraceCombosByIds(ids, binary=bn)]
        assert len(host) == len(dev) == len(plain) == len(ids) - 1
        assert [t.id for t in host] == [t.id for t in dev] == ids[:-1]
        for a, b, c in zip(host, dev, plain):
            assert [s.id for s in a.spans] == [s.id for s in b.spans]
            assert resolved(a) == resolved(b) == resolved(c)
            assert set(a.binary_annotations) == {s.id for s in a.spans}
        assert resolved(host[0]) == expect_binaries(hand, [1, 2, 3]) and len(resolved(host[0])) == 6
        assert resolved(host[-1]) == resolved(host[0])  # the id asked twice
        assert sum(len(resolved(t)) for t in host) >= 300
        assert [flat(t.getBinaryAnnotationsByKey(hash_string("sql.query"))) for t in host[:1]] == \
            [[x for x in flat(host[0].getBinaryAnnotations()) if x[0] == hash_string("sql.query")]]
        assert len(host[0].getBinaryAnnotationsByKey(hash_string("sql.query"))) == 2
        # without binary= nothing changes
        assert all(t.binary_annotations is None and t.getBinaryAnnotations() == [] for t in sp.getTracesByIds(ids))

        # -- with the time-skew adjuster: host path and adjust_on_device=True; span 3 is pruned
        kw = dict(adjust=("TIME_SKEW",), annotations=an, binary=bn, decoder=dd)
        combos_h = sp.getTraceCombosByIds(ids, **kw)
        combos_d = sp.getTraceCombosByIds(ids, adjust_on_device=True, **kw)
        lines_h = sp.getTraceTimelinesByIds(ids, **kw)
        lines_d = sp.getTraceTimelinesByIds(ids, adjust_on_device=True, **kw)
        traces_d = sp.getTracesByIds(ids, adjust=("TIME_SKEW",), annotations=an, adjust_on_device=True, binary=bn)
        assert len(combos_h) == len(combos_d) == len(traces_d) == len(ids) - 1
        for h, d, t in zip(combos_h, combos_d, traces_d):
            assert [s.id for s in h.trace.spans] == [s.id for s in d.trace.spans] == [s.id for s in t.spans]
            assert resolved(h.trace) == resolved(d.trace) == resolved(t)
            assert (h.timeline is None) == (d.timeline is None)
            if h.timeline is not None:
                assert flat(h.timeline.binary_annotations) == flat(d.timeline.binary_annotations) == resolved(h.trace)
                assert [tuple(a) for a in h.timeline.annotations] == [tuple(a) for a in d.timeline.annotations]
        assert [s.id for s in combos_h[0].trace.spans] == [1, 2]
        want = expect_binaries(hand, [1, 2])
        assert resolved(combos_h[0].trace) == want and len(want) == 5
        assert flat(combos_d[0].timeline.binary_annotations) == want
        assert [flat(t.binary_annotations) for t in lines_h] == [flat(t.binary_annotations) for t in lines_d]
        assert [flat(t.binary_annotations) for t in lines_h] == [flat(c.timeline.binary_annotations) for c in combos_h if c.timeline is not None]
        assert lines_h[0].binary_annotations[0].host.service_id in ("Web", "db")
        # timelines without binary= keep the empty fourth field
        assert all(t.binary_annotations == [] for t in sp.getTraceTimelinesByIds(ids, adjust=("TIME_SKEW",), annotations=an, decoder=dd))
