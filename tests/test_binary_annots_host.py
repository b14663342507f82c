"""Binary annotations without a device: the C ABI of include/zkbinannots.h (NULL arguments refused before any device
is touched, the layout that makes zk_bn a facade over the annotation store's core, an empty store answering), and
Trace / TraceTimeline.of / with_annotations over hand-built traces with binary rows. No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from zipkin_amd import (BinaryAnnotation, BinaryAnnotationRows, Endpoint, TimeSkewAdjuster, Trace, TraceBinaryAnnotationStore,
                        TraceCombo, TraceSpanStore, TraceTimeline, ZkError, _abi)
from zipkin_amd.annotstore import row_bits
from zipkin_amd.binannotstore import BINARY_ROW_COLUMNS, binary_annotation_key, binary_row_bits
from zipkin_amd.ingest import hash_string

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "zkbinannots.h").read_text()
BAD = _abi.ZK_ERR_INVALID_ARG


# ---- the ABI -------------------------------------------------------------------------------------------------
def test_every_entry_point_refuses_null():
    L = _abi.lib()
    h, cfg = C.c_void_p(), _abi.zk_an_config()
    assert L.zk_bn_create(None, C.byref(h)) == BAD
    assert L.zk_bn_create(C.byref(cfg), None) == BAD
    assert L.zk_bn_destroy(None) == BAD
    assert L.zk_bn_last_error(None) == b"null handle"
    ab = BinaryAnnotationRows.empty(1).abi()
    assert L.zk_bn_observe(None, C.byref(ab), 1, 0) == BAD
    assert L.zk_bn_reset(None) == BAD
    assert L.zk_bn_compact(None) == BAD
    a = C.c_uint64()
    assert L.zk_bn_info(None, C.byref(a), C.byref(a), C.byref(a)) == BAD
    ids, counts = np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    assert L.zk_bn_gather(None, ids.ctypes.data, 4, 0, counts.ctypes.data_as(_abi._U32P), None, 0, C.byref(a)) == BAD
    out = (C.c_double * 3)()
    assert L.zk_bn_observe_ms(None, out) == BAD
    assert L.zk_bn_query_ms(None, C.cast(out, C.POINTER(C.c_double))) == BAD


def test_a_live_handle_refuses_null_arguments_and_bad_asks():
    L = _abi.lib()
    with TraceBinaryAnnotationStore() as store:  # (no device is opened: nothing below reaches one)
        h = store._h
        total, ids, counts = C.c_uint64(7), np.zeros(_abi.ZK_BN_MAX_IDS + 1, np.uint64), np.full(_abi.ZK_BN_MAX_IDS + 1, 9, np.uint32)
        cp = counts.ctypes.data_as(_abi._U32P)
        assert L.zk_bn_observe(h, None, 1, 0) == BAD and L.zk_bn_last_error(h) == b"null argument"
        rows = BinaryAnnotationRows.empty(2)
        for k, _ in BINARY_ROW_COLUMNS:
            ab = rows.abi()
            setattr(ab, k, None)
            assert L.zk_bn_observe(h, C.byref(ab), 2, 0) == BAD and L.zk_bn_last_error(h) == b"null column"
        ab = rows.abi()
        assert L.zk_bn_observe(h, C.byref(ab), 2, 2) == BAD  # ZK_BATCH_TRACE_CLUSTERED is no flag of this call
        assert L.zk_bn_observe(h, C.byref(ab), 2 ** 32, 0) == _abi.ZK_ERR_UNSUPPORTED
        assert L.zk_bn_observe(h, C.byref(ab), 0, 0) == _abi.ZK_OK
        assert L.zk_bn_gather(h, ids.ctypes.data, 4, 0, cp, None, 0, None) == BAD
        assert L.zk_bn_gather(h, None, 4, 0, cp, None, 0, C.byref(total)) == BAD
        assert L.zk_bn_gather(h, ids.ctypes.data, 4, 0, None, None, 0, C.byref(total)) == BAD
        assert L.zk_bn_gather(h, ids.ctypes.data, 4, 2, cp, None, 0, C.byref(total)) == BAD
        assert L.zk_bn_gather(h, ids.ctypes.data, 4, 0, cp, None, 1, C.byref(total)) == BAD  # cap without columns
        ab = rows.abi()
        ab.key = None
        assert L.zk_bn_gather(h, ids.ctypes.data, 4, 0, cp, C.byref(ab), 2, C.byref(total)) == BAD
        assert L.zk_bn_gather(h, ids.ctypes.data, len(ids), 0, cp, None, 0, C.byref(total)) == BAD
        assert total.value == 7 and (counts == 9).all()  # a refused ask writes nothing
        assert L.zk_bn_observe_ms(h, None) == BAD and L.zk_bn_query_ms(h, None) == BAD
        with pytest.raises(ZkError):
            store.observe_ms()
        with pytest.raises(ZkError):
            store.query_ms()


def test_an_empty_store_answers_without_a_device():
    with TraceBinaryAnnotationStore() as store:
        assert store.info() == {"entries": 0, "segments": 0, "bytes": 0}
        counts, rows = store.gather([0, 2 ** 64 - 1, 5, 5])
        assert counts.tolist() == [0, 0, 0, 0] and len(rows) == 0
        assert store.getBinaryAnnotationsByTraceIds([3, 4]) == [[], []]
        assert store.getBinaryAnnotationsByTraceIds([]) == []
        store.compact()
        store.reset()
        store.observe(BinaryAnnotationRows.empty(0))
        assert store.info()["entries"] == 0
    cfg = _abi.zk_an_config()
    cfg.device = -1
    assert _abi.lib().zk_bn_create(C.byref(cfg), C.byref(C.c_void_p())) == BAD
    cfg.device, cfg.expire_chunk = 0, 12345  # (ignored: there is no expiry)
    h = C.c_void_p()
    assert _abi.lib().zk_bn_create(C.byref(cfg), C.byref(h)) == _abi.ZK_OK and _abi.lib().zk_bn_destroy(h) == _abi.ZK_OK


def test_layouts_and_constants_are_the_headers():
    assert C.sizeof(_abi.zk_bn_cols) == C.sizeof(_abi.zk_an_cols) == 56
    an, bn = [f[0] for f in _abi.zk_an_cols._fields_], [f[0] for f in _abi.zk_bn_cols._fields_]
    assert bn == [k for k, _ in BINARY_ROW_COLUMNS] and [("ts" if k == "key" else k) for k in bn] == an
    for k in bn:
        assert getattr(_abi.zk_bn_cols, k).offset == getattr(_abi.zk_an_cols, "ts" if k == "key" else k).offset
    assert sum(np.dtype(dt).itemsize for _, dt in BINARY_ROW_COLUMNS) == _abi.ZK_BN_ROW_BYTES == 44
    for name, value in re.findall(r"#define (ZK_BN_\w+)\s+(\w+)", HEADER):
        want = getattr(_abi, value) if value.startswith("ZK_AN_") else int(value.rstrip("u"))
        assert getattr(_abi, name) == want, name
    assert "static_assert" in (ROOT / "zipkin_amd" / "csrc" / "zk_an.hip").read_text().split("zk_bn_create")[0].split("typed facade")[1]
    assert "zk_bn_expire" not in HEADER.split("#ifndef")[1] and not hasattr(_abi.lib(), "zk_bn_expire")
    # the bits word and the canonical order
    assert binary_row_bits(6, True, 0xFFFF) == 6 | 8 | 0xFFFF0000 and binary_row_bits(9, False) == 7 and binary_row_bits(-1, False) == 7
    assert binary_row_bits(3, True, 80) == row_bits(3, True, 80)
    rows = [(1, 2, 1 << 63, 5, 0, 0, 6), (1, 2, 1, 5, 0, 0, 6), (1, 2, 1, 5, 0, 0, 0), (1, 1, 2 ** 64 - 1, 9, 0, 0, 1), (1, 2, 1, 4, 0, 0, 6)]
    assert sorted(rows, key=binary_annotation_key) == [rows[3], rows[0], rows[2], rows[4], rows[1]]  # the key as a SIGNED value


# ---- Trace, TraceTimeline, with_annotations --------------------------------------------------------------------
TID = 9
K = {name: hash_string(name) for name in ("http.uri", "sql.query", "lost", "stray", "z")}
F_ANN = _abi.ZK_F_HAS_ANNOTATIONS | _abi.ZK_F_SVC_SERVER


def span_rows():
    """(trace_id, span_id, parent_id, first, last, service_id, flags): a root, its child, a span whose parent is missing"""
    P = _abi.ZK_F_HAS_PARENT
    return [(TID, 1, 0, 100, 200, 0, F_ANN), (TID, 2, 1, 110, 190, 1, F_ANN | P), (TID, 3, 999, 150, 150, 1, F_ANN | P)]


def annotation_rows():
    web, db = (0x0A000001, 0, row_bits(0, True, 80)), (0x0A000002, 1, row_bits(0, True, 3306))

    def row(sid, ts, text, kind, host):
        return (TID, sid, ts, hash_string(text), host[0], host[1], host[2] | kind)

    return [row(1, 100, "sr", 3, web), row(1, 200, "ss", 4, web), row(2, 110, "cs", 1, web), row(2, 190, "cr", 2, web),
            row(2, 1120, "sr", 3, db), row(2, 1180, "ss", 4, db), row(3, 150, "custom", 0, db)]


def binary_rows():
    h = binary_row_bits(6, True, 80)
    return [(TID, 2, K["sql.query"], hash_string(b"select 2"), 0x0A000002, 1, binary_row_bits(1, True, 3306)),
            (TID, 1, K["http.uri"], hash_string(b"/x"), 0x0A000001, 0, h),
            (TID, 2, K["sql.query"], hash_string(b"select 1"), 0x0A000002, 1, binary_row_bits(1, True, 3306)),
            (TID, 3, K["lost"], hash_string(b"gone"), 0, 0, binary_row_bits(6, False)),
            (TID, 424242, K["stray"], hash_string(b"v"), 0, 0, 6),  # a row of a span the trace has no record of
            (TID, 1, K["z"], hash_string(b""), 0, 0, binary_row_bits(0, False))]


def by_span(rows, order):
    return [BinaryAnnotation.of_row(r) for sid in order for r in sorted((r for r in rows if r[1] == sid), key=binary_annotation_key)]


def test_the_default_stays_empty():
    t = Trace(span_rows(), annotations=annotation_rows())
    assert t.binary_annotations is None and t.getBinaryAnnotations() == [] and t.getBinaryAnnotationsByKey(K["z"]) == []
    assert TraceTimeline.of(t).binary_annotations == []
    assert TimeSkewAdjuster.adjust(t).binary_annotations is None
    assert TraceCombo.of(t, TraceTimeline.of(t)).timeline.binary_annotations == []


@pytest.mark.parametrize("annotated", (False, True))
def test_a_trace_carries_its_binary_annotations_in_span_order(annotated):
    rng = np.random.default_rng(5)
    rows = binary_rows()
    t = Trace(span_rows(), annotations=annotation_rows() if annotated else None, binary=[rows[i] for i in rng.permutation(len(rows))])
    assert [s.id for s in t.spans] == [1, 2, 3]
    assert set(t.binary_annotations) == {1, 2, 3}  # the unknown span's row is ignored
    want = by_span(rows, [1, 2, 3])
    assert t.getBinaryAnnotations() == want and len(want) == 5
    assert [b.span_id for b in want] == [1, 1, 2, 2, 3] and want[-1].host is None and want[2].host == Endpoint(0x0A000002, 3306, 1)
    assert t.getBinaryAnnotationsByKey(K["sql.query"]) == [b for b in want if b.key == K["sql.query"]] and len(t.getBinaryAnnotationsByKey(K["sql.query"])) == 2
    assert t.getBinaryAnnotationsByKey(K["stray"]) == []
    assert want[2].type == 1 and {b.type for b in want} == {0, 1, 6}
    # attached after the trace is built: the same answer
    assert Trace(span_rows(), annotations=annotation_rows() if annotated else None).attach_binary(rows).getBinaryAnnotations() == want


def test_the_adjuster_prunes_a_span_and_its_binary_annotations():
    rows = binary_rows()
    t = Trace(span_rows(), annotations=annotation_rows(), binary=rows)
    adjusted = TimeSkewAdjuster.adjust(t)
    assert [s.id for s in adjusted.spans] == [1, 2]  # span 3's parent chain does not reach the root
    assert set(adjusted.binary_annotations) == {1, 2}
    assert adjusted.getBinaryAnnotations() == by_span(rows, [1, 2]) and len(adjusted.getBinaryAnnotations()) == 4
    assert t.getBinaryAnnotations() == by_span(rows, [1, 2, 3])  # the trace it came from is unchanged
    kept = t.with_annotations({2: t.annotations[2]})
    assert [s.id for s in kept.spans] == [2] and kept.getBinaryAnnotations() == by_span(rows, [2])


class Texts:
    """a decoder's string() and bytes() over a few known texts"""

    def __init__(self, *texts):
        self.t = {hash_string(x): (x.encode() if isinstance(x, str) else x) for x in texts}

    def bytes(self, h):
        return self.t[h]

    def string(self, h):
        return self.t[h].decode("utf-8", "surrogateescape")


def test_the_timeline_carries_them_resolved():
    rows = binary_rows()
    t = TimeSkewAdjuster.adjust(Trace(span_rows(), annotations=annotation_rows(), binary=rows))
    assert TraceTimeline.of(t).binary_annotations == by_span(rows, [1, 2])
    dec = Texts("http.uri", "sql.query", "z", b"/x", b"select 1", b"select 2", b"", "cs", "cr", "sr", "ss")
    line = TraceTimeline.of(t, dec, ["Web", "db"])
    got = [(b.key, b.value, b.type, b.host, b.span_id) for b in line.binary_annotations]
    one, two = sorted([b"select 1", b"select 2"], key=lambda v: hash_string(v))
    uri = ("http.uri", b"/x", 6, Endpoint(0x0A000001, 80, "Web"), 1)
    zed = ("z", b"", 0, None, 1)
    first = [uri, zed] if binary_annotation_key(rows[1]) < binary_annotation_key(rows[5]) else [zed, uri]
    assert got == first + [("sql.query", one, 1, Endpoint(0x0A000002, 3306, "db"), 2), ("sql.query", two, 1, Endpoint(0x0A000002, 3306, "db"), 2)]
    assert line.trace_id == TID and line.root_span_id == 1 and len(line.annotations) == 6
    with pytest.raises(ValueError):
        TraceTimeline.of(t, None, ["only one"])


class HostSpanStore(TraceSpanStore):
    """TraceSpanStore's query methods over a plain list of rows: no handle, no device."""

    def __init__(self, rows, services=None):
        self.rows, self.services, self.span_names, self._h = rows, services, None, None

    def getSpansByTraceIds(self, ids):
        return [list(self.rows) for i in ids if int(i) == TID]


class HostRows:
    def __init__(self, rows):
        self.rows = rows

    def getAnnotationsByTraceIds(self, ids):
        return [[r for r in self.rows if r[0] == int(i)] for i in ids]

    getBinaryAnnotationsByTraceIds = getAnnotationsByTraceIds


def test_the_by_id_calls_take_binary_on_the_host_path():
    sp, an, bn = HostSpanStore(span_rows(), ["Web", "db"]), HostRows(annotation_rows()), HostRows(binary_rows())
    rows = binary_rows()
    plain = sp.getTracesByIds([TID, 5], binary=bn)  # (no annotations= needed)
    assert len(plain) == 1 and plain[0].getBinaryAnnotations() == by_span(rows, [1, 2, 3])
    assert sp.getTracesByIds([TID])[0].binary_annotations is None
    adjusted = sp.getTracesByIds([TID], adjust=("TIME_SKEW",), annotations=an, binary=bn)
    assert adjusted[0].getBinaryAnnotations() == by_span(rows, [1, 2])
    lines = sp.getTraceTimelinesByIds([TID], adjust=("TIME_SKEW",), annotations=an, binary=bn)
    assert [(b.key, b.span_id) for b in lines[0].binary_annotations] == [(b.key, b.span_id) for b in by_span(rows, [1, 2])]
    assert lines[0].binary_annotations[-1].host == Endpoint(0x0A000002, 3306, "db")  # the service through the dictionary
    assert sp.getTraceTimelinesByIds([TID], adjust=("TIME_SKEW",), annotations=an)[0].binary_annotations == []
    combos = sp.getTraceCombosByIds([TID], adjust=("TIME_SKEW",), annotations=an, binary=bn)
    assert combos[0].trace.getBinaryAnnotations() == by_span(rows, [1, 2])
    assert combos[0].timeline.binary_annotations == lines[0].binary_annotations
    assert [tuple(a) for a in combos[0].timeline.annotations] == [tuple(a) for a in lines[0].annotations]
    bare = sp.getTraceCombosByIds([TID], binary=bn)
    assert bare[0].timeline is None and bare[0].trace.getBinaryAnnotations() == by_span(rows, [1, 2, 3])
