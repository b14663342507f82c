"""zk_an_adjusted_traces' C ABI (include/zkannots.h) and the argument checks of adjust_on_device= on
TraceSpanStore.getTraceCombosByIds, getTraceTimelinesByIds and getTracesByIds: the structs' layouts are the
header's, NULL handles and arguments and too many ids are refused before any device is touched, and the keyword
accepts TIME_SKEW, once, with an annotation store, and nothing else. No GPU.

A span store handle cannot be made without a device (zk_sp_create opens one), so the answer of an empty
annotation store beside an empty span store is checked in tests/test_gpu_annot_trace.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import tsaref as T
from tests.test_annot_adjust_abi import HostAnnotationStore, HostSpanStore
from zipkin_amd import AnnotationRows, TraceAnnotationStore, _abi
from zipkin_amd.columns import ADJUSTED_TRACE_HEAD, ADJUSTED_TRACE_SPAN
from zipkin_amd.spanstore import TRACE_HEAD, TRACE_SPAN

HEADER = (Path(__file__).resolve().parent.parent / "include" / "zkannots.h").read_text()
BAD = _abi.ZK_ERR_INVALID_ARG
SKEW = ("TIME_SKEW",)
C_TYPES = {"uint64_t": (C.c_uint64, np.uint64), "int64_t": (C.c_int64, np.int64), "uint32_t": (C.c_uint32, np.uint32)}


def header_fields(name):
    """[(field, C type name)] of `typedef struct name {...} name;` in the header."""
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(m.group(2), m.group(1)) for m in re.finditer(r"(\w+)\s+(\w+);", body)]


@pytest.mark.parametrize("name, struct, dtype, base", [("zk_an_trace", _abi.zk_an_trace, ADJUSTED_TRACE_HEAD, TRACE_HEAD),
                                                       ("zk_an_span", _abi.zk_an_span, ADJUSTED_TRACE_SPAN, TRACE_SPAN)])
def test_the_structs_are_the_headers(name, struct, dtype, base):
    fields = header_fields(name)
    assert [f for f, _ in fields] == [f for f, _ in struct._fields_] == list(dtype.names)
    at = 0
    for f, ctype in fields:  # natural alignment, no padding: the offsets are the running sum
        c, n = C_TYPES[ctype]
        assert dict(struct._fields_)[f] is c and dtype[f] == np.dtype(n)
        assert getattr(struct, f).offset == dtype.fields[f][1] == at
        at += C.sizeof(c)
    assert at == C.sizeof(struct) == dtype.itemsize == 56
    # zk_sp_trace's / zk_sp_span's fields come first, under the same names and at the same offsets
    assert dtype.names[:len(base.names)] == base.names
    assert all(dtype.fields[f][1] == base.fields[f][1] and dtype[f] == base[f] for f in base.names)


def test_the_symbol_and_the_state_bits():
    assert hasattr(_abi.lib(), "zk_an_adjusted_traces") and "zk_an_adjusted_traces" in _abi.SYMBOLS
    assert hasattr(TraceAnnotationStore, "adjusted_traces")
    bits = [_abi.ZK_SP_TR_FOUND, _abi.ZK_SP_TR_TIMED, _abi.ZK_SP_TR_OVERFLOW, _abi.ZK_AN_ADJ_ANNOTATED, _abi.ZK_AN_ADJ_OVERFLOW]
    assert all(b and b & (b - 1) == 0 for b in bits) and len(set(bits)) == 5


def test_null_arguments_and_too_many_ids_are_refused_without_a_device():
    L = _abi.lib()
    ids, heads = np.zeros(4, np.uint64), np.zeros(4, ADJUSTED_TRACE_HEAD)
    totals = (C.c_uint64 * 3)(7, 7, 7)
    # every check below answers before the span store's handle is used for more than its device ordinal, so
    # zeroed memory stands in for it
    fake = C.create_string_buffer(4096)
    sp = C.cast(fake, C.c_void_p)
    one_span, one_svc, one_row = np.zeros(1, ADJUSTED_TRACE_SPAN), np.zeros(1, np.uint32), AnnotationRows.empty(1)

    def call(an, sp_, ids_=ids.ctypes.data, n=4, flags=0, heads_=heads.ctypes.data, spans=None, cap_spans=0, svc=None, cap_svc=0,
             rows=None, cap_rows=0, totals_=totals):
        return L.zk_an_adjusted_traces(an, sp_, ids_, n, flags, heads_, spans, cap_spans, svc, cap_svc, rows, cap_rows, totals_)

    assert call(None, sp) == BAD
    with TraceAnnotationStore() as store:  # (no device is opened: nothing below reaches one)
        h = store._h
        assert call(h, None) == BAD and L.zk_an_last_error(h) == b"null argument"
        assert call(h, sp, totals_=None) == BAD
        assert call(h, sp, ids_=None) == BAD
        assert call(h, sp, heads_=None) == BAD
        assert call(h, sp, flags=2) == BAD and L.zk_an_last_error(h) == b"unknown flag"
        assert call(h, sp, cap_spans=1) == BAD and L.zk_an_last_error(h) == b"null output"
        assert call(h, sp, cap_svc=1) == BAD
        assert call(h, sp, cap_rows=1) == BAD and L.zk_an_last_error(h) == b"null output column"
        for k, _ in _abi.zk_an_cols._fields_:
            ab = one_row.abi()
            setattr(ab, k, None)
            assert call(h, sp, rows=C.byref(ab), cap_rows=1) == BAD
        many = np.zeros(_abi.ZK_AN_MAX_IDS + 1, np.uint64)
        many_heads = np.zeros(_abi.ZK_AN_MAX_IDS + 1, ADJUSTED_TRACE_HEAD)
        assert call(h, sp, ids_=many.ctypes.data, n=len(many), heads_=many_heads.ctypes.data) == BAD
        assert L.zk_an_last_error(h) == b"more than ZK_AN_MAX_IDS ids"
        assert list(totals) == [7, 7, 7] and not heads.view(np.uint8).any()  # nothing was written
        # n == 0 is ZK_OK, with or without outputs; the totals are set
        ab = one_row.abi()
        assert call(h, sp, ids_=None, n=0, heads_=None) == _abi.ZK_OK and list(totals) == [0, 0, 0]
        totals[:] = [7, 7, 7]
        assert call(h, sp, n=0, spans=one_span.ctypes.data, cap_spans=1, svc=one_svc.ctypes.data, cap_svc=1, rows=C.byref(ab),
                    cap_rows=1) == _abi.ZK_OK and list(totals) == [0, 0, 0]
        assert not one_span.view(np.uint8).any() and not one_svc.any() and not any(one_row.rows()[0])


# ---- adjust_on_device= on a handle-less store ------------------------------------------------------------------
class Recording(HostSpanStore):
    """What would go to the device is recorded instead: the three entry points share one device path."""

    def _combos_adjusted_on_device(self, ids, annotations, decoder=None, lists=True, timelines=True):
        self.asked.append(([int(i) for i in ids], annotations, decoder))
        return []


def stores():
    rows = [T.golden_rows(c) for c in T.golden()["cases"][:3]]
    return Recording([r for s, _ in rows for r in s]), HostAnnotationStore([r for _, a in rows for r in a])


def entry_points(spans):
    return (spans.getTraceCombosByIds, spans.getTraceTimelinesByIds, spans.getTracesByIds)


def test_adjust_on_device_takes_time_skew_once_with_an_annotation_store():
    spans, annots = stores()
    ids = sorted({r[0] for r in spans.model})
    for call in entry_points(spans):
        before = len(spans.asked)
        for adjust in (SKEW, "TIME_SKEW", ["TIME_SKEW"], ("NOTHING", "TIME_SKEW"), ("TIME_SKEW", "NOTHING", "NOTHING")):
            assert call(ids, adjust=adjust, annotations=annots, adjust_on_device=True) == []
        assert len(spans.asked) == before + 5 and all(a[:2] == (ids, annots) for a in spans.asked)
        for adjust in ((), ("NOTHING",), ("TIME_SKEW", "TIME_SKEW"), ("TIME_SKEW", "NOTHING", "TIME_SKEW"), ("SOMETHING",)):
            with pytest.raises(ValueError):
                call(ids, adjust=adjust, annotations=annots, adjust_on_device=True)
        with pytest.raises(ValueError):
            call(ids, adjust=SKEW, adjust_on_device=True)  # no annotation store
        with pytest.raises(ValueError):
            call(ids, adjust_on_device=True)
        assert len(spans.asked) == before + 5  # nothing refused reached the device
    with pytest.raises(ValueError):
        spans.getTraceCombosByIds(ids, on_device=True, adjust=SKEW, annotations=annots, adjust_on_device=True)
    # the timelines' decoder travels to the device path
    marker = object()
    spans.getTraceTimelinesByIds(ids, adjust=SKEW, annotations=annots, decoder=marker, adjust_on_device=True)
    assert spans.asked[-1][2] is marker


def test_every_existing_call_keeps_its_answer():
    spans, annots = stores()
    ids = sorted({r[0] for r in spans.model})
    with pytest.raises(ValueError):  # on_device=True with TIME_SKEW is still refused, not ignored
        spans.getTraceCombosByIds(ids, on_device=True, adjust=SKEW, annotations=annots)
    rows = {c["trace_id"]: T.golden_rows(c) for c in T.golden()["cases"][:3]}
    want = [T.adjust(T.annotated(*rows[i])) for i in ids]
    for off in ({}, {"adjust_on_device": False}):
        combos = spans.getTraceCombosByIds(ids, adjust=SKEW, annotations=annots, **off)
        traces = spans.getTracesByIds(ids, adjust=SKEW, annotations=annots, **off)
        lines = spans.getTraceTimelinesByIds(ids, adjust=SKEW, annotations=annots, **off)
        for i, c, t, ln, w in zip(ids, combos, traces, lines, want):
            assert {s.id: [tuple(a[:3]) + (None if a.host is None else tuple(a.host),) for a in s.annotations] for s in t.spans} == T.view(w)
            assert [s.id for s in c.trace.spans] == [s["id"] for s in w] and t.rows is not None
            assert (ln.trace_id, ln.root_span_id, [tuple(a) for a in ln.annotations]) == T.timeline(w, i)
            assert [tuple(a) for a in c.timeline.annotations] == T.timeline(w, i)[2]
    assert not spans.asked
