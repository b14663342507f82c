"""zk_an_adjusted_summaries' C ABI (include/zkannots.h) and the argument checks of adjust_on_device= on
TraceSpanStore.getTraceSummariesByIds: the symbol and the constants exist, NULL handles and arguments are refused
before any device is touched, and the keyword accepts TIME_SKEW, once, with an annotation store, and nothing
else. No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import zipkin_amd
from tests import anref as A
from tests import spref as R
from tests import tsaref as T
from zipkin_amd import TraceAnnotationStore, TraceSpanStore, _abi
from zipkin_amd.annotstore import ADJUSTED_ENTRY_COLUMNS, ADJUSTED_HEAD
from zipkin_amd.spanstore import ENTRY_COLUMNS, SUMMARY_HEAD

HEADER = (Path(__file__).resolve().parent.parent / "include" / "zkannots.h").read_text()
BAD = _abi.ZK_ERR_INVALID_ARG
SKEW = ("TIME_SKEW",)


def test_the_symbol_and_the_constants():
    assert hasattr(_abi.lib(), "zk_an_adjusted_summaries")
    for name in ("ZK_AN_ADJ_MAX_ROWS", "ZK_AN_ADJ_WAVE_ROWS", "ZK_AN_ADJ_ANNOTATED", "ZK_AN_ADJ_OVERFLOW"):
        m = re.search(rf"#define {name}\s+(\d+)u", HEADER)
        assert m and int(m.group(1)) == getattr(_abi, name), name
    rows = _abi.ZK_AN_ADJ_MAX_ROWS
    assert rows >= 1024 and rows & (rows - 1) == 0
    # the new state bits lie beside zk_sp_summaries' ones
    old = _abi.ZK_SP_SUM_FOUND | _abi.ZK_SP_SUM_TIMED | _abi.ZK_SP_SUM_OVERFLOW
    assert _abi.ZK_AN_ADJ_ANNOTATED & old == 0 and _abi.ZK_AN_ADJ_OVERFLOW & (old | _abi.ZK_AN_ADJ_ANNOTATED) == 0
    assert ADJUSTED_HEAD == SUMMARY_HEAD and ADJUSTED_HEAD.itemsize == C.sizeof(_abi.zk_sp_summary) == 40
    assert ADJUSTED_ENTRY_COLUMNS == ENTRY_COLUMNS
    assert (zipkin_amd.ADJ_ANNOTATED, zipkin_amd.ADJ_OVERFLOW) == (_abi.ZK_AN_ADJ_ANNOTATED, _abi.ZK_AN_ADJ_OVERFLOW)
    assert zipkin_amd.ADJUSTED_HEAD is ADJUSTED_HEAD and hasattr(TraceAnnotationStore, "adjusted_summaries")


def test_null_handles_and_arguments_are_refused_without_a_device():
    L = _abi.lib()
    ids, heads, total = np.zeros(4, np.uint64), np.zeros(4, SUMMARY_HEAD), C.c_uint64(7)
    # a span store cannot be made without a device; every check below answers before the handle is read, so
    # zeroed memory stands in for it
    fake = C.create_string_buffer(4096)
    sp = C.cast(fake, C.c_void_p)

    def call(an, sp_, ids_=ids.ctypes.data, n=4, flags=0, heads_=heads.ctypes.data, out=None, cap=0, n_out=C.byref(total)):
        return L.zk_an_adjusted_summaries(an, sp_, ids_, n, flags, heads_, out, cap, n_out)

    assert call(None, sp) == BAD
    with TraceAnnotationStore() as store:  # (no device is opened: nothing below reaches one)
        h = store._h
        assert call(h, None) == BAD and L.zk_an_last_error(h) == b"null argument"
        assert call(h, sp, n_out=None) == BAD
        assert call(h, sp, ids_=None) == BAD
        assert call(h, sp, heads_=None) == BAD
        assert call(h, sp, flags=2) == BAD and L.zk_an_last_error(h) == b"unknown flag"
        assert call(h, sp, cap=1) == BAD and L.zk_an_last_error(h) == b"null output column"
        for k, _ in ENTRY_COLUMNS:
            cols = {c: np.zeros(1, dt) for c, dt in ENTRY_COLUMNS}
            out = _abi.zk_sp_span_ts(*[cols[c].ctypes.data for c, _ in ENTRY_COLUMNS])
            setattr(out, k, None)
            assert call(h, sp, out=C.byref(out), cap=1) == BAD
        many = np.zeros(_abi.ZK_AN_MAX_IDS + 1, np.uint64)
        many_heads = np.zeros(_abi.ZK_AN_MAX_IDS + 1, SUMMARY_HEAD)
        assert call(h, sp, ids_=many.ctypes.data, n=len(many), heads_=many_heads.ctypes.data) == BAD
        assert L.zk_an_last_error(h) == b"more than ZK_AN_MAX_IDS ids"
        assert total.value == 7 and not heads.view(np.uint8).any()  # nothing was written


# ---- adjust_on_device= on a handle-less store ------------------------------------------------------------------
class HostSpanStore(TraceSpanStore):
    """TraceSpanStore's query methods over a plain list of rows: no handle, no device. What would go to the
    device is recorded instead."""

    def __init__(self, model):
        self.model, self.services, self.span_names, self._h = model, None, None, None
        self.asked = []

    def getSpansByTraceIds(self, ids):
        return R.spans_by_trace_ids(self.model, [int(i) for i in ids])

    def _summaries_adjusted_on_device(self, ids, annotations):
        self.asked.append((ids.tolist(), annotations))
        return "device"


class HostAnnotationStore:
    def __init__(self, model):
        self.model = model

    def getAnnotationsByTraceIds(self, ids):
        return A.by_trace_ids(self.model, [int(i) for i in ids])


def stores():
    rows = [T.golden_rows(c) for c in T.golden()["cases"][:3]]
    return HostSpanStore([r for s, _ in rows for r in s]), HostAnnotationStore([r for _, a in rows for r in a])


def test_adjust_on_device_takes_time_skew_once_with_an_annotation_store():
    spans, annots = stores()
    ids = sorted({r[0] for r in spans.model})
    for adjust in (SKEW, "TIME_SKEW", ["TIME_SKEW"], ("NOTHING", "TIME_SKEW"), ("TIME_SKEW", "NOTHING", "NOTHING")):
        assert spans.getTraceSummariesByIds(ids, adjust=adjust, annotations=annots, adjust_on_device=True) == "device"
    assert all(a == (ids, annots) for a in spans.asked) and len(spans.asked) == 5
    for adjust in ((), ("NOTHING",), ("TIME_SKEW", "TIME_SKEW"), ("TIME_SKEW", "NOTHING", "TIME_SKEW")):
        with pytest.raises(ValueError):
            spans.getTraceSummariesByIds(ids, adjust=adjust, annotations=annots, adjust_on_device=True)
    with pytest.raises(ValueError):
        spans.getTraceSummariesByIds(ids, adjust=("SOMETHING",), annotations=annots, adjust_on_device=True)
    with pytest.raises(ValueError):
        spans.getTraceSummariesByIds(ids, adjust=SKEW, adjust_on_device=True)  # no annotation store
    with pytest.raises(ValueError):
        spans.getTraceSummariesByIds(ids, adjust_on_device=True)
    with pytest.raises(ValueError):
        spans.getTraceSummariesByIds(ids, on_device=True, adjust=SKEW, annotations=annots, adjust_on_device=True)
    assert len(spans.asked) == 5  # nothing refused reached the device


def test_every_existing_call_keeps_its_answer():
    spans, annots = stores()
    ids = sorted({r[0] for r in spans.model})
    # on_device=True with TIME_SKEW is still refused, not ignored
    for call in (spans.getTraceSummariesByIds, spans.getTraceCombosByIds):
        with pytest.raises(ValueError):
            call(ids, on_device=True, adjust=SKEW, annotations=annots)
    # without the keyword, and with it False, the host path answers as before
    host = spans.getTraceSummariesByIds(ids, adjust=SKEW, annotations=annots)
    assert host == spans.getTraceSummariesByIds(ids, adjust=SKEW, annotations=annots, adjust_on_device=False) and not spans.asked
    rows = {c["trace_id"]: T.golden_rows(c) for c in T.golden()["cases"][:3]}
    assert [(s.trace_id, s.start, s.end, s.duration_micro, [tuple(x) for x in s.span_timestamps], s.endpoints) for s in host] == \
        [T.summary(T.adjust(T.annotated(*rows[i])), i) for i in ids]
