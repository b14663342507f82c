"""What zk_an_adjusted_traces (include/zkannots.h) must answer, derived from tests/tsaref.py's spans: the raw
heads, 56-B spans, services and row columns of an asked trace. The adjuster is tsaref's, unchanged; the depths
are restated here from the rule (root-most span at 1, level by level down the children, a span reached twice
keeps its first depth). Nothing of zipkin_amd's Trace, TimeSkewAdjuster or TraceTimeline is imported."""
import ctypes as C

import numpy as np

from tests import anref as A
from tests import spref as S
from tests import tsaref as T
from zipkin_amd import AnnotationRows, DeviceAnnotationRows, DeviceColumns, _abi
from zipkin_amd.columns import ADJUSTED_TRACE_HEAD, ADJUSTED_TRACE_SPAN

FOUND, TIMED, TR_OVERFLOW = _abi.ZK_SP_TR_FOUND, _abi.ZK_SP_TR_TIMED, _abi.ZK_SP_TR_OVERFLOW
ANNOTATED, OVERFLOW = _abi.ZK_AN_ADJ_ANNOTATED, _abi.ZK_AN_ADJ_OVERFLOW
MAX_ROWS, MAX_FRAGMENTS, WAVE = _abi.ZK_AN_ADJ_MAX_ROWS, _abi.ZK_SP_TRACE_MAX_ROWS, _abi.ZK_AN_ADJ_WAVE_ROWS
B_HAS_PARENT, B_TIMED = _abi.ZK_SP_SPAN_HAS_PARENT, _abi.ZK_SP_SPAN_TIMED
B_PARENT_FOUND, B_ROOT_MOST = _abi.ZK_SP_SPAN_PARENT_FOUND, _abi.ZK_SP_SPAN_ROOT_MOST
SENTINEL = 0xA5
ZERO_HEAD = (0,) * 10


def depths(spans, root):
    """span id -> depth under `root` (depth 1), over spans in their order."""
    kids = {}
    for s in spans:
        if s["parent"] is not None:
            kids.setdefault(s["parent"], []).append(s)
    out, level, d = {}, [root], 1
    while level:
        nxt = []
        for s in level:
            if s["id"] not in out:
                out[s["id"]] = d
                nxt += kids.get(s["id"], [])
        level, d = nxt, d + 1
    return out


def expect(tid, span_rows, ann_rows):
    """(head, spans, services, rows) of one found trace as tuples and lists of tuples, the raw call's fields
    in the structs' order."""
    if len(span_rows) > MAX_FRAGMENTS or len(ann_rows) > MAX_ROWS:
        state, start, end = FOUND | OVERFLOW, 0, 0
        if ann_rows:
            state |= ANNOTATED
        else:
            se = S.start_end(span_rows)
            state |= TR_OVERFLOW | (TIMED if se else 0)
            start, end = se or (0, 0)
        return (tid, start, end, 0, len(span_rows), 0, 0, state, 0, 0), [], [], []
    model = T.annotated(span_rows, ann_rows)
    adjusted = T.adjust(model) if ann_rows else model  # a trace without rows in the annotation store is not adjusted
    own = {s["id"]: len(s["ann"]) for s in model}
    root = T.root_most(adjusted)
    depth = depths(adjusted, root)
    ids = {s["id"] for s in adjusted}
    stored = sorted(ann_rows, key=A.key)
    spans, services, rows = [], [], []
    for s in adjusted:
        injected = len(s["ann"]) - own[s["id"]]
        assert injected in (0, 2)
        bits = (B_HAS_PARENT if s["parent"] is not None else 0) | (B_TIMED if s["first"] is not None else 0) | \
            (B_PARENT_FOUND if s["parent"] is not None and s["parent"] in ids else 0) | (B_ROOT_MOST if s is root else 0)
        spans.append((s["id"], s["parent"] or 0, s["first"] or 0, s["last"] or 0, s["name"], depth.get(s["id"], 0), len(s["services"]),
                      bits, len(s["ann"]), injected))
        services += s["services"]
        mine = [r for r in stored if r[1] == s["id"]]
        assert len(mine) == own[s["id"]]
        for k, (ts, value, kind, host) in enumerate(s["ann"]):
            if k < len(mine):  # a stored row: only its ts may have moved
                r = mine[k]
                assert (value, kind) == (r[3], r[6] & A.KIND_MASK)
                rows.append((tid, s["id"], ts, r[3], r[4], r[5], r[6]))
            elif host is None:
                rows.append((tid, s["id"], ts, value, 0, 0, kind))
            else:
                rows.append((tid, s["id"], ts, value, host[0], host[2], kind | A.HAS_HOST | (host[1] << A.PORT_SHIFT)))
    timed = [s for s in adjusted if s["first"] is not None]
    start, end = (min(s["first"] for s in timed), max(s["last"] for s in timed)) if timed else (0, 0)
    state = FOUND | (TIMED if timed else 0) | (ANNOTATED if ann_rows else 0)
    return (tid, start, end, root["id"], len(span_rows), len(spans), len(services), state, len(rows), 0), spans, services, rows


class World:
    """Traces as (span rows, annotation rows) by trace id, fed to both stores shuffled, in `parts` observes each."""

    def __init__(self, traces=None):
        self.traces, self._expected = dict(traces or {}), {}

    def add(self, tid, span_rows, ann_rows):
        assert tid not in self.traces
        self.traces[tid] = (list(span_rows), list(ann_rows))

    def add_case(self, case):
        self.add(case["trace_id"], *T.golden_rows(case))

    def feed(self, spans, annots, seed=1, parts=3):
        span_rows = [r for s, _ in self.traces.values() for r in s]
        ann_rows = [r for _, a in self.traces.values() for r in a]
        rng = np.random.default_rng(seed)
        for part in np.array_split(rng.permutation(len(span_rows)), parts):
            spans.observe(DeviceColumns.from_host(S.cols_of([span_rows[i] for i in part])))
        for part in np.array_split(rng.permutation(len(ann_rows)), parts):
            if len(part):
                annots.observe(DeviceAnnotationRows.from_host(AnnotationRows.of_rows([ann_rows[i] for i in part]), annots.device))

    def expect(self, tid):
        if tid not in self.traces:
            return ZERO_HEAD, [], [], []
        if tid not in self._expected:
            self._expected[tid] = expect(tid, *self.traces[tid])
        return self._expected[tid]


def answers(heads, spans, services, rows):
    """The raw call's answer per asked id: [(head, spans, services, rows)] as expect() has them."""
    sp, sv, rw = spans.tolist(), services.tolist(), rows.rows()
    out, a, b, c = [], 0, 0, 0
    for h in heads.tolist():
        out.append((tuple(h), sp[a:a + h[5]], sv[b:b + h[6]], rw[c:c + h[8]]))
        a, b, c = a + h[5], b + h[6], c + h[8]
    assert (a, b, c) == (len(sp), len(sv), len(rw))
    return out


def raw(annots, spans, ids, caps, flags=0, ptr=None):
    """zk_an_adjusted_traces into sentinel-filled outputs of caps = (spans, services, rows) entries:
    (status, totals, heads, spans, services, rows)."""
    ids = np.ascontiguousarray(np.asarray(ids, np.uint64))

    def filled(n, dt):
        return np.frombuffer(bytes([SENTINEL]) * (max(n, 1) * np.dtype(dt).itemsize), dt).copy()

    heads = filled(len(ids), ADJUSTED_TRACE_HEAD)
    o_spans, o_svc = filled(caps[0], ADJUSTED_TRACE_SPAN), filled(caps[1], np.uint32)
    o_rows = AnnotationRows(*[filled(caps[2], dt) for dt in A.DTYPES])
    ab = o_rows.abi()
    totals = (C.c_uint64 * 3)(12345, 12345, 12345)
    st = annots._L.zk_an_adjusted_traces(annots._h, spans._h, ids.ctypes.data if ptr is None else ptr, len(ids), flags, heads.ctypes.data,
                                         o_spans.ctypes.data, caps[0], o_svc.ctypes.data, caps[1], C.byref(ab), caps[2], totals)
    return st, tuple(totals), heads[:len(ids)], o_spans, o_svc, o_rows
