"""The time-skew adjuster and the trace timeline on the host (zipkin_amd/spanstore.py), before any device runs:
the product classes against the hand-worked vectors (tests/golden/time_skew.json) and against the independent
restatement tests/tsaref.py on seeded random traces. Every comparison is exact equality. No GPU."""
import numpy as np
import pytest

from tests import anref as A
from tests import spref as R
from tests import tsaref as T
from zipkin_amd import (AnnotatedSpan, Span, TimeSkewAdjuster, Trace, TraceCombo, TraceSpanStore, TraceSummary,
                        TraceTimeline)

G = T.golden()
TEXT = {T.fnv_mix(t.encode()): t for t in ("cs", "cr", "sr", "ss", "foo", "bar", "x")}
SKEW = ("TIME_SKEW",)


def product_view(trace):
    return {s.id: [(a.ts, a.value, a.kind, None if a.host is None else tuple(a.host)) for a in s.annotations] for s in trace.spans}


def summary_tuple(s):
    return None if s is None else (s.trace_id, s.start, s.end, s.duration_micro, [tuple(x) for x in s.span_timestamps], s.endpoints)


def timeline_tuple(t):
    return None if t is None else (t.trace_id, t.root_span_id, [tuple(a) for a in t.annotations])


class HostSpanStore(TraceSpanStore):
    """TraceSpanStore's query methods over a plain list of rows: no handle, no device."""

    def __init__(self, model, services=None):
        self.model, self.services, self.span_names, self._h = model, services, None, None

    def getSpansByTraceIds(self, ids):
        return R.spans_by_trace_ids(self.model, [int(i) for i in ids])


class HostAnnotationStore:
    def __init__(self, model):
        self.model = model

    def getAnnotationsByTraceIds(self, ids):
        return A.by_trace_ids(self.model, [int(i) for i in ids])


# ---- the hand-worked vectors ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G["cases"], ids=lambda c: c["name"])
def test_golden_vectors(case):
    spans, anns = T.golden_rows(case)
    e, tid = case["expect"], case["trace_id"]
    rng = np.random.default_rng(tid)
    trace = Trace([spans[i] for i in rng.permutation(len(spans))], annotations=[anns[i] for i in rng.permutation(len(anns))])
    assert all(isinstance(s, AnnotatedSpan) and isinstance(s, Span) for s in trace.spans)
    for adjusted, model in ((TimeSkewAdjuster.adjust(trace), T.adjust(T.annotated(spans, anns))),):
        want = {int(k): [tuple(a) for a in v] for k, v in e["annotations"].items()}
        assert {k: [(a[0], TEXT[a[1]]) for a in v] for k, v in product_view(adjusted).items()} == want
        assert {k: [(a[0], TEXT[a[1]]) for a in v] for k, v in T.view(model).items()} == want
        assert [s.id for s in adjusted.spans] == e["span_order"] == [s["id"] for s in model]
        se = adjusted.getStartAndEndTimestamp()
        assert list(se) == e["start_end"]
        sm = TraceSummary.of(adjusted)
        assert (sm.trace_id, sm.start, sm.end, sm.duration_micro) == (tid, e["start_end"][0], e["start_end"][1], e["duration_micro"])
        assert summary_tuple(sm) == T.summary(model, tid)
        tl = TraceTimeline.of(adjusted)
        assert (tl.trace_id, tl.root_span_id, tl.binary_annotations) == (tid, e["root_span_id"], [])
        assert [(a.ts, TEXT[a.value], a.span_id) for a in tl.annotations] == [tuple(x) for x in e["timeline"]]
        assert timeline_tuple(tl) == T.timeline(model, tid)
    # injected annotations carry the endpoint of the first child's first cs / cr
    if case["name"] == "client_only_with_a_child_injection_and_manual_shift":
        adjusted = TimeSkewAdjuster.adjust(trace)
        assert [a.host for a in adjusted.getSpanById(1).annotations[2:]] == [(G["hosts"]["B"], 80, G["hosts"]["B"] & 0xFF)] * 2
        assert [a.kind for a in adjusted.getSpanById(1).annotations] == [A.CS, A.CR, A.SR, A.SS]


def test_the_truncating_division_differs_from_floor():
    case = next(c for c in G["cases"] if c["name"] == "odd_negative_difference_through_wrap_around")
    a = {x[1]: x[0] for x in case["spans"][0]["annotations"]}
    endpoint = (G["hosts"]["B"], 80, 2)
    got = TimeSkewAdjuster.skew(a["cs"], a["cr"], a["sr"], a["ss"], endpoint)
    assert got == (endpoint, 2 ** 62 - 4) == T.skew_of(a["cs"], a["cr"], a["sr"], a["ss"], endpoint)
    cd_sd = T.jlong(T.jlong(a["cr"] - a["cs"]) - T.jlong(a["ss"] - a["sr"]))
    assert cd_sd == -2 ** 63 + 9 and cd_sd // 2 != T.jhalf(cd_sd) == -2 ** 62 + 5


# ---- seeded random traces ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_random_traces_against_the_restatement(seed):
    rng = np.random.default_rng(1000 + seed)
    case = T.random_case(rng, 2 ** 64 - 1 - seed if seed % 2 else seed)
    spans, anns = T.golden_rows(case)
    tid = case["trace_id"]
    trace = Trace(spans, annotations=anns)
    model = T.annotated(spans, anns)
    assert product_view(trace) == T.view(model) and [s.id for s in trace.spans] == [s["id"] for s in model]
    for adjust in ((), ("NOTHING",), SKEW, ("TIME_SKEW", "TIME_SKEW"), ("NOTHING", "TIME_SKEW")):
        got = trace
        for name in adjust:
            got = {"NOTHING": lambda t: t, "TIME_SKEW": TimeSkewAdjuster.adjust}[name](got)
        want = T.fold(model, adjust)
        assert product_view(got) == T.view(want)
        assert [(s.id, s.parent, s.first, s.last, list(s.services)) for s in got.spans] == \
            [(s["id"], s["parent"], s["first"], s["last"], s["services"]) for s in want]
        assert summary_tuple(TraceSummary.of(got)) == T.summary(want, tid)
        assert timeline_tuple(TraceTimeline.of(got)) == T.timeline(want, tid)
    assert product_view(trace) == T.view(model)  # the adjuster leaves its input as it was


def test_some_random_trace_is_adjusted_in_both_directions():
    """The generator reaches what it is meant to reach: positive and negative skews, injection, dropped spans."""
    signs, injected, dropped = set(), 0, 0
    for seed in range(40):
        case = T.random_case(np.random.default_rng(1000 + seed), seed)
        spans, anns = T.golden_rows(case)
        before, after = T.annotated(spans, anns), T.adjust(T.annotated(spans, anns))
        b = T.view(before)
        for sid, lst in T.view(after).items():
            signs |= {np.sign(x[0] - y[0]) for x, y in zip(lst, b[sid])}
            injected += len(lst) > len(b[sid])
        dropped += len(after) < len(before)
    assert signs == {-1, 0, 1} and injected and dropped


# ---- a long parent chain -----------------------------------------------------------------------------------
def test_a_parent_chain_of_2048_spans():
    n, tid, a, b = 2048, 77, G["hosts"]["A"], G["hosts"]["B"]
    case = {"trace_id": tid, "spans": []}
    for i in range(n):  # every span: the client on A, the server on B, whose clock is 1000 ahead
        t0 = 10 * i
        case["spans"].append({"id": i + 1, "parent": i or None, "annotations": [
            [t0, "cs", a], [t0 + 1001, "sr", b], [t0 + 1005, "ss", b], [t0 + 6, "cr", a]]})
    spans, anns = T.golden_rows(case)
    got = TimeSkewAdjuster.adjust(Trace(spans, annotations=anns))
    assert len(got.spans) == n
    assert product_view(got) == T.view(T.adjust(T.annotated(spans, anns)))
    # the parent's skew moves a child's B annotations first; its own skew is then nothing
    assert [(x.ts, x.kind) for x in got.getSpanById(n).annotations] == \
        [(10 * (n - 1), A.CS), (10 * (n - 1) + 6, A.CR), (10 * (n - 1) + 1, A.SR), (10 * (n - 1) + 5, A.SS)]
    assert max(got.toSpanDepths().values()) == n


# ---- the query methods ---------------------------------------------------------------------------------------
def stores(seeds=range(12)):
    span_model, ann_model, cases = [], [], []
    for seed in seeds:
        case = T.random_case(np.random.default_rng(2000 + seed), 500 + seed, max_spans=16)
        spans, anns = T.golden_rows(case)
        span_model += spans
        ann_model += anns
        cases.append((case["trace_id"], spans, anns))
    return HostSpanStore(span_model), HostAnnotationStore(ann_model), cases


def test_adjust_nothing_reproduces_todays_answers():
    store, annots, cases = stores()
    ids = [c[0] for c in cases][::-1] + [404]
    by = {tid: spans for tid, spans, _ in cases}
    plain = store.getTracesByIds(ids)
    assert [t.annotations for t in plain] == [None] * len(cases) and not any(isinstance(s, AnnotatedSpan) for t in plain for s in t.spans)
    assert [[tuple(s) for s in t.spans] for t in plain] == [[tuple(s) for s in Trace(by[i]).spans] for i in ids if i in by]
    for name in ("getTracesByIds", "getTraceSummariesByIds", "getTraceCombosByIds"):
        call = getattr(store, name)
        got, again = call(ids), call(ids, adjust=())
        if name == "getTracesByIds":
            got, again = ([[tuple(s) for s in t.spans] for t in x] for x in (got, again))
        elif name == "getTraceCombosByIds":
            assert all(c.timeline is None for c in got + again)
            got, again = ([([tuple(s) for s in c.trace.spans], c.summary, c.span_depths) for c in x] for x in (got, again))
        assert got == again and len(got) == len(cases)
    assert [summary_tuple(s) for s in store.getTraceSummariesByIds(ids)] == [R.summary(by[i]) for i in ids if i in by]
    assert [c.span_depths for c in store.getTraceCombosByIds(ids)] == [R.span_depths(by[i]) for i in ids if i in by]


def test_query_methods_fold_the_adjusters():
    store, annots, cases = stores()
    ids = [c[0] for c in cases] + [404, cases[0][0]]
    want = [T.adjust(T.annotated(s, a)) for _, s, a in cases] + [T.adjust(T.annotated(*cases[0][1:]))]
    tids = [c[0] for c in cases] + [cases[0][0]]
    got = store.getTracesByIds(ids, adjust=SKEW, annotations=annots)
    assert [product_view(t) for t in got] == [T.view(w) for w in want]
    sums = store.getTraceSummariesByIds(ids, adjust=SKEW, annotations=annots)
    assert [summary_tuple(s) for s in sums] == [s for s in (T.summary(w, t) for w, t in zip(want, tids)) if s is not None]
    lines = store.getTraceTimelinesByIds(ids, adjust=SKEW, annotations=annots)
    assert [timeline_tuple(t) for t in lines] == [T.timeline(w, t) for w, t in zip(want, tids)]
    raw = store.getTraceTimelinesByIds(ids, annotations=annots)
    assert [timeline_tuple(t) for t in raw] == [T.timeline(T.annotated(s, a), t) for t, s, a in cases + [cases[0]]]
    combos = store.getTraceCombosByIds(ids, adjust=SKEW, annotations=annots)
    assert [timeline_tuple(c.timeline) for c in combos] == [timeline_tuple(t) for t in lines]
    assert [summary_tuple(c.summary) for c in combos] == [T.summary(w, t) for w, t in zip(want, tids)]
    assert all(isinstance(c, TraceCombo) and c.span_depths == c.trace.toSpanDepths() for c in combos)
    # a service dictionary names the hosts; a missing host is "Unknown"
    names = [f"svc{i}" for i in range(256)]
    named = HostSpanStore(store.model, services=names).getTraceTimelinesByIds(tids[:3], adjust=SKEW, annotations=annots)
    assert [timeline_tuple(t) for t in named] == [T.timeline(w, t, names) for w, t in zip(want[:3], tids[:3])]
    assert any(a.service == "Unknown" for t in named for a in t.annotations) or \
        all(h is not None for w in want[:3] for s in w for *_, h in s["ann"])


def test_a_trace_absent_from_the_annotation_store_is_unadjusted():
    store, annots, cases = stores()
    tid, spans, _ = cases[0]
    empty = HostAnnotationStore([])
    got = store.getTracesByIds([tid], adjust=SKEW, annotations=empty)[0]
    assert [tuple(s) for s in got.spans] == [tuple(s) for s in Trace(spans).spans] and len(got.spans) == len(R.trace(spans))
    assert [summary_tuple(s) for s in store.getTraceSummariesByIds([tid], adjust=SKEW, annotations=empty)] == [R.summary(spans)]
    assert store.getTraceTimelinesByIds([tid], annotations=empty)[0].annotations == []


def test_the_arguments_are_checked():
    store, annots, cases = stores(range(2))
    ids = [cases[0][0]]
    for call in (store.getTracesByIds, store.getTraceSummariesByIds, store.getTraceCombosByIds, store.getTraceTimelinesByIds):
        with pytest.raises(ValueError):
            call(ids, adjust=SKEW)  # no annotation store
        with pytest.raises(ValueError):
            call(ids, adjust=("SKEW",), annotations=annots)
    with pytest.raises(ValueError):
        store.getTraceTimelinesByIds(ids)
    for call in (store.getTraceSummariesByIds, store.getTraceCombosByIds):
        with pytest.raises(ValueError):
            call(ids, on_device=True, adjust=SKEW, annotations=annots)


def test_time_skew_changes_nothing_when_the_core_annotations_are_in_order():
    a, b, c, tid = G["hosts"]["A"], G["hosts"]["B"], G["hosts"]["C"], 9
    case = {"trace_id": tid, "spans": [
        {"id": 1, "parent": None, "annotations": [[100, "cs", a], [110, "sr", b], [190, "ss", b], [200, "cr", a], [150, "foo", b]]},
        {"id": 2, "parent": 1, "annotations": [[120, "cs", b], [125, "sr", c], [135, "ss", c], [140, "cr", b]]},
        {"id": 3, "parent": 1, "annotations": [[150, "cs", b], [151, "sr", a], [159, "ss", a], [160, "cr", b]]},
        {"id": 4, "parent": 3, "annotations": [[153, "sr", c], [155, "ss", c]]},
        {"id": 9, "parent": 8, "annotations": [[300, "cs", a]]}]}
    spans, anns = T.golden_rows(case)
    trace = Trace(spans, annotations=anns)
    got = TimeSkewAdjuster.adjust(trace)
    assert [s.id for s in got.spans] == [1, 2, 3, 4]  # (the span outside the root's tree goes)
    before = product_view(trace)
    assert product_view(got) == {k: before[k] for k in (1, 2, 3, 4)}
    assert [tuple(s) for s in got.spans] == [tuple(s) for s in trace.spans if s.id != 9]
