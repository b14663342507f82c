"""The host side of the span store by trace id (include/zkspans.h, zipkin_amd/spanstore.py): the reference
model against the reference's own test vectors, and Trace / TraceSummary against the model. No GPU."""
import numpy as np
import pytest

from tests import spref as R
from zipkin_amd import Trace, TraceSummary, tracegen_host
from zipkin_amd.spanstore import Timespan

P, T, C, S = R.HAS_PARENT, R.TIMED, R.SVC_CLIENT, R.SVC_SERVER


def row(span, parent=None, first=0, last=0, svc=None, side=C, timed=True, name=0, trace=7):
    fl = (P if parent is not None else 0) | (T if timed else 0) | (side if svc is not None else 0) | (name << R.NAME_SHIFT)
    return (trace, span, parent or 0, first, last, svc or 0, fl)


def same_as_model(rows, services=None):
    """Trace and TraceSummary over the rows equal the model; returns the Trace."""
    t = Trace(rows, services)
    ref = R.trace(rows, services)
    assert [(s.id, s.parent, s.name, s.first, s.last, list(s.services)) for s in t.spans] == \
        [(s["id"], s["parent"], s["name"], s["first"], s["last"], s["services"]) for s in ref]
    se = R.start_end(rows)
    assert t.getStartAndEndTimestamp() == (None if se is None else Timespan(*se))
    assert [tuple(x) for x in t.spanTimestamps()] == R.span_timestamps(rows, services)
    assert t.serviceCounts() == R.service_counts(rows, services)
    assert t.services == set(R.service_counts(rows, services))
    assert t.toSpanDepths() == R.span_depths(rows)
    root = R.root_most(rows)
    assert (t.getRootMostSpan().id if t.getRootMostSpan() else None) == (root["id"] if root else None)
    got, want = TraceSummary.of(t), R.summary(rows, services)
    assert (None if got is None else (got.trace_id, got.start, got.end, got.duration_micro,
                                      [tuple(x) for x in got.span_timestamps], got.endpoints)) == want
    return t


@pytest.mark.parametrize("case", R.golden()["cases"], ids=lambda c: c["name"])
def test_model_and_trace_against_the_reference_vectors(case):
    g = R.golden()
    rows = R.golden_rows(case, g["services"])
    e = case["expect"]
    se = R.start_end(rows)
    assert (None if se is None else list(se)) == e["start_end"]
    assert [s["id"] for s in R.trace(rows)] == e["span_order"]
    sm = R.summary(rows, g["services"])
    if e["start_end"] is None:
        assert sm is None
    else:
        assert sm[3] == e["duration_micro"] and sm[1:3] == tuple(e["start_end"]) and sm[0] == case["trace_id"]
    if "services" in e:
        assert sorted(R.service_counts(rows, g["services"])) == e["services"]
    if "depths" in e:
        assert R.span_depths(rows) == {int(k): v for k, v in e["depths"].items()}
    if "root_span" in e:
        assert R.root_most(rows)["id"] == e["root_span"]
    t = same_as_model(rows, g["services"])
    assert t.duration == (e["start_end"][1] - e["start_end"][0] if e["start_end"] else 0)
    if "children" in e:
        assert {str(k): [s.id for s in v] for k, v in t.getIdToChildrenMap().items()} == e["children"]
    if "root_span" in e:
        assert t.getRootSpan().id == e["root_span"]
    # the order of the rows does not matter
    assert [s.id for s in Trace(rows[::-1]).spans] == e["span_order"]


def test_the_file_says_why_service_counts_is_left_out():
    assert "get service counts" in R.golden()["description"]


def test_generated_traces_with_split_fragments():
    """TraceGen's spans come as a client and a server fragment of one span id: every trace of a generated
    batch, its rows shuffled, against the model; with a services dictionary too."""
    cols = tracegen_host(seed=5, num_traces=60, max_depth=5, num_services=9)
    cols.set_name_ids((cols.span_id % np.uint64(5)).astype(np.int64))
    store = R.rows_of(cols)
    ids = sorted({r[0] for r in store})
    assert len(ids) == 60
    names = [f"Svc{i}" for i in range(9)]
    rng = np.random.default_rng(1)
    split = 0
    for i in ids:
        _, rows = R.gather(store, [i])
        split += len(rows) > len({r[1] for r in rows})
        rows = [rows[j] for j in rng.permutation(len(rows))]
        same_as_model(rows)
        t = same_as_model(rows, names)
        assert all(isinstance(v, str) and v == v.lower() for v in t.services)
    assert split > 30  # (fragments of one span in several rows)


def test_fragments_merge_by_span_id():
    rows = [row(5, 1, 300, 400, svc=2, side=C, name=0), row(5, 1, 250, 350, svc=4, side=S, name=9),
            row(5, None, -5, 999, timed=False), row(1, None, 100, 500, svc=2, side=S, name=3)]
    t = same_as_model(rows)
    s = t.getSpanById(5)
    assert (s.first, s.last, s.parent, s.name, s.services) == (250, 400, 1, 9, (2, 4))  # two services, the untimed row's times ignored
    assert t.serviceCounts() == {2: 2, 4: 1}
    assert [tuple(x) for x in t.spanTimestamps()] == [(2, 100, 500), (2, 250, 400), (4, 250, 400)]
    assert t.toSpanDepths() == {1: 1, 5: 2}


def test_an_untimed_only_span_sorts_last_and_a_trace_of_them_has_no_summary():
    rows = [row(9, None, 1, 2, timed=False, svc=1), row(3, 9, 50, 60, svc=1), row(2 ** 64 - 1, 9, 10, 20, timed=False)]
    t = same_as_model(rows)
    assert [s.id for s in t.spans] == [3, 9, 2 ** 64 - 1]  # untimed as INT64_MAX, ties by span id unsigned
    assert t.getSpanById(9).first is None and t.getStartAndEndTimestamp() == Timespan(50, 60)
    only = same_as_model([rows[0], rows[2]])
    assert only.getStartAndEndTimestamp() is None and TraceSummary.of(only) is None and only.duration == 0
    assert only.services == {1} and only.spanTimestamps() == []


def test_a_missing_root():
    # no span without a parent: from the first span upwards through the parents the trace holds
    rows = [row(20, 10, 5, 6), row(30, 20, 7, 8), row(40, 30, 1, 2), row(50, 77, 9, 9)]
    t = same_as_model(rows)
    assert t.getRootSpan() is None and t.getRootMostSpan().id == 20
    assert t.toSpanDepths() == {20: 1, 30: 2, 40: 3}
    # the reference's own pair: a parent id that no span has
    pair = same_as_model([row(200, 100), row(100, 12345)])
    assert pair.getRootMostSpan().id == 100 and pair.toSpanDepths() == {100: 1, 200: 2}
    # a parent chain that closes on itself ends
    loop = same_as_model([row(1, 2, 1, 1), row(2, 1, 2, 2)])
    assert loop.toSpanDepths() in ({1: 2, 2: 1}, {1: 1, 2: 2})
    assert Trace([]).toSpanDepths() is None and Trace([]).id is None and TraceSummary.of(Trace([])) is None


def test_duration_micro_wraps_to_32_bits():
    a = TraceSummary.of(same_as_model([row(1, None, 0, 2 ** 31)]))
    assert (a.start, a.end, a.duration_micro) == (0, 2 ** 31, -2 ** 31)
    b = same_as_model([row(1, None, R.INT64_MIN, R.INT64_MAX)])
    sb = TraceSummary.of(b)
    assert (sb.start, sb.end, sb.duration_micro) == (R.INT64_MIN, R.INT64_MAX, -1) and b.duration == -1
    c = TraceSummary.of(same_as_model([row(1, None, 0, 2 ** 32 + 5, svc=3), row(2, 1, 7, 8)]))
    assert c.duration_micro == 5 and c.endpoints == []
    assert c.span_timestamps[0].duration == 2 ** 32 + 5


def test_names_from_the_dictionaries():
    rows = [row(1, None, 1, 2, svc=1, name=2), row(2, 1, 3, 4, svc=0, side=S)]
    t = Trace(rows, ["Web", "DB"], ["get", "Put"])
    assert [(s.name, s.services) for s in t.spans] == [("Put", ("db",)), (None, ("web",))]
    with pytest.raises(ValueError):
        Trace(rows, ["Web"])


def test_model_store_is_a_multiset_in_canonical_order():
    a = [row(2, None, 5, 6, trace=1), row(1, None, 9, 9, trace=1), row(1, None, -3, 9, trace=1), row(4, None, trace=2)]
    store = R.rows_of([R.cols_of(a), R.cols_of(a[:2])])
    assert R.exist(store, [1, 2, 3]) == [True, True, False]
    counts, rows = R.gather(store, [2, 3, 1, 2])
    assert counts == [1, 0, 5, 1]
    assert rows[0] == rows[-1] == a[3]
    assert rows[1:6] == [a[2], a[1], a[1], a[0], a[0]]  # signed first_ts, equal rows as often as entered
    assert R.spans_by_trace_ids(store, [3, 2]) == [[a[3]]]
    assert all(R.bucket(R.id_in_bucket(b, k)) == b for b in (0, 1, 4095) for k in (0, 1, 12345))
