"""The annotation store's expiry model (tests/anexpref.py) on hand cases, and SpanRetention
(zipkin_amd/retention.py) with annotation stores over fake handles. No GPU."""
from tests import anexpref as X
from tests import spexpref as SX
from tests.anref import INT64_MAX, INT64_MIN
from tests.spref import TIMED
from zipkin_amd import SpanRetention, _abi

DAY_US = 24 * 3600 * 1_000_000


def arow(tid, ts, span=1):
    return (tid, span, ts, 0, 0, 0, 0)


def srow(tid, last, timed=True, span=1):
    return (tid, span, 0, 0, last, 0, TIMED if timed else 0)


class FakeStore:
    """A store as its model has it: a list of rows. `log` is shared, so the order of the calls over all stores
    can be read."""

    def __init__(self, name, rows, model, log):
        self.name, self.rows, self.model, self.log = name, list(rows), model, log

    def tracesExist(self, ids):
        self.log.append((self.name, "tracesExist"))
        have = {r[0] for r in self.rows}
        return {i for i in ids if i in have}

    def expire(self, min_end, pins=None):
        self.log.append((self.name, "expire", min_end, dict(pins or {})))
        left = self.model.survivors(self.rows, min_end, pins)
        removed, self.rows = len(self.rows) - len(left), left
        return removed


# ---- the model ----------------------------------------------------------------------------------------------
def test_model_whole_traces_by_the_maximum_ts_of_their_rows():
    rows = [arow(1, 10), arow(1, 50, span=2), arow(1, -7, span=3), arow(2, 49), arow(3, INT64_MIN), arow(3, INT64_MIN, span=2)]
    assert X.ends(rows) == {1: 50, 2: 49, 3: INT64_MIN}
    assert X.survivors(rows, 50) == rows[:3]           # end == cut stays, whole
    assert X.survivors(rows, 51) == []
    assert X.survivors(rows, 49) == rows[:4]
    assert X.survivors(rows, INT64_MIN) == rows        # an INT64_MIN-only trace stays at the floor only
    assert X.survivors(rows, INT64_MIN + 1) == rows[:4]
    assert X.survivors([arow(7, INT64_MAX), arow(7, 0)], INT64_MAX) == [arow(7, INT64_MAX), arow(7, 0)]
    assert X.survivors([arow(7, INT64_MAX - 1)], INT64_MAX) == []


def test_model_pins_replace_the_default_both_ways():
    rows = [arow(1, 10), arow(2, 60), arow(3, INT64_MIN)]
    assert X.survivors(rows, 50, {1: 5}) == rows[:2]              # a pin below the default keeps its trace
    assert X.survivors(rows, 50, {1: 10}) == rows[:2] and X.survivors(rows, 50, {1: 11}) == [rows[1]]
    assert X.survivors(rows, 50, {2: 61}) == []                   # a stricter pin removes its trace alone
    assert X.survivors(rows, 0, {2: 61}) == [rows[0]]
    assert X.survivors(rows, 50, {3: INT64_MIN}) == rows[1:]      # a pin at the floor keeps an INT64_MIN-only trace
    assert X.survivors(rows, 50, {99: INT64_MIN}) == [rows[1]]    # a pin for an absent id changes nothing


# ---- SpanRetention with annotation stores -------------------------------------------------------------------
def test_annotation_shards_get_the_span_shards_cutoff_and_pins_after_them():
    log = []
    spans = [FakeStore("s0", [srow(1, 0), srow(2, 0)], SX, log), FakeStore("s1", [srow(3, 0), srow(4, 5 * DAY_US)], SX, log)]
    annots = [FakeStore("a0", [arow(1, 0), arow(1, -5), arow(4, 5 * DAY_US)], X, log),
              FakeStore("a1", [arow(3, 0), arow(3, -1), arow(2, 0)], X, log)]
    r = SpanRetention(ttl_seconds=24 * 3600, spans=spans, annotations=annots)
    assert r.annotations == annots
    r.setTimeToLive(3, 10 * 24 * 3600)
    del log[:]
    out = r.expire(5 * DAY_US)
    want = (4 * DAY_US, {3: -5 * DAY_US})
    expires = [c for c in log if c[1] == "expire"]
    assert expires == [("s0", "expire") + want, ("s1", "expire") + want, ("a0", "expire") + want, ("a1", "expire") + want]
    assert out == {"cutoff": 4 * DAY_US, "spans": 2, "annotations": 3}
    assert {x[0] for a in annots for x in a.rows} == {3, 4} == {x[0] for s in spans for x in s.rows}
    # the pins' bookkeeping asks the span stores only
    assert {c[0] for c in log if c[1] == "tracesExist"} == {"s0", "s1"}
    assert r.pins == {3: 10 * 24 * 3600}
    one = SpanRetention(spans=spans[0], annotations=annots[0])
    assert one.spans == [spans[0]] and one.annotations == [annots[0]]
    assert SpanRetention(annotations=tuple(annots)).annotations == annots
    assert SpanRetention.MAX_PINS == _abi.ZK_AN_MAX_PINS


def test_annotations_is_in_the_result_only_when_they_were_given():
    def run(with_annots):
        log = []
        spans = FakeStore("s", [srow(1, 1 * DAY_US), srow(2, 1 * DAY_US), srow(3, 9 * DAY_US)], SX, log)
        annots = FakeStore("a", [arow(1, 1 * DAY_US), arow(2, 1 * DAY_US), arow(2, 0), arow(3, 9 * DAY_US)], X, log)
        r = SpanRetention(spans=spans, annotations=annots) if with_annots else SpanRetention(spans=spans)
        r.setTimeToLive(1, 30 * 24 * 3600)
        r.setTimeToLive(3, 3600)
        del log[:]
        return r.expire(10 * DAY_US), [c for c in log if c[0] == "s"], r.pins, annots.rows

    out0, calls0, pins0, _ = run(False)
    out1, calls1, pins1, left = run(True)
    assert out0 == {"cutoff": 3 * DAY_US, "spans": 2}                       # today's dict, key for key
    assert out1 == {"cutoff": 3 * DAY_US, "spans": 2, "annotations": 3}
    assert list(out1)[:2] == list(out0) and calls0 == calls1 and pins0 == pins1 == {1: 30 * 24 * 3600}
    assert left == [arow(1, 1 * DAY_US)]
    assert SpanRetention().annotations == [] and SpanRetention().expire(0) == {"cutoff": -7 * DAY_US, "spans": 0}
    # annotation stores alone: the default cutoff, no pins
    log = []
    a = FakeStore("a", [arow(1, 0), arow(2, 8 * DAY_US)], X, log)
    assert SpanRetention(annotations=a).expire(10 * DAY_US) == {"cutoff": 3 * DAY_US, "spans": 0, "annotations": 1}
    assert log == [("a", "expire", 3 * DAY_US, {})]
