"""SpanRetention (zipkin_amd/retention.py) over fake handles, and the expiry model (tests/spexpref.py) on
hand cases. No GPU."""
import pytest

from tests import spexpref as X
from tests.spref import INT64_MAX, INT64_MIN, TIMED
from zipkin_amd import IndexRetention, SpanRetention

DAY_US = 24 * 3600 * 1_000_000


def row(tid, last, timed=True, span=1):
    return (tid, span, 0, 0, last, 0, TIMED if timed else 0)


class FakeStore:
    """A span store as the model has it: a list of rows."""

    def __init__(self, rows):
        self.rows = list(rows)
        self.have = {r[0] for r in self.rows}
        self.calls = []

    def tracesExist(self, ids):
        return {i for i in ids if i in self.have}

    def expire(self, min_end, pins=None):
        self.calls.append((min_end, dict(pins or {})))
        left = X.survivors(self.rows, min_end, pins)
        removed, self.rows = len(self.rows) - len(left), left
        self.have = {r[0] for r in left}
        return removed


# ---- the model ----------------------------------------------------------------------------------------------
def test_model_whole_traces_by_the_end_of_their_timed_rows():
    rows = [row(1, 10), row(1, 50, span=2), row(1, 99, timed=False, span=3), row(2, 49), row(3, INT64_MAX, timed=False)]
    assert X.ends(rows) == {1: 50, 2: 49, 3: INT64_MIN}
    assert X.survivors(rows, 50) == rows[:3]          # end == cutoff stays, with its untimed row
    assert X.survivors(rows, 51) == []                 # the untimed last_ts keeps nothing
    assert X.survivors(rows, INT64_MIN) == rows        # an untimed-only trace stays at the floor
    assert X.survivors(rows, INT64_MIN + 1) == rows[:4]
    assert X.survivors([row(7, INT64_MAX)], INT64_MAX) == [row(7, INT64_MAX)]
    assert X.timed_ids(rows) == {1, 2}


def test_model_pins_replace_the_default_for_their_trace():
    rows = [row(1, 10), row(2, 60), row(3, 0, timed=False)]
    assert X.survivors(rows, 50, {1: 5}) == rows[:2]              # a pin below the cutoff keeps its trace
    assert X.survivors(rows, 50, {2: 61}) == []                   # a stricter pin removes its trace alone
    assert X.survivors(rows, 0, {2: 61}) == [rows[0]]
    assert X.survivors(rows, 50, {3: INT64_MIN}) == rows[1:]      # a pin at the floor keeps an untimed-only trace
    assert X.survivors(rows, 50, {99: INT64_MIN}) == [rows[1]]    # a pin for an absent id changes nothing


# ---- SpanRetention ------------------------------------------------------------------------------------------
def test_defaults_and_refused_ttls():
    r = SpanRetention()
    assert r.ttl_seconds == 7 * 24 * 3600 and r.spans == [] and r.pins == {}
    assert IndexRetention().ttl_seconds == 3 * 24 * 3600  # (it stays as it was: the span ttl is the longer one)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            SpanRetention(ttl_seconds=bad)
        with pytest.raises(ValueError):
            SpanRetention(spans=FakeStore([row(1, 0)])).setTimeToLive(1, bad)
    assert SpanRetention(ttl_seconds=3.0).ttl_seconds == 3


def test_cutoff_is_clamped_at_both_int64_ends():
    r = SpanRetention(ttl_seconds=1)
    assert r.cutoff(5_000_000) == 4_000_000
    assert r.cutoff(INT64_MIN) == INT64_MIN and r.cutoff(INT64_MIN + 999_999) == INT64_MIN
    assert r.cutoff(INT64_MIN + 1_000_001) == INT64_MIN + 1
    assert r.cutoff(INT64_MAX) == INT64_MAX - 1_000_000
    assert r.cutoff(INT64_MAX + 10 ** 9) == INT64_MAX


def test_pin_bookkeeping():
    store = FakeStore([row(1, 1 * DAY_US), row(2, 1 * DAY_US), row(3, 9 * DAY_US)])
    r = SpanRetention(spans=store)
    r.setTimeToLive(99, 3600)                      # not a member: ignored
    assert r.pins == {}
    with pytest.raises(ValueError, match="The trace 99 does not have any ttl set!"):
        r.getTimeToLive(99)
    assert r.getTimeToLive(1) == 7 * 24 * 3600     # the default
    r.setTimeToLive(1, 30 * 24 * 3600)
    r.setTimeToLive(3, 3600)
    assert r.getTimeToLive(1) == 30 * 24 * 3600 and r.getTimeToLive(3) == 3600 and r.getTimeToLive(2) == 7 * 24 * 3600
    now = 10 * DAY_US
    out = r.expire(now)
    assert out == {"cutoff": 3 * DAY_US, "spans": 2}
    assert store.calls == [(3 * DAY_US, {1: now - 30 * DAY_US, 3: now - 3600 * 1_000_000})]
    assert {x[0] for x in store.rows} == {1}       # 1 stays by its pin, 2 goes by the default, 3 by its stricter pin
    assert r.pins == {1: 30 * 24 * 3600}            # the pin of the trace that went is dropped
    with pytest.raises(ValueError):
        r.getTimeToLive(3)


def test_every_shard_gets_every_pin():
    a, b = FakeStore([row(1, 0), row(2, 0)]), FakeStore([row(3, 0), row(4, 5 * DAY_US)])
    r = SpanRetention(ttl_seconds=24 * 3600, spans=[a, b])
    r.setTimeToLive(3, 10 * 24 * 3600)
    assert r.getTimeToLive(3) == 10 * 24 * 3600 and r.getTimeToLive(1) == 24 * 3600
    out = r.expire(5 * DAY_US)
    assert out == {"cutoff": 4 * DAY_US, "spans": 2}
    assert a.calls == b.calls == [(4 * DAY_US, {3: -5 * DAY_US})]
    assert a.rows == [] and {x[0] for x in b.rows} == {3, 4} and r.pins == {3: 10 * 24 * 3600}
    assert SpanRetention(spans=a).spans == [a] and SpanRetention(spans=(a, b)).spans == [a, b]


def test_one_expiry_carries_every_pin():
    from zipkin_amd import _abi

    assert SpanRetention.MAX_PINS == _abi.ZK_SP_MAX_PINS
    r = SpanRetention(spans=FakeStore([row(t, 0) for t in range(SpanRetention.MAX_PINS + 1)]))
    for t in range(SpanRetention.MAX_PINS):
        r.setTimeToLive(t, 60)
    r.setTimeToLive(5, 90)  # a pinned trace may be pinned anew
    with pytest.raises(ValueError):
        r.setTimeToLive(SpanRetention.MAX_PINS, 60)
    assert len(r.pins) == SpanRetention.MAX_PINS and r.pins[5] == 90
