"""The span store's expiry on the device (include/zkspans.h "Expiry", zk_sp_expire) against
tests/spexpref.py: after every call the store answers exactly as a fresh store that observed only the
model's survivors. Every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

from tests import spexpref as X
from tests import spref as R
from zipkin_amd import (DeviceColumns, SpanColumns, SpanRetention, TraceDurationIndex, TraceSpanStore, ZkError, _abi,
                        tracegen_host)

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
MIN, MAX = R.INT64_MIN, R.INT64_MAX
SCATTER_CHUNK = 16384  # k_sp_scatter's and the rewrite's stretch per workgroup
FIND_PART = 4096       # the lookups split a slice longer than this over several workgroups


@pytest.fixture()
def make(gpu):
    made = []

    def factory(**kw):
        made.append(TraceSpanStore(device=gpu, **kw))
        return made[-1]

    yield factory
    for s in made:
        s.close()


def cols_of(rows) -> SpanColumns:
    c = SpanColumns.empty(len(rows))
    for j, k in enumerate(R.COLS):
        col = getattr(c, k)
        col[:] = np.array([r[j] for r in rows], col.dtype)
    return c


def observe_rows(store, batches):
    for rows in batches:
        if rows:
            store.observe(DeviceColumns.from_host(cols_of(rows)))


def frag(tid, last, timed=True, rng=None):
    """One fragment of trace tid: last_ts as given, the other columns noise."""
    rng = rng or np.random.default_rng(tid & 0xFFFF)
    fl = int(rng.integers(0, 2 ** 32)) & ~R.TIMED | (R.TIMED if timed else 0)
    return (tid, int(rng.integers(0, 6)), int(rng.integers(0, 6)), int(rng.integers(-2 ** 63, 2 ** 63)), last,
            int(rng.integers(0, 2 ** 32)), fl)


def same_as_fresh(store, make, left, ids):
    """The store against a fresh one that observed `left`, and both against the model."""
    fresh = make()
    observe_rows(fresh, [left])
    assert store.info()["entries"] == fresh.info()["entries"] == len(left)
    assert store.tracesExist(ids) == fresh.tracesExist(ids) == {r[0] for r in left}
    got = store.getSpansByTraceIds(ids)
    assert got == fresh.getSpansByTraceIds(ids)
    assert got == R.spans_by_trace_ids(left, ids)


def expire_and_check(store, make, rows, min_end, pins=None, extra=()):
    """One expiry of a store that holds `rows`; the survivors."""
    left = X.survivors(rows, min_end, pins)
    before = store.info()["entries"]
    assert before == len(rows)
    removed = store.expire(min_end, pins)
    assert removed == len(rows) - len(left) == before - store.info()["entries"]
    same_as_fresh(store, make, left, sorted({r[0] for r in rows}) + list(extra))
    return left


def split(rows, k, seed):
    perm = np.random.default_rng(seed).permutation(len(rows))
    cuts = np.linspace(0, len(rows), k + 1).astype(int)
    return [[rows[i] for i in perm[a:b]] for a, b in zip(cuts[:-1], cuts[1:])]


# ---- 1. mixed traces at the boundary -------------------------------------------------------------------------
def test_mixed_traces_at_the_boundary(make):
    rng = np.random.default_rng(1)
    ids = [0, U64] + np.unique(rng.integers(0, 2 ** 64, 3000, dtype=np.uint64)).tolist()
    rows = []
    for t in ids:
        for _ in range(int(rng.integers(1, 13))):
            timed = rng.random() < 0.8
            last = int(rng.integers(0, 1000)) if timed else int(rng.choice([MAX, MIN, 500, 2000]))
            rows.append(frag(t, last, timed, rng))
    end = X.ends(rows)
    cut = int(np.median([e for e in end.values() if e != MIN]))
    at_cut = [t for t, e in end.items() if e == cut]
    assert at_cut and any(e == cut - 1 for e in end.values()) and any(e == MIN for e in end.values())
    store = make()
    observe_rows(store, split(rows, 5, seed=1))
    assert store.info()["segments"] == 5
    absent = [int(ids[5]) ^ 1, 12345]
    left = expire_and_check(store, make, rows, cut, extra=absent)
    assert 0 < len(left) < len(rows) and set(at_cut) <= {r[0] for r in left}  # end == cutoff stays
    assert store.info()["segments"] == 1
    left2 = expire_and_check(store, make, left, cut + 1, extra=absent)
    assert not set(at_cut) & {r[0] for r in left2} and len(left2) < len(left)
    assert expire_and_check(store, make, left2, cut + 1) == left2  # nothing more goes


# ---- 2. a trace across three segments ------------------------------------------------------------------------
@pytest.mark.parametrize("cut,stays", [(100, True), (101, False)], ids=("end_at_cut", "one_above"))
def test_a_trace_across_three_segments(make, cut, stays):
    t, other = R.id_in_bucket(77, 0), R.id_in_bucket(77, 1)
    segs = [[frag(t, 10), frag(t, 20), frag(other, 100), frag(5, 500)],
            [frag(t, 30), frag(t, MAX, timed=False), frag(other, 10), frag(6, 50)],
            [frag(7, 100), frag(t, 100), frag(8, 101)]]
    rows = [r for s in segs for r in s]
    store = make()
    observe_rows(store, segs)
    assert store.info()["segments"] == 3
    left = expire_and_check(store, make, rows, cut, extra=[9])
    assert sum(r[0] == t for r in left) == (5 if stays else 0)


# ---- 3. untimed fragments ----------------------------------------------------------------------------------------
def test_untimed_fragments(make):
    u, t1, t2 = 11, 0, U64
    rows = [frag(u, MAX, timed=False), frag(u, 7, timed=False), frag(t1, 5), frag(t1, MAX, timed=False),
            frag(t1, MAX, timed=False), frag(t2, MAX), frag(t2, 3, timed=False), frag(13, MAX - 1), frag(14, MIN)]
    store = make()
    observe_rows(store, split(rows, 2, seed=3))
    # an untimed-only trace (and a timed end at INT64_MIN) stays at INT64_MIN: without a pass, and through
    # the passes (a pin for an absent id sends the call there)
    assert expire_and_check(store, make, rows, MIN) == rows
    assert expire_and_check(store, make, rows, MIN, pins={999: 0}) == rows
    left = expire_and_check(store, make, rows, MIN + 1)
    assert {r[0] for r in left} == {t1, t2, 13}
    left = expire_and_check(store, make, left, 6)       # the untimed fragments at INT64_MAX keep no trace
    assert {r[0] for r in left} == {t2, 13}
    left = expire_and_check(store, make, left, MAX)     # a timed fragment at INT64_MAX keeps its trace
    assert {r[0] for r in left} == {t2} and len(left) == 2


# ---- 4. INT64_MIN without pins ------------------------------------------------------------------------------------
def test_int64_min_without_pins_changes_nothing(make):
    rows = [frag(t % 50, t % 17, t % 3 != 0) for t in range(400)]
    store = make()
    observe_rows(store, split(rows, 3, seed=4))
    before = store.info()
    assert store.expire(MIN) == 0 and store.expire(MIN, {}) == 0
    assert store.info() == before and before["segments"] == 3
    same_as_fresh(store, make, rows, list(range(52)))
    empty = make()
    assert empty.expire(0) == 0 and empty.expire(MAX, {5: MIN}) == 0
    assert empty.info() == {"entries": 0, "segments": 0, "bytes": 0}


# ---- 5. a long trace -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut,stays", [(900, True), (901, False)], ids=("stays", "goes"))
def test_a_long_trace(make, cut, stays):
    n = 20000
    assert n > SCATTER_CHUNK and n // 2 > FIND_PART
    long_id, other = R.id_in_bucket(9, 0), R.id_in_bucket(9, 1)
    rng = np.random.default_rng(5)
    rows = [frag(long_id, int(rng.integers(0, 900)), rng.random() < 0.1, rng) for _ in range(n - 1)]
    rows.insert(n - 3, frag(long_id, 900, True, rng))  # its end, in the second segment
    rows += [frag(other, 950, True, rng) for _ in range(300)] + [frag(int(x), 10 * int(x) % 1800, True, rng) for x in range(200)]
    segs = [rows[:n // 2] + rows[n:n + 250], rows[n // 2:n] + rows[n + 250:]]
    store = make()
    observe_rows(store, segs)
    left = expire_and_check(store, make, rows, cut, extra=[R.id_in_bucket(9, 2)])
    assert sum(r[0] == long_id for r in left) == (n if stays else 0) and sum(r[0] == other for r in left) == 300


# ---- 6. a skewed store ---------------------------------------------------------------------------------------------
def test_a_skewed_store(make):
    rng = np.random.default_rng(6)
    heavy = [R.id_in_bucket(1234, k) for k in range(300)]
    assert {R.bucket(i) for i in heavy} == {1234}
    spread = np.unique(rng.integers(0, 2 ** 64, 400, dtype=np.uint64)).tolist()
    rows = [frag(t, int(rng.integers(0, 100)), rng.random() < 0.7, rng) for t in heavy for _ in range(20)]
    rows += [frag(t, int(rng.integers(0, 100)), rng.random() < 0.7, rng) for t in spread for _ in range(int(rng.integers(1, 7)))]
    assert sum(r[0] in set(heavy) for r in rows) == 6000 and len(rows) > 6000 + 1024
    cut = int(np.median(list(X.ends(rows).values())))
    pins = {heavy[0]: MIN, heavy[1]: MAX, spread[0]: MIN}
    lefts = []
    for chunk in (1024, 0):  # the big bucket above the chunk and the rest in several ranges; then one range
        store = make(expire_chunk=chunk)
        observe_rows(store, split(rows, 3, seed=6))
        lefts.append(expire_and_check(store, make, rows, cut, pins=pins, extra=[R.id_in_bucket(1234, 300)]))
        assert 0 < len(lefts[-1]) < len(rows)
    assert lefts[0] == lefts[1]


# ---- 7. 64 segments ------------------------------------------------------------------------------------------------
def test_64_time_sorted_segments(make):
    rng = np.random.default_rng(7)
    segs = [[frag(1000 * k + t, 100 * k + int(rng.integers(0, 100)), True, rng) for t in range(20) for _ in range(2)] for k in range(64)]
    for k in range(64):
        segs[k][0] = segs[k][0][:4] + (100 * k + 99,) + segs[k][0][5:]  # trace 1000 k ends at the segment's top
    rows = [r for s in segs for r in s]
    store = make()
    observe_rows(store, segs)
    before = store.info()
    assert before["segments"] == 64
    cut = 100 * 20 + 50
    left = expire_and_check(store, make, rows, cut)
    after = store.info()
    # 20 segments freed, the 21st rewritten, 43 untouched
    assert after["segments"] == 44 and 0 < len(left) - 43 * 40 < 40 and after["bytes"] < before["bytes"]


def test_64_segments_each_half_expiring(make):
    rng = np.random.default_rng(8)
    segs = [[frag(1000 * k + t, (0 if t % 2 else 100) + int(rng.integers(0, 50)), t % 5 != 0, rng) for t in range(16) for _ in range(3)]
            for k in range(64)]
    rows = [r for s in segs for r in s]
    store = make()
    observe_rows(store, segs)
    assert store.info()["segments"] == 64
    left = expire_and_check(store, make, rows, 100)
    assert store.info()["segments"] == 1 and 0 < len(left) < len(rows)
    # a later observe of older data enters the store again (the cut is made once), and goes at the next cut
    again = segs[0] + [frag(77777, 5), frag(1000, 150)]
    observe_rows(store, [again])
    rows2 = left + again
    assert store.info()["segments"] == 2
    same_as_fresh(store, make, rows2, sorted({r[0] for r in rows2}))
    left2 = expire_and_check(store, make, rows2, 100)
    assert store.info()["segments"] <= 2 and 77777 not in {r[0] for r in left2} and len(left2) > len(left)


# ---- 8. pins ---------------------------------------------------------------------------------------------------------
def raw_expire(store, min_end, ids, cuts):
    ids, cuts, removed = np.array(ids, np.uint64), np.array(cuts, np.int64), C.c_uint64(77)
    st = store._L.zk_sp_expire(store._h, min_end, ids.ctypes.data, cuts.ctypes.data, len(ids), C.byref(removed))
    return st, int(removed.value)


def test_pins(make):
    a, b, c, d, e, f = 21, 22, 0, 24, 25, U64
    rows = [frag(a, 10), frag(a, 3, timed=False), frag(b, 60), frag(b, 61, timed=False), frag(c, 9, timed=False),
            frag(d, 100), frag(e, 20), frag(f, MAX), frag(f, 1)]
    ids = [a, b, c, d, e, f]

    def fresh_store():
        s = make()
        observe_rows(s, split(rows, 2, seed=8))
        return s

    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, 50, {a: 5})} == {a, b, d, f}     # below the cutoff, pinned: stays
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, 50, {a: 11})} == {b, d, f}       # the pin is a cutoff too
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, 50, {b: 61})} == {d, f}          # a stricter pin: its trace alone
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, MIN, {b: 61})} == {a, c, d, e, f}
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, 50, {c: MIN})} == {b, c, d, f}   # an untimed-only trace, pinned
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, 50, {c: MIN + 1})} == {b, d, f}
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, MAX, {f: MAX, d: 100, e: 21})} == {d, f}
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, 50, {404: MIN, 405: MAX})} == {b, d, f}  # absent ids
    # a duplicated pin, too many pins: refused, the store unchanged
    store = fresh_store()
    before = store.info()
    assert raw_expire(store, 50, [a, b, a], [1, 2, 3]) == (_abi.ZK_ERR_INVALID_ARG, 0)
    n = _abi.ZK_SP_MAX_PINS + 1
    assert raw_expire(store, 50, list(range(1000, 1000 + n)), [0] * n) == (_abi.ZK_ERR_INVALID_ARG, 0)
    with pytest.raises(ValueError):
        store.expire(50, {1000 + i: 0 for i in range(n)})
    assert store.info() == before
    same_as_fresh(store, make, rows, ids)


def test_4096_pins_in_one_call(make):
    rng = np.random.default_rng(9)
    ids = np.unique(rng.integers(0, 2 ** 64, 3000, dtype=np.uint64)).tolist()
    rows = [frag(t, int(rng.integers(0, 100)), rng.random() < 0.9, rng) for t in ids for _ in range(int(rng.integers(1, 4)))]
    pins = {t: int(rng.integers(0, 100)) for t in ids[:2500]}
    pins.update({int(x): MIN for x in rng.integers(0, 2 ** 64, 4096 - len(pins), dtype=np.uint64) if int(x) not in set(ids)})
    assert len(pins) == _abi.ZK_SP_MAX_PINS
    store = make()
    observe_rows(store, split(rows, 3, seed=9))
    left = expire_and_check(store, make, rows, 50, pins)
    default = X.survivors(rows, 50)
    assert left != default and 0 < len(left) < len(rows)


# ---- 9. the invariant with the duration index ----------------------------------------------------------------
def test_the_duration_index_holds_the_same_ids(make, gpu):
    cols = tracegen_host(seed=41, num_traces=400, max_depth=5, num_services=7)
    rows = R.rows_of(cols) + [frag(R.id_in_bucket(3, 1), MAX, timed=False) for _ in range(3)]
    parts = split(rows, 4, seed=41)
    cut = int(np.median([e for e in X.ends(rows).values() if e != MIN]))
    store = make()
    with TraceDurationIndex(device=gpu) as td:
        for p in parts:
            d = DeviceColumns.from_host(cols_of(p))
            store.observe(d)
            td.observe(d)
        left = expire_and_check(store, make, rows, cut)
        td.expire(cut)
        ids = sorted({r[0] for r in rows})
        found = td.lookup(ids)[2]
        held = {i for i, f in zip(ids, found.tolist()) if f}
    assert held == X.timed_ids(left) == store.tracesExist(ids) and 0 < len(held) < 400


# ---- 10. SpanRetention end to end ----------------------------------------------------------------------------
def test_span_retention_on_two_shards(make):
    day = 24 * 3600 * 1_000_000
    now = 20 * day
    rows = [frag(t, (t % 20) * day + 5, True) for t in range(200) for _ in range(2)] + [frag(500, 0, timed=False)]
    shards = [[r for r in rows if r[0] % 2 == k] for k in (0, 1)]
    stores = [make(), make()]
    for s, sh in zip(stores, shards):
        observe_rows(s, split(sh, 2, seed=10))
    ret = SpanRetention(spans=stores)
    assert ret.ttl_seconds == 7 * 24 * 3600 and ret.getTimeToLive(3) == 7 * 24 * 3600
    ret.setTimeToLive(3, 30 * 24 * 3600)    # trace 3 ends on day 3: only the pin keeps it
    ret.setTimeToLive(19, 3600)             # trace 19 ends on day 19: its pin sends it away
    ret.setTimeToLive(9999, 3600)           # not in any shard: no pin
    assert ret.pins == {3: 30 * 24 * 3600, 19: 3600} and ret.getTimeToLive(3) == 30 * 24 * 3600
    with pytest.raises(ValueError, match="The trace 9999 does not have any ttl set!"):
        ret.getTimeToLive(9999)
    out = ret.expire(now)
    pins = {3: now - 30 * day, 19: now - 3600 * 1_000_000}
    lefts = [X.survivors(sh, now - 7 * day, pins) for sh in shards]
    assert out == {"cutoff": 13 * day, "spans": len(rows) - len(lefts[0]) - len(lefts[1])}
    for s, sh, left in zip(stores, shards, lefts):
        same_as_fresh(s, make, left, sorted({r[0] for r in sh}))
    alive = {r[0] for left in lefts for r in left}
    assert 3 in alive and 19 not in alive and 500 not in alive and 13 in alive and 12 not in alive
    assert ret.pins == {3: 30 * 24 * 3600}  # the pin of the trace that went is dropped


# ---- timing ----------------------------------------------------------------------------------------------------------
def test_expire_ms(make):
    rows = [frag(t % 100, t % 40, True) for t in range(3000)]
    store = make(timing=True)
    with pytest.raises(ZkError):
        store.expire_ms()
    observe_rows(store, split(rows, 2, seed=11))
    for cut in (20, 20):  # a rewrite, then an expiry where nothing goes
        store.expire(cut)
        ms = store.expire_ms()
        assert tuple(ms) == TraceSpanStore.EXPIRE_PHASES and all(np.isfinite(v) and v >= 0 for v in ms.values())
    plain = make()
    observe_rows(plain, [rows])
    plain.expire(20)
    with pytest.raises(ZkError) as e:
        plain.expire_ms()
    assert e.value.status == _abi.ZK_ERR_INVALID_ARG
