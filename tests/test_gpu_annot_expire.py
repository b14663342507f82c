"""The annotation store's expiry on the device (include/zkannots.h "Expiry", zk_an_expire) against
tests/anexpref.py: expire returns the rows the model removes, and after every call the store answers exactly as
a fresh store that observed only the model's survivors. Every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

from tests import anexpref as X
from tests import anref as R
from tests import spexpref as SX
from tests import spref as S
from tests.richgen import gen_traces
from tests.test_ingest import encode_all
from zipkin_amd import (AnnotationRows, DeviceAnnotationRows, SpanRetention, TraceAnnotationStore, TraceSpanStore, ZkError,
                        _abi)
from zipkin_amd.ingest import SpanDecoder

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
MIN, MAX = R.INT64_MIN, R.INT64_MAX
STRETCH = 16384  # k_an_scatter's and the rewrite's stretch per workgroup


@pytest.fixture()
def make(gpu):
    made = []

    def factory(**kw):
        made.append(TraceAnnotationStore(device=gpu, **kw))
        return made[-1]

    yield factory
    for s in made:
        s.close()


def row(tid, ts, rng=None, span=None):
    """One row of trace tid at ts; the other columns noise (a few span ids, so that the order's later keys decide)."""
    rng = rng or np.random.default_rng((tid ^ ts) & 0xFFFF)
    return (tid, int(rng.integers(0, 4)) * (2 ** 62 + 1) if span is None else span, ts, int(rng.integers(0, 3)) * (2 ** 63 - 5),
            int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32)))


def bulk(tids, tss, seed=0):
    """Row tuples from two sequences, the other columns noise."""
    cols = R.noise(np.asarray(tids, np.uint64), seed)
    cols[2] = np.asarray(tss, np.int64)
    return list(zip(*[c.tolist() for c in cols]))


def observe_rows(store, batches):
    for rows in batches:
        if rows:
            store.observe(DeviceAnnotationRows.from_host(AnnotationRows.of_rows(rows), store.device))


def same_as_fresh(store, make, left, ids):
    """The store against a fresh one that observed `left`, and both against the model: counts and rows in
    canonical order of every asked id, and the entries."""
    fresh = make()
    observe_rows(fresh, [left])
    assert store.info()["entries"] == fresh.info()["entries"] == len(left)
    got = store.getAnnotationsByTraceIds(ids)
    assert got == fresh.getAnnotationsByTraceIds(ids)
    assert got == R.by_trace_ids(left, ids)


def expire_and_check(store, make, rows, min_end, pins=None, extra=(404404,)):
    """One expiry of a store that holds `rows`; the survivors. The asked ids: every id ever present, and
    absent ones."""
    left = X.survivors(rows, min_end, pins)
    before = store.info()
    assert before["entries"] == len(rows)
    removed = store.expire(min_end, pins)
    after = store.info()
    assert removed == len(rows) - len(left) == before["entries"] - after["entries"]
    assert after["segments"] <= before["segments"]
    same_as_fresh(store, make, left, sorted({r[0] for r in rows}) + list(extra))
    return left


def split(rows, k, seed):
    perm = np.random.default_rng(seed).permutation(len(rows))
    cuts = np.linspace(0, len(rows), k + 1).astype(int)
    return [[rows[i] for i in perm[a:b]] for a, b in zip(cuts[:-1], cuts[1:])]


# ---- 1. mixed traces at the boundary -------------------------------------------------------------------------
def test_mixed_traces_at_the_boundary(make):
    rng = np.random.default_rng(1)
    ids = np.unique(rng.integers(1, 2 ** 64 - 1, 3000, dtype=np.uint64)).tolist()
    rows = [row(t, int(rng.integers(0, 1000)), rng) for t in ids for _ in range(int(rng.integers(1, 13)))]
    cut = int(np.median(list(X.ends(rows).values())))
    # trace id 0 (the slot behind the table) ends AT the cut: it stays first, then goes; 2^64 - 1 ends one below
    rows += [row(0, cut, rng), row(0, cut - 5, rng), row(0, MIN, rng), row(U64, cut - 1, rng), row(U64, cut - 1, rng)]
    end = X.ends(rows)
    at_cut = [t for t, e in end.items() if e == cut]
    below = [t for t, e in end.items() if e == cut - 1]
    assert 0 in at_cut and U64 in below and len(at_cut) > 1 and len(below) > 1
    store = make()
    observe_rows(store, split(rows, 5, seed=1))
    assert store.info()["segments"] == 5
    absent = [int(ids[5]) ^ 1, 12345]
    left = expire_and_check(store, make, rows, cut, extra=absent)
    assert 0 < len(left) < len(rows) and set(at_cut) <= {r[0] for r in left}  # end == cut stays
    assert not set(below) & {r[0] for r in left}                               # end == cut - 1 goes
    assert store.info()["segments"] == 1
    left2 = expire_and_check(store, make, left, cut + 1, extra=absent)
    assert not set(at_cut) & {r[0] for r in left2} and 0 < len(left2) < len(left)
    assert expire_and_check(store, make, left2, cut + 1) == left2  # nothing more goes


# ---- 2. a trace across three segments ------------------------------------------------------------------------
@pytest.mark.parametrize("cut,stays", [(100, True), (101, False)], ids=("end_at_cut", "one_above"))
def test_a_trace_across_three_segments(make, cut, stays):
    t, other = R.id_in_bucket(77, 0), R.id_in_bucket(77, 1)
    segs = [[row(t, 10), row(t, 20), row(other, 100), row(5, 500)],
            [row(t, 30), row(t, 100), row(other, 10), row(6, 50)],   # the trace's maximum lies here only
            [row(7, 100), row(t, 40), row(t, MIN), row(8, 101)]]
    rows = [r for s in segs for r in s]
    store = make()
    observe_rows(store, segs)
    assert store.info()["segments"] == 3
    left = expire_and_check(store, make, rows, cut, extra=[9])
    assert sum(r[0] == t for r in left) == (6 if stays else 0)


# ---- 3. the bounds of ts -------------------------------------------------------------------------------------
def test_ts_bounds(make):
    low, top, mid = 11, U64, 0
    rows = [row(low, MIN, span=1), row(low, MIN, span=2), row(top, MAX), row(top, 3), row(mid, 5), row(13, MAX - 1), row(14, MIN + 1)]

    def fresh_store():
        s = make()
        observe_rows(s, split(rows, 2, seed=3))
        return s

    # an INT64_MIN-only trace stays at INT64_MIN when a pin on another trace sends the call through the passes
    assert expire_and_check(fresh_store(), make, rows, MIN, pins={mid: 5}) == rows
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, MIN, pins={mid: 6})} == {low, top, 13, 14}
    assert expire_and_check(fresh_store(), make, rows, MIN, pins={999: 0}) == rows
    store = fresh_store()
    left = expire_and_check(store, make, rows, MIN + 1)  # it goes at INT64_MIN + 1
    assert {r[0] for r in left} == {top, mid, 13, 14}
    left = expire_and_check(store, make, left, MIN + 2)
    assert {r[0] for r in left} == {top, mid, 13}
    # an end at INT64_MAX is the table's all ones, the mark of a pinned trace: it stays at INT64_MAX without
    # pins, with an unrelated pin (present and absent), and when it is itself pinned at INT64_MAX
    for pins in (None, {13: MIN}, {13: MAX}, {999: MIN}, {top: MAX}, {top: MAX, mid: MIN}):
        left = expire_and_check(fresh_store(), make, rows, MAX, pins=pins)
        want = {top} | ({13} if pins == {13: MIN} else set()) | ({mid} if pins and mid in pins else set())
        assert {r[0] for r in left} == want, pins
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, 0, pins={top: MAX})} == {top, mid, 13}


# ---- 4. INT64_MIN without pins -------------------------------------------------------------------------------
def test_int64_min_without_pins_changes_nothing(make):
    rows = [row(t % 50, t % 17 - 8) for t in range(400)] + [row(77, MIN)]
    store = make()
    observe_rows(store, split(rows, 3, seed=4))
    before = store.info()
    assert store.expire(MIN) == 0 and store.expire(MIN, {}) == 0
    assert store.info() == before and before["segments"] == 3 and before["entries"] == len(rows)
    same_as_fresh(store, make, rows, list(range(52)) + [77])
    empty = make()
    assert empty.expire(0) == 0 and empty.expire(MAX, {5: MIN}) == 0
    assert empty.info() == {"entries": 0, "segments": 0, "bytes": 0}


# ---- 5. word and stretch edges -------------------------------------------------------------------------------
EDGES = [(n, "alternate") for n in (63, 64, 65, STRETCH - 1, STRETCH, STRETCH + 1)] + \
        [(n, m) for n in (63, 64, 65) for m in ("all_go", "all_stay")]


@pytest.mark.parametrize("n,mode", EDGES, ids=lambda v: str(v))
def test_word_and_stretch_edges(make, n, mode):
    """Bucket 500 holds n rows behind bucket 499's one row, every bucket a range of its own (expire_chunk=1): the
    big slice is [1, n + 1), off the mark words' boundaries at both ends."""
    lone = R.id_in_bucket(499, 0)
    traces = [R.id_in_bucket(500, k) for k in range(6)]
    assert R.bucket(lone) == 499 and {R.bucket(t) for t in traces} == {500}
    if mode == "alternate":  # neighbours go and stay in turn: mixed words; then a run that goes and one that stays
        which = [i % 6 for i in range(n)]
        if n > 1000:
            which[300:500] = [1] * 200
            which[600:800] = [2] * 200
        ts = [50 if k % 2 else 150 for k in which]
    else:
        which = [i % 6 for i in range(n)]
        ts = [50 if mode == "all_go" else 150] * n
    rows = [row(lone, 150 if mode == "all_go" else 50)] + bulk([traces[k] for k in which], ts, seed=n)
    store = make(expire_chunk=1)
    observe_rows(store, [rows])
    left = expire_and_check(store, make, rows, 100, extra=[R.id_in_bucket(500, 6), R.id_in_bucket(501, 0)])
    if mode == "alternate":
        assert {r[0] for r in left} == {traces[0], traces[2], traces[4]} and 0 < len(left) < n
    else:
        assert len(left) == (1 if mode == "all_go" else n)


# ---- 6. the run fold -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut,stays", [(900, True), (901, False)], ids=("stays", "goes"))
def test_a_long_run_with_its_maximum_inside(make, cut, stays):
    n, at = 20000, 12345
    assert n > STRETCH and at % 64 not in (0, 63)
    long_id, other = R.id_in_bucket(9, 0), R.id_in_bucket(9, 1)
    rng = np.random.default_rng(5)
    ts = rng.integers(0, 900, n).tolist()
    ts[at] = 900  # the trace's one maximum, at a lane that is not its run's first
    rows = bulk([long_id] * n, ts, seed=5) + bulk([other] * 300, [950] * 300, seed=6)
    store = make()
    observe_rows(store, [rows])
    left = expire_and_check(store, make, rows, cut, extra=[R.id_in_bucket(9, 2)])
    assert sum(r[0] == long_id for r in left) == (n if stays else 0) and sum(r[0] == other for r in left) == 300


def test_runs_of_length_one_and_a_run_across_a_wave_row(make):
    a, b, c, d, e = (R.id_in_bucket(2000, k) for k in range(5))
    # consecutive rows alternate between two traces of one bucket; each trace's maximum is one row in the middle
    ts_alt = [10] * 300
    ts_alt[150], ts_alt[151] = 100, 99
    alt = bulk([a, b] * 150, ts_alt, seed=1)
    # runs of 40, 50 and 100 rows: the middle one lies across the 64-entry boundary, its maximum is its last row
    ts_run = [10] * 190
    ts_run[89] = 100
    ts_run[40 + 189 - 89] = 99
    run = bulk([c] * 40 + [d] * 50 + [e] * 100, ts_run, seed=2)
    for rows in (alt, run, alt + run):
        store = make()
        observe_rows(store, [rows])
        left = expire_and_check(store, make, rows, 100)
        assert {r[0] for r in left} == {a, d} & {r[0] for r in rows}


# ---- 7. ranges -----------------------------------------------------------------------------------------------
def ranged_rows():
    rng = np.random.default_rng(7)
    big = [R.id_in_bucket(3000, k) for k in range(10)]       # 200 rows in one bucket: above the chunk of 64
    spread = np.unique(rng.integers(0, 2 ** 64, 300, dtype=np.uint64)).tolist()
    rows = [row(t, int(rng.integers(0, 100)), rng) for t in big for _ in range(20)]
    rows += [row(t, int(rng.integers(0, 100)), rng) for t in spread for _ in range(int(rng.integers(1, 5)))]
    lo, hi = min(spread, key=R.bucket), max(spread, key=R.bucket)
    assert R.bucket(lo) < 1000 and R.bucket(hi) > 3000 and len(rows) > 4 * 64
    pins = {lo: MAX, hi: MIN, big[0]: MIN, big[1]: MAX, spread[7]: MIN, 31337: MIN}  # in different ranges, and an absent id
    return rows, pins, big


def test_ranges(make):
    rows, pins, big = ranged_rows()
    cut = int(np.median(list(X.ends(rows).values())))
    lefts = []
    for chunk in (64, 0):  # many ranges, the big bucket one of its own; then one range
        store = make(expire_chunk=chunk)
        observe_rows(store, split(rows, 3, seed=7))
        lefts.append(expire_and_check(store, make, rows, cut, pins=pins, extra=[R.id_in_bucket(3000, 10)]))
        assert 0 < len(lefts[-1]) < len(rows)
        assert sum(r[0] == big[0] for r in lefts[-1]) == 20 and big[1] not in {r[0] for r in lefts[-1]}
    assert lefts[0] == lefts[1] != X.survivors(rows, cut)


# ---- 8. a skewed store ---------------------------------------------------------------------------------------
def test_a_skewed_store(make):
    rng = np.random.default_rng(6)
    heavy = [R.id_in_bucket(1234, k) for k in range(300)]
    spread = np.unique(rng.integers(0, 2 ** 64, 400, dtype=np.uint64)).tolist()
    tids = np.repeat(np.array(heavy, np.uint64), 20).tolist() + [t for t in spread for _ in range(int(rng.integers(1, 7)))]
    rows = bulk(tids, rng.integers(0, 100, len(tids)).tolist(), seed=8)
    assert sum(r[0] in set(heavy) for r in rows) == 6000 and len(rows) > 6000 + 1024
    cut = int(np.median(list(X.ends(rows).values())))
    store = make(expire_chunk=1024)  # the big bucket above the chunk, the rest in several ranges
    observe_rows(store, split(rows, 3, seed=6))
    left = expire_and_check(store, make, rows, cut, pins={heavy[0]: MIN, heavy[1]: MAX, spread[0]: MIN}, extra=[R.id_in_bucket(1234, 300)])
    assert 0 < len(left) < len(rows)


# ---- 9., 10. 64 segments -------------------------------------------------------------------------------------
def test_64_time_sorted_segments(make):
    rng = np.random.default_rng(9)
    segs = [[row(1000 * k + t, 100 * k + int(rng.integers(0, 100)), rng) for t in range(20) for _ in range(2)] for k in range(64)]
    for k in range(64):
        segs[k][0] = segs[k][0][:2] + (100 * k + 99,) + segs[k][0][3:]  # trace 1000 k ends at the segment's top
    rows = [r for s in segs for r in s]
    store = make()
    observe_rows(store, segs)
    before = store.info()
    per_segment = before["bytes"] // 64
    assert before["segments"] == 64 and before["bytes"] == 64 * per_segment  # (equal sizes: equal bytes)
    cut = 100 * 20 + 50
    left = expire_and_check(store, make, rows, cut)
    after = store.info()
    # 20 segments freed whole, the 21st rewritten, 43 untouched: their bytes are still there
    assert after["segments"] == 44 and 0 < len(left) - 43 * 40 < 40
    assert 43 * per_segment < after["bytes"] <= 44 * per_segment
    # a cut between two segments: old ones freed, nothing rewritten, the bytes those of the untouched ones
    cut2 = 100 * 30
    left2 = expire_and_check(store, make, left, cut2)
    assert len(left2) == 34 * 40 and store.info()["segments"] == 34 and store.info()["bytes"] == 34 * per_segment


def test_64_segments_each_half_expiring_then_observe_and_expire_again(make):
    rng = np.random.default_rng(10)
    segs = [[row(1000 * k + t, (0 if t % 2 else 100) + int(rng.integers(0, 50)), rng) for t in range(16) for _ in range(3)]
            for k in range(64)]
    rows = [r for s in segs for r in s]
    store = make()
    observe_rows(store, segs)
    assert store.info()["segments"] == 64
    left = expire_and_check(store, make, rows, 100)
    assert store.info()["segments"] == 1 and 0 < len(left) < len(rows)
    # 14. a later observe of older rows enters the store again (the cut is made once), and goes at the next cut
    again = segs[0] + [row(77777, 5), row(1000, 150)]  # (trace 1 went with the first cut)
    observe_rows(store, [again])
    rows2 = left + again
    assert store.info()["segments"] == 2
    same_as_fresh(store, make, rows2, sorted({r[0] for r in rows2}))
    assert len(store.getAnnotationsByTraceIds([1])[0]) == 3  # an expired trace's rows are back
    left2 = expire_and_check(store, make, rows2, 100)
    assert store.info()["segments"] <= 2 and not {77777, 1} & {r[0] for r in left2} and len(left2) > len(left)


# ---- 11. pins ------------------------------------------------------------------------------------------------
def raw_expire(store, min_end, ids, cuts):
    ids, cuts, removed = np.array(ids, np.uint64), np.array(cuts, np.int64), C.c_uint64(77)
    st = store._L.zk_an_expire(store._h, min_end, ids.ctypes.data, cuts.ctypes.data, len(ids), C.byref(removed))
    return st, int(removed.value)


def test_pins(make):
    a, b, c, d, e, f = 21, 22, 0, 24, 25, U64
    rows = [row(a, 10), row(a, 3), row(b, 60), row(b, -61), row(c, MIN), row(d, 100), row(e, 20), row(f, MAX), row(f, 1)]
    ids = [a, b, c, d, e, f]

    def fresh_store():
        s = make()
        observe_rows(s, split(rows, 2, seed=8))
        return s

    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, 50, {a: 5})} == {a, b, d, f}     # below the default, pinned: stays
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, 50, {a: 11})} == {b, d, f}       # the pin is a cutoff too
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, 50, {b: 61})} == {d, f}          # a higher pin: its trace alone
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, MIN, {b: 61})} == {a, c, d, e, f}
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, 50, {c: MIN})} == {b, c, d, f}   # id 0, its end at the floor
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, 50, {c: MIN + 1})} == {b, d, f}
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, MAX, {f: MAX, d: 100, e: 21})} == {d, f}
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, 50, {404: MIN, 405: MAX})} == {b, d, f}  # absent ids
    # given unsorted (descending ids)
    assert {r[0] for r in expire_and_check(fresh_store(), make, rows, 50, {f: MAX, e: 20, b: 61, a: MIN, c: MIN})} == {a, c, d, e, f}
    # a duplicated pin, too many pins: refused, the store unchanged
    store = fresh_store()
    before = store.info()
    assert raw_expire(store, 50, [a, b, a], [1, 2, 3]) == (_abi.ZK_ERR_INVALID_ARG, 0)
    n = _abi.ZK_AN_MAX_PINS + 1
    assert raw_expire(store, 50, list(range(1000, 1000 + n)), [0] * n) == (_abi.ZK_ERR_INVALID_ARG, 0)
    with pytest.raises(ValueError):
        store.expire(50, {1000 + i: 0 for i in range(n)})
    assert store.info() == before
    same_as_fresh(store, make, rows, ids)


def test_4096_pins_in_one_call(make):
    rng = np.random.default_rng(11)
    ids = np.unique(rng.integers(0, 2 ** 64, 3000, dtype=np.uint64)).tolist()
    rows = [row(t, int(rng.integers(0, 100)), rng) for t in ids for _ in range(int(rng.integers(1, 4)))]
    pins = {t: int(rng.integers(0, 100)) for t in ids[:2500]}
    pins.update({int(x): MIN for x in rng.integers(0, 2 ** 64, 4096 - len(pins), dtype=np.uint64) if int(x) not in set(ids)})
    assert len(pins) == _abi.ZK_AN_MAX_PINS
    store = make()
    observe_rows(store, split(rows, 3, seed=9))
    left = expire_and_check(store, make, rows, 50, pins)
    assert left != X.survivors(rows, 50) and 0 < len(left) < len(rows)


# ---- 12. the invariant with the span store -------------------------------------------------------------------
def test_the_span_store_holds_the_same_traces(make, gpu):
    spans = gen_traces(31, 60, max_depth=4)
    blobs = encode_all(spans, True)
    assert 200 < len(blobs) < 2000
    dec = SpanDecoder()
    parts = [blobs[k::3] for k in range(3)]  # three batches, every trace spread over all of them
    sp_rows, an_rows = [], []
    annots = make()
    made = []

    def span_store(rows_batches):
        made.append(TraceSpanStore(device=gpu))
        for b in rows_batches:
            made[-1].observe(S.cols_of(b))
        return made[-1]

    try:
        batches = []
        for p in parts:
            cols, rej, rows = dec.decode_annotated(p, row_cap=16 * len(p))
            assert rej == 0
            batches.append(S.rows_of(cols))
            sp_rows += batches[-1]
            an_rows += rows.rows()
            annots.observe(rows)
        store = span_store(batches)
        sp_end, an_end = SX.ends(sp_rows), X.ends(an_rows)
        assert an_end == {t: e for t, e in sp_end.items() if t in an_end} and len(an_end) == 60  # the decoder's last = max ts
        order = sorted(an_end, key=an_end.get)
        old, young = order[3], order[-3]
        ttl = 3600
        now = an_end[order[30]] + ttl * 1_000_000  # the default cutoff: the median end
        ret = SpanRetention(ttl_seconds=ttl, spans=store, annotations=annots)
        ret.setTimeToLive(old, 2 * 3600)  # a pin that keeps an old trace
        ret.setTimeToLive(young, 1)       # a pin that removes a young one
        pins = {old: now - 2 * 3600 * 1_000_000, young: now - 1_000_000}
        cut = now - ttl * 1_000_000
        sp_left, an_left = SX.survivors(sp_rows, cut, pins), X.survivors(an_rows, cut, pins)
        out = ret.expire(now)
        assert out == {"cutoff": cut, "spans": len(sp_rows) - len(sp_left), "annotations": len(an_rows) - len(an_left)}
        ids = sorted(sp_end) + [404]
        held = {i for i, rows in zip(ids, annots.getAnnotationsByTraceIds(ids)) if rows}
        alive = store.tracesExist(ids)
        assert held == {r[0] for r in an_left} == alive & set(an_end) == alive  # (every generated span has annotations)
        assert old in held and young not in held and 25 <= len(held) <= 35
        same_as_fresh(annots, make, an_left, ids)
        # the answers built over both stores equal those of a fresh pair fed only the survivors
        fresh_an = make()
        observe_rows(fresh_an, [an_left])
        fresh_sp = span_store([sp_left])
        sums = store.getTraceSummariesByIds(ids, adjust=("TIME_SKEW",), annotations=annots)
        assert sums == fresh_sp.getTraceSummariesByIds(ids, adjust=("TIME_SKEW",), annotations=fresh_an)
        assert [s.trace_id for s in sums] == [i for i in ids if i in held]
        lines = store.getTraceTimelinesByIds(ids, adjust=("TIME_SKEW",), annotations=annots)
        assert lines == fresh_sp.getTraceTimelinesByIds(ids, adjust=("TIME_SKEW",), annotations=fresh_an)
        assert len(lines) == len(held) and all(t.annotations for t in lines)
    finally:
        for s in made:
            s.close()


# ---- 13. timing ----------------------------------------------------------------------------------------------
def test_expire_ms(make):
    rows = [row(t % 100, t % 40) for t in range(3000)]
    store = make(timing=True)
    with pytest.raises(ZkError):
        store.expire_ms()
    observe_rows(store, split(rows, 2, seed=11))
    for cut in (20, 20):  # a rewrite, then an expiry where nothing goes
        store.expire(cut)
        ms = store.expire_ms()
        assert tuple(ms) == TraceAnnotationStore.EXPIRE_PHASES and all(np.isfinite(v) and v >= 0 for v in ms.values())
    assert store.expire(MIN) == 0  # no pass: no timing to read
    with pytest.raises(ZkError):
        store.expire_ms()
    plain = make()
    observe_rows(plain, [rows])
    plain.expire(20)
    with pytest.raises(ZkError) as e:
        plain.expire_ms()
    assert e.value.status == _abi.ZK_ERR_INVALID_ARG
