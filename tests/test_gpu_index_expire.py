"""Index retention on the device: zk_ix_expire, zk_ax_expire, zk_td_expire and IndexRetention
(include/zkindex.h, zkannindex.h, zkduration.h "Expiry"; zipkin_amd/retention.py).

The expected answers are those of the existing reference models (tests/ixref.py, axref.py, tdref.py) run
on the FILTERED entries: after expire(c) a handle must answer every existing query as a fresh handle that
observed only the survivors. Every comparison is exact equality; nothing depends on the order inside a
service's slice."""
import numpy as np
import pytest

from oracle.spans import Annotation, BinaryAnnotation, Endpoint, Span
from tests import axref, ixref, tdref, thriftenc
from zipkin_amd import (AnnotationItems, DeviceAnnotationItems, DeviceColumns, IndexRetention, TraceAnnotationIndex,
                        TraceDurationIndex, TraceNameIndex, ZkError, _abi)
from zipkin_amd.ingest import SpanDecoder

pytestmark = pytest.mark.gpu

T0 = 1_400_000_000_000_000
U64 = 2 ** 64 - 1
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
KEYS = (0x1111, U64, 0)          # annotation key hashes of the ax batches
VALS = (0, 0x77, U64)            # 0: a time annotation; odd: a binary annotation's value hash


def some_ids(seed, n):
    """n distinct traceIds spread over 64 bits, 0 and 2^64 - 1 among them (test_gpu_trace_index.py's)."""
    ids = np.unique(np.random.default_rng(seed).integers(1, 2 ** 64 - 1, 2 * n, dtype=np.uint64))[:n]
    np.random.default_rng(seed + 1).shuffle(ids)
    ids[0], ids[1] = 0, U64
    return ids


# ---- the two segment indices behind one face ---------------------------------------------------------------
class Ix:
    """TraceNameIndex: a batch is SpanColumns, an entry (service, name, ts, trace_id)."""
    TS = 2

    @staticmethod
    def make(gpu, S, **kw):
        return TraceNameIndex(S, device=gpu, **kw)

    @staticmethod
    def batch(svc, ts, tid, seed=0):
        return ixref.batch(svc, np.random.default_rng(seed).integers(0, 4, len(tid)), ts, tid, seed=seed)

    @staticmethod
    def observe(idx, b):
        idx.observe(DeviceColumns.from_host(b))

    @staticmethod
    def entries(b, S):
        return ixref.entries_of(b, S)

    @staticmethod
    def check_service(idx, e, s, mid):
        for name, end, limit in ((ixref.ANY, INT64_MAX, 4096), (ixref.ANY, INT64_MAX, 7), (1, mid, 50), (3, INT64_MIN, 5)):
            got = idx.getTraceIdsByName(s, name, end, limit)
            rows, matched = ixref.trace_ids(e, s, name, end, limit)
            assert [tuple(t) for t in got] == rows and idx.matched == matched, (s, name, end, limit)
        assert idx.getSpanNames(s) == set(ixref.span_names(e, s)), s

    @staticmethod
    def service_counts(e, S):
        return ixref.service_counts(e, S).tolist()


class Ax:
    """TraceAnnotationIndex: a batch is AnnotationItems, an entry (service, key, val, ts, trace_id)."""
    TS = 3

    @staticmethod
    def make(gpu, S, **kw):
        return TraceAnnotationIndex(S, device=gpu, **kw)

    @staticmethod
    def batch(svc, ts, tid, seed=0):
        rng = np.random.default_rng(seed)
        n = len(tid)
        svc = np.broadcast_to(np.asarray(svc, np.uint32), (n,))
        ts = np.broadcast_to(np.asarray(ts, np.int64), (n,))
        return AnnotationItems(svc, np.array(KEYS, np.uint64)[rng.integers(0, 3, n)], np.array(VALS, np.uint64)[rng.integers(0, 3, n)],
                               ts, np.asarray(tid, np.uint64))

    @staticmethod
    def observe(idx, b):
        idx.observe(DeviceAnnotationItems.from_host(b, idx.device))

    @staticmethod
    def entries(b, S):
        return b.rows()

    @staticmethod
    def check_service(idx, e, s, mid):
        for key, val, end, limit in ((KEYS[0], axref.ANY, INT64_MAX, 4096), (KEYS[1], axref.ANY, INT64_MAX, 7),
                                     (KEYS[2], VALS[1], mid, 50), (KEYS[0], VALS[2], INT64_MIN, 5)):
            got, matched = idx.trace_ids(s, key, val, end, limit)
            rows, want = axref.trace_ids(e, s, key, val, end, limit)
            assert [tuple(t) for t in got] == rows and matched == want, (s, key, val, end, limit)

    @staticmethod
    def service_counts(e, S):
        return np.bincount(np.array([x[0] for x in e], np.int64), minlength=S).tolist()


KINDS = pytest.mark.parametrize("K", (Ix, Ax), ids=("ix", "ax"))


@pytest.fixture()
def make(gpu):
    made = []

    def factory(K, S, **kw):
        made.append(K.make(gpu, S, **kw))
        return made[-1]

    yield factory
    for idx in made:
        idx.close()


def survivors(K, e, cut):
    return [x for x in e if x[K.TS] >= cut]


def check(K, idx, e, S, services=None, mid=T0):
    """Every existing query of the handle against the reference over the entries e."""
    counts = K.service_counts(e, S)
    assert idx.service_counts().tolist() == counts
    assert idx.info()["entries"] == len(e)
    if K is Ix:
        assert idx.getAllServiceNames() == {s for s in range(S) if counts[s]}
    for s in range(S) if services is None else services:
        K.check_service(idx, e, s, mid)


def expire(K, idx, e, cut):
    """idx.expire(cut) with its removed count checked; returns the surviving entries."""
    left = survivors(K, e, cut)
    assert idx.expire(cut) == len(e) - len(left)
    return left


# ---- 1. general cases: the ends of int64, the cut at an occurring ts, equal entries ---------------------------
@KINDS
def test_cutoffs_at_the_ends_and_at_an_occurring_ts(make, K):
    S = 4
    rng = np.random.default_rng(1)
    n = 600
    ts = T0 + rng.integers(0, 40, n)
    ts[:6] = [INT64_MIN, INT64_MIN, INT64_MAX, INT64_MAX, -1, 0]
    tid = some_ids(2, n)
    tid[2], tid[3], tid[4], tid[5] = 0, U64, 0, U64  # the extreme ids at the extreme times too
    svc = rng.integers(0, S, n)
    b = K.batch(svc, ts, tid, seed=3)
    triple = K.batch([1, 2], [T0 + 20, T0 + 19], [0xABCDEF, 0xABCDEF], seed=4)  # a pair entered three times, at the cut and below it
    idx = make(K, S)
    K.observe(idx, b)
    for _ in range(3):
        K.observe(idx, triple)
    e = K.entries(b, S) + 3 * K.entries(triple, S)
    check(K, idx, e, S, mid=T0 + 20)
    before = idx.info()
    e = expire(K, idx, e, INT64_MIN)  # removes nothing: nothing is rewritten or reallocated
    assert idx.info() == before and len(e) == n + 6
    check(K, idx, e, S, mid=T0 + 20)
    e = expire(K, idx, e, T0 + 20)    # a ts that occurs: kept, all three copies of the pair at it too
    assert sum(1 for x in e if x[K.TS] == T0 + 20) >= 4 and not any(x[K.TS] == T0 + 19 for x in e)
    assert sum(1 for x in e if x[-1] == 0xABCDEF) == 3  # all copies stay, all copies below the cut went
    assert idx.info()["segments"] == 1                  # four mixed segments became one
    check(K, idx, e, S, mid=T0 + 25)
    e = expire(K, idx, e, T0 + 21)    # that ts + 1: removed
    assert not any(x[K.TS] == T0 + 20 for x in e) and not any(x[-1] == 0xABCDEF for x in e)
    check(K, idx, e, S, mid=T0 + 25)
    e = expire(K, idx, e, INT64_MAX)  # keeps only the entries at exactly INT64_MAX
    assert len(e) == 2 and {x[-1] for x in e} == {0, U64}
    check(K, idx, e, S)
    assert idx.expire(INT64_MAX) == 0 and idx.info()["entries"] == 2


@KINDS
def test_an_empty_handle_and_everything_expiring(make, K):
    idx = make(K, 3)
    assert idx.expire(0) == 0 and idx.expire(INT64_MAX) == 0
    assert idx.info() == {"entries": 0, "segments": 0, "bytes": 0}
    b = K.batch([0, 2, 2], [T0, T0 + 1, T0 + 2], [7, 8, 9])
    K.observe(idx, b)
    assert idx.expire(T0 + 3) == 3
    assert idx.info() == {"entries": 0, "segments": 0, "bytes": 0} and idx.service_counts().tolist() == [0, 0, 0]
    check(K, idx, [], 3)
    assert idx.expire(0) == 0
    K.observe(idx, b)  # the handle goes on working
    check(K, idx, K.entries(b, 3), 3)


# ---- 2. segment sizes and service layouts ---------------------------------------------------------------------
def layout(name, n, rng):
    """(S, service ids of n entries, the services worth asking)."""
    if name == "S5":
        return 5, rng.integers(0, 5, n), None
    if name == "two_ends":  # S = 4096 with only services 0 and 4095 populated
        return 4096, np.where(rng.integers(0, 2, n) == 0, 0, 4095), (0, 4095, 1, 2047, 4094)
    assert name == "last_only"  # S = 4096 with only service 4095 populated
    return 4096, np.full(n, 4095), (4095, 0, 4094)


@KINDS
@pytest.mark.parametrize("lay", ("S5", "two_ends", "last_only"))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 1025, 4097, 40_000))
def test_segment_sizes(make, K, lay, n):
    """Three segments of n entries with interleaved timestamps: all are mixed and become one. 1025 and
    4097 cross the 1024-entry counting tile; 40 000 is past the 16384-entry stretch of a workgroup, so
    several workgroups share a service's cursor."""
    rng = np.random.default_rng(n)
    S, svc, ask = layout(lay, 3 * n, rng)
    span = 1000
    ts = T0 + rng.integers(0, span, 3 * n)
    ts[0:3 * n:n] = T0          # every segment has an entry that goes
    ts[n - 1:3 * n:n] = T0 + span  # and one that stays (n == 1: it stays)
    tid = some_ids(n, 3 * n)
    idx = make(K, S)
    e = []
    for g in range(3):
        b = K.batch(svc[g * n:(g + 1) * n], ts[g * n:(g + 1) * n], tid[g * n:(g + 1) * n], seed=g)
        K.observe(idx, b)
        e += K.entries(b, S)
    assert idx.info()["segments"] == 3
    cut = T0 + span // 2
    e = expire(K, idx, e, cut)
    info = idx.info()
    assert info["segments"] == (3 if n == 1 else 1)  # n == 1: no segment loses anything
    check(K, idx, e, S, ask, mid=T0 + 3 * span // 4)
    idx.compact()
    check(K, idx, e, S, ask, mid=T0 + 3 * span // 4)


@KINDS
@pytest.mark.parametrize("G", (1, 3))
def test_a_tile_that_spans_thousands_of_services(make, K, G):
    """S = 4096 with every service holding 0..3 entries per segment: a workgroup's stretch spans all of them."""
    S = 4096
    idx = make(K, S)
    e = []
    for g in range(G):
        rng = np.random.default_rng(40 + g)
        svc = np.repeat(np.arange(S), rng.integers(0, 4, S))
        n = len(svc)
        perm = rng.permutation(n)
        b = K.batch(svc[perm], T0 + rng.integers(0, 100, n), some_ids(50 + g, n), seed=g)
        K.observe(idx, b)
        e += K.entries(b, S)
    e = expire(K, idx, e, T0 + 50)
    assert idx.info()["segments"] == 1
    check(K, idx, e, S, list(range(0, S, 97)) + [1, 2, 4094, 4095], mid=T0 + 75)
    e = expire(K, idx, e, T0 + 99)  # nearly every service loses its last entries
    check(K, idx, e, S, list(range(0, S, 61)) + [4095], mid=T0 + 99)


# ---- 3. which segments stay, go, and are rewritten --------------------------------------------------------------
@KINDS
@pytest.mark.parametrize("G", (1, 3, 64))
def test_time_disjoint_segments(make, K, G):
    """Segment g holds the timestamps [T0 + 1000 g, T0 + 1000 (g + 1)): a cut inside segment k frees the
    k before it, rewrites segment k alone and leaves the others untouched; a cut on a boundary rewrites
    nothing."""
    S, n = 5, 300
    idx = make(K, S)
    e = []
    for g in range(G):
        rng = np.random.default_rng(100 + g)
        ts = T0 + 1000 * g + rng.integers(0, 1000, n)
        ts[0], ts[1] = T0 + 1000 * g, T0 + 1000 * g + 999
        b = K.batch(rng.integers(0, S, n), ts, some_ids(200 + g, n), seed=g)
        K.observe(idx, b)
        e += K.entries(b, S)
    assert idx.info()["segments"] == G
    k = G // 2
    before = idx.info()
    cut = T0 + 1000 * k + 500
    e = expire(K, idx, e, cut)
    info = idx.info()
    assert info["segments"] == G - k and info["bytes"] < before["bytes"]
    check(K, idx, e, S, mid=T0 + 1000 * k + 700)
    if G > 1:
        cut = T0 + 1000 * (k + 1)
        e = expire(K, idx, e, cut)  # on the boundary: the rewritten segment goes whole, none is mixed
        assert idx.info()["segments"] == G - k - 1
        check(K, idx, e, S, mid=T0 + 1000 * (k + 1) + 500)
    before = idx.info()
    assert idx.expire(cut) == 0 and idx.info() == before  # nothing expires: nothing changes


@KINDS
@pytest.mark.parametrize("G", (1, 3, 64))
def test_interleaved_segments_become_one(make, K, G):
    S, n = 5, 257
    idx = make(K, S)
    e = []
    for g in range(G):
        rng = np.random.default_rng(300 + g)
        ts = T0 + rng.integers(0, 1000, n)
        ts[0], ts[1] = T0, T0 + 999
        b = K.batch(rng.integers(0, S, n), ts, some_ids(400 + g, n), seed=g)
        K.observe(idx, b)
        e += K.entries(b, S)
    # two segments more that lose nothing: they are kept untouched beside the rewritten one
    for g in range(2 if G < 64 else 0):
        b = K.batch(np.arange(20) % S, T0 + 5000 + np.arange(20), some_ids(500 + g, 20), seed=g)
        K.observe(idx, b)
        e += K.entries(b, S)
    kept = idx.info()["segments"] - G
    e = expire(K, idx, e, T0 + 500)
    assert idx.info()["segments"] == 1 + kept
    check(K, idx, e, S, mid=T0 + 750)


@KINDS
def test_bytes_fall_when_half_of_a_large_segment_expires(make, K):
    S, n = 5, 40_000
    rng = np.random.default_rng(7)
    ts = T0 + np.arange(n) % 1000
    b = K.batch(rng.integers(0, S, n), ts, some_ids(8, n), seed=9)
    idx = make(K, S)
    K.observe(idx, b)
    e = K.entries(b, S)
    before = idx.info()
    assert idx.expire(T0) == 0 and idx.info() == before  # nothing expires: bytes, segments and entries unchanged
    e = expire(K, idx, e, T0 + 500)
    after = idx.info()
    assert after["entries"] == n // 2 and after["segments"] == 1 and after["bytes"] < before["bytes"]
    assert after["bytes"] <= before["bytes"] // 2 + 1024  # sized for the survivors (256-B column alignment)
    check(K, idx, e, S, mid=T0 + 750)


# ---- 4. a sequence: older data observed again, a second cut, a compaction ---------------------------------------
@KINDS
def test_observe_expire_observe_older_expire_compact(make, K):
    S = 6
    rng = np.random.default_rng(11)
    mk = lambda lo, hi, n, seed: K.batch(rng.integers(0, S, n), T0 + rng.integers(lo, hi, n), some_ids(seed, n), seed=seed)  # noqa: E731
    new, old, newer = mk(0, 1000, 5000, 12), mk(0, 400, 3000, 13), mk(900, 2000, 2000, 14)
    idx = make(K, S)
    K.observe(idx, new)
    K.observe(idx, old)
    e = K.entries(new, S) + K.entries(old, S)
    e = expire(K, idx, e, T0 + 500)
    check(K, idx, e, S, mid=T0 + 600)
    K.observe(idx, old)    # expiry is a one-time cut: older data enters again
    K.observe(idx, newer)
    e = e + K.entries(old, S) + K.entries(newer, S)
    assert idx.info()["segments"] == 3
    check(K, idx, e, S, mid=T0 + 300)
    e = expire(K, idx, e, T0 + 200)  # `old` is mixed, the two others lose nothing
    assert idx.info()["segments"] == 3
    check(K, idx, e, S, mid=T0 + 300)
    idx.compact()
    assert idx.info()["segments"] == 1
    check(K, idx, e, S, mid=T0 + 300)
    e = expire(K, idx, e, T0 + 950)  # the merged segment is mixed
    assert idx.info()["segments"] == 1
    check(K, idx, e, S, mid=T0 + 1500)


def test_names_disappear_with_their_entries(make):
    services, span_names = ["web", "db", "cache"], ["get", "put", "scan"]
    #                 web: get old, put new | db: scan old only | cache: get new
    b = ixref.batch([0, 0, 0, 1, 1, 2], [1, 2, 1, 3, 3, 1], [T0, T0 + 9, T0 + 1, T0 + 2, T0 + 3, T0 + 9], [1, 2, 3, 4, 5, 6])
    idx = make(Ix, 3, services=services, span_names=span_names)
    Ix.observe(idx, b)
    assert idx.getSpanNames("web") == {"get", "put"} and idx.getAllServiceNames() == {"web", "db", "cache"}
    assert idx.expire(T0 + 5) == 4
    assert idx.getSpanNames("web") == {"put"} and idx.getSpanNames("db") == set() and idx.getSpanNames("cache") == {"get"}
    assert idx.getAllServiceNames() == {"web", "cache"}
    assert idx.getTraceIdsByName("db", None, INT64_MAX, 10) == [] and idx.matched == 0
    assert [tuple(t) for t in idx.getTraceIdsByName("web", None, INT64_MAX, 10)] == [(2, T0 + 9)]


@KINDS
def test_the_65th_observe_after_an_expiry_still_merges(make, K):
    S = 4
    idx = make(K, S)
    e, k = [], 0

    def add(count, lo):
        nonlocal e, k
        for _ in range(count):
            rng = np.random.default_rng(600 + k)
            n = 30 + k % 9
            b = K.batch(rng.integers(0, S, n), T0 + lo + rng.integers(0, 1000, n), some_ids(700 + k, n), seed=k)
            K.observe(idx, b)
            e += K.entries(b, S)
            k += 1

    add(64, 0)
    assert idx.info()["segments"] == 64
    e = expire(K, idx, e, T0 + 500)
    assert idx.info()["segments"] == 1
    add(63, 2000)
    assert idx.info()["segments"] == 64
    add(1, 2000)  # the 65th: the 64 are merged first
    assert idx.info()["segments"] == 2
    check(K, idx, e, S, mid=T0 + 2500)
    e = expire(K, idx, e, T0 + 2500)
    assert idx.info()["segments"] == 1
    check(K, idx, e, S, mid=T0 + 2750)


@KINDS
def test_expire_timing(make, K):
    S = 3
    b = K.batch(np.arange(5000) % S, T0 + np.arange(5000), some_ids(21, 5000))
    t = make(K, S, timing=True)
    with pytest.raises(ZkError):
        t.expire_ms()
    K.observe(t, b)
    assert t.expire(T0 + 2500) == 2500
    ms = t.expire_ms()
    assert set(ms) == {"count", "size", "rewrite"} and all(v >= 0 for v in ms.values())
    assert t.expire(T0) == 0 and set(t.expire_ms()) == {"count", "size", "rewrite"}
    plain = make(K, S)
    K.observe(plain, b)
    plain.expire(T0 + 1)
    with pytest.raises(ZkError) as err:
        plain.expire_ms()
    assert err.value.status == _abi.ZK_ERR_INVALID_ARG


# ---- 5. the duration table ---------------------------------------------------------------------------------------
ABSENT = np.array([3, 5, 2 ** 63, U64 - 1], np.uint64)


@pytest.fixture()
def h(gpu):
    with TraceDurationIndex(device=gpu) as idx:
        yield idx


def sizing(traces):
    slots = 1024
    while slots < 2 * traces:
        slots *= 2
    return slots


def check_td(h, table, ids, ks=(1, 64)):
    """lookup over `ids`, top in all four orders, and the trace count against the reference table."""
    ids = np.unique(np.concatenate([np.asarray(ids, np.uint64), ABSENT]))
    s, d, found = h.lookup(ids)
    for i, tid in enumerate(ids.tolist()):
        assert bool(found[i]) == (tid in table), tid
        if tid in table:
            assert (int(s[i]), int(d[i])) == (table[tid][0], tdref.duration(*table[tid])), tid
    assert h.info()["traces"] == len(table)
    for order in tdref.ORDERS:
        for k in ks:
            assert [tuple(t) for t in h.top(order, k)] == tdref.top(table, order, k), (order, k)
            assert h.matched == len(table)
    lo, hi = T0 + 100, T0 + 600
    assert [tuple(t) for t in h.top("duration-desc", 20, lo, hi)] == tdref.top(table, "duration-desc", 20, lo, hi)


def expire_td(h, table, cut):
    left = {t: v for t, v in table.items() if v[1] >= cut}
    slots = h.info()["slots"]
    assert h.expire(cut) == len(table) - len(left)
    assert h.info()["slots"] == (slots if len(left) == len(table) else sizing(len(left)))
    return left


@pytest.mark.parametrize("n", (1, 1000, 5000))
def test_single_fragment_traces(h, n):
    rng = np.random.default_rng(n)
    ids = some_ids(n + 1, max(n, 2))[:n]
    first = T0 + rng.integers(0, 1000, n)
    last = first + rng.integers(0, 1000, n)
    b = tdref.fill(ids, first, last, np.ones(n, bool))
    assert h.expire(0) == 0 and h.info() == {"slots": 0, "traces": 0, "bytes": 0}  # an empty handle
    h.observe(DeviceColumns.from_host(b))
    table = tdref.table_of(b)
    assert h.info()["slots"] == sizing(n)
    before = h.info()
    table = expire_td(h, table, INT64_MIN)
    assert h.info() == before and len(table) == n
    cut = int(np.median(last)) + 1 if n > 1 else int(last[0])
    table = expire_td(h, table, cut)  # about half goes (n == 1: end == cut stays)
    assert len(table) == (1 if n == 1 else int((last >= cut).sum()))
    check_td(h, table, ids)
    table = expire_td(h, table, INT64_MAX)
    assert table == {} and h.info()["traces"] == 0 and h.info()["slots"] == 1024
    check_td(h, table, ids)
    h.observe(DeviceColumns.from_host(b))  # the original batch again restores the original table
    check_td(h, tdref.table_of(b), ids)


def test_a_trace_whose_end_passes_the_cutoff_in_the_second_batch(h):
    n = 2000
    ids = some_ids(31, n)
    rng = np.random.default_rng(32)
    first1 = T0 + rng.integers(0, 500, n)
    b1 = tdref.fill(ids, first1, first1 + rng.integers(0, 100, n), np.ones(n, bool))       # every end < T0 + 600
    late = rng.integers(0, 2, n) == 1
    first2 = T0 + 300 + rng.integers(0, 500, late.sum())
    b2 = tdref.fill(ids[late], first2, T0 + 600 + rng.integers(0, 400, late.sum()), np.ones(late.sum(), bool))  # end >= T0 + 600
    for b in (b1, b2):
        h.observe(DeviceColumns.from_host(b))
    table = tdref.table_of([b1, b2])
    table = expire_td(h, table, T0 + 600)  # `end` decides, not `start`: a trace still receiving fragments stays
    assert set(table) == set(ids[late].tolist())
    check_td(h, table, ids)
    assert all(table[t][0] < T0 + 600 for t in table)
    # idempotent re-observe: the original batches again restore the original table
    for b in (b1, b2):
        h.observe(DeviceColumns.from_host(b))
    check_td(h, tdref.table_of([b1, b2]), ids)
    assert h.info()["slots"] == sizing(n + late.sum())  # (sized for the stayers plus the runs of the last batch)


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_survivors_behind_removed_keys_are_still_found(h, seed):
    """3000 ids in 8192 slots, every other one expiring: with linear probing well over a hundred survivors
    sit behind a removed key, so a delete in place would lose them."""
    n = 3000
    ids = some_ids(seed, n)
    last = T0 + 500 - (np.arange(n) % 2)  # the odd ones end one below the cut
    b = tdref.fill(ids, np.full(n, T0), last, np.ones(n, bool))
    h.observe(DeviceColumns.from_host(b))
    assert h.info()["slots"] == 8192
    table = expire_td(h, tdref.table_of(b), T0 + 500)
    assert len(table) == n // 2 and h.info()["slots"] == 4096
    check_td(h, table, ids)


def test_trace_id_zero_and_all_ones(h):
    mk = lambda end0, end1: tdref.build([(0, [(T0, end0, True)]), (U64, [(T0 + 1, end1, True)]), (9, [(T0, T0 + 50, True)])])  # noqa: E731
    b = mk(T0 + 100, T0 + 10)
    h.observe(b)
    table = expire_td(h, tdref.table_of(b), T0 + 50)  # 0 kept, 2^64 - 1 removed, 9 at the cut kept
    assert set(table) == {0, 9}
    check_td(h, table, [0, U64, 9])
    h.reset()
    b = mk(T0 + 10, T0 + 100)
    h.observe(b)
    table = expire_td(h, tdref.table_of(b), T0 + 51)  # 0 removed, 2^64 - 1 kept
    assert set(table) == {U64}
    check_td(h, table, [0, U64, 9])
    h.observe(b)  # traceId 0 enters its slot again
    check_td(h, tdref.table_of(b), [0, U64, 9])


def test_a_reserve_hint_does_not_survive_an_expiry(h):
    n = 500
    ids = some_ids(41, n)
    b = tdref.fill(ids, np.full(n, T0), T0 + np.arange(n), np.ones(n, bool))
    h.reserve(10_000)
    h.observe(DeviceColumns.from_host(b))
    assert h.info()["slots"] == 32768
    table = expire_td(h, tdref.table_of(b), T0)        # nothing expires: slots unchanged
    assert h.info()["slots"] == 32768
    table = expire_td(h, table, T0 + 250)              # the one operation that shrinks the table
    assert h.info()["slots"] == 1024 and h.info()["bytes"] == 1025 * 24
    check_td(h, table, ids)


def test_td_expire_timing(gpu):
    b = tdref.fill(some_ids(42, 3000), np.full(3000, T0), T0 + np.arange(3000), np.ones(3000, bool))
    with TraceDurationIndex(device=gpu, timing=True) as t:
        with pytest.raises(ZkError):
            t.expire_ms()
        t.observe(DeviceColumns.from_host(b))
        assert t.expire(T0 + 1500) == 1500
        ms = t.expire_ms()
        assert set(ms) == {"count", "size", "rebuild"} and all(v >= 0 for v in ms.values())
    with TraceDurationIndex(device=gpu) as plain:
        plain.observe(DeviceColumns.from_host(b))
        plain.expire(T0 + 1)
        with pytest.raises(ZkError):
            plain.expire_ms()


# ---- 6. the invariant: one cutoff over the three indices -----------------------------------------------------------
def test_every_id_the_trace_id_queries_return_is_in_the_duration_index(gpu):
    web, db = Endpoint(1, 80, "web"), Endpoint(2, 5432, "db")
    SEC = 1_000_000
    spans = []
    for t in range(1, 121):
        start = T0 + (t * 7919 % 100) * SEC
        anns = [Annotation(start, "sr", web), Annotation(start + 900, "ss", web), Annotation(start + 10, "retry", web)]
        bas = (BinaryAnnotation("http.uri", b"/a", "String", web),)
        spans.append(Span(t, "get" if t % 2 else "put", 100 + t, None, tuple(anns), bas))
        if t % 3 == 0:  # a second, later fragment: the trace outlives its first span's entries
            later = start + 40 * SEC
            spans.append(Span(t, "query", 500 + t, 100 + t, (Annotation(later, "sr", db), Annotation(later + 50, "ss", db),
                                                               Annotation(later + 5, "retry", db))))
    dec = SpanDecoder()
    cols, rejected, items = dec.decode_indexed([thriftenc.snappy(thriftenc.span(s)) for s in spans], span_names=True)
    assert rejected == 0
    services, span_names = dec.service_names(), dec.span_names()
    S = len(services)
    with TraceNameIndex(S, device=gpu, services=services, span_names=span_names) as names, \
            TraceAnnotationIndex(S, device=gpu, services=services) as anns_idx, TraceDurationIndex(device=gpu) as durations:
        names.observe(DeviceColumns.from_host(cols))
        anns_idx.observe(items)
        durations.observe(cols)
        ne, ae, table = ixref.entries_of(cols, S), items.rows(), tdref.table_of(cols)
        policy = IndexRetention(30, names=names, annotations=[anns_idx], durations=durations)
        assert policy.getDataTimeToLive() == 30
        now = T0 + 90 * SEC
        cut = now - 30 * SEC
        got = policy.expire(now)
        ne, ae = [x for x in ne if x[2] >= cut], [x for x in ae if x[3] >= cut]
        left = {t: v for t, v in table.items() if v[1] >= cut}
        assert got == {"cutoff": cut, "names": names_removed(cols, S, cut), "annotations": len(items) - len(ae),
                       "durations": len(table) - len(left)}
        assert 0 < len(left) < len(table) and 0 < len(ne) and 0 < len(ae)
        returned = set()
        for svc in ("web", "db"):
            s = services.index(svc)
            rows = names.getTraceIdsByName(svc, None, INT64_MAX, 4096)
            assert [tuple(t) for t in rows] == ixref.trace_ids(ne, s, ixref.ANY, INT64_MAX, 4096)[0]
            by_ann = anns_idx.getTraceIdsByAnnotation(svc, "retry", None, INT64_MAX, 4096)
            assert [tuple(t) for t in by_ann] == axref.by_annotation(ae, s, "retry", None, INT64_MAX, 4096)
            by_bin = anns_idx.getTraceIdsByAnnotation(svc, "http.uri", b"/a", INT64_MAX, 4096)
            for answer in (rows, by_ann, by_bin):
                ids = [t.trace_id for t in answer]
                assert all(t.timestamp >= cut for t in answer)
                if ids:
                    assert durations.lookup(ids)[2].all()  # every id the index returns is in the duration index
                    for order in tdref.ORDERS:
                        assert sorted(durations.sortTraceIds(ids, len(ids), order)) == sorted(ids)  # none is lost
                returned |= set(ids)
        assert returned and returned <= set(left)
        # (the case the invariant is about: a trace that stays although older entries of it went)
        assert any(x[3] in left for x in ixref.entries_of(cols, S) if x[2] < cut)


def names_removed(cols, S, cut):
    return sum(1 for x in ixref.entries_of(cols, S) if x[2] < cut)
