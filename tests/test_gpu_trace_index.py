"""The trace-id index by service and span name on the device (include/zkindex.h,
zipkin_amd/nameindex.py) against tests/ixref.py and the validator's vectors
(tests/golden/trace_ids_by_name.json). Every comparison is exact equality; nothing depends on the order
inside a service's slice."""
import ctypes as C

import numpy as np
import pytest

from tests import ixref, tdref
from tests.ixref import ANY, INT64_MAX, INT64_MIN, SVC_CLIENT, SVC_SERVER
from zipkin_amd import DeviceColumns, IndexedTraceId, TraceDurationIndex, TraceNameIndex, ZkError, _abi

pytestmark = pytest.mark.gpu

T0 = 1_400_000_000_000_000
U64 = 2 ** 64 - 1


@pytest.fixture()
def make(gpu):
    made = []

    def factory(S, **kw):
        made.append(TraceNameIndex(S, device=gpu, **kw))
        return made[-1]

    yield factory
    for idx in made:
        idx.close()


def observe_all(idx, batches, device=True):
    for b in batches:
        idx.observe(DeviceColumns.from_host(b) if device else b)


def ask(idx, entries, service, name, end_ts, limit):
    got = idx.getTraceIdsByName(service, name, end_ts, limit)
    rows, matched = ixref.trace_ids(entries, service, name, end_ts, limit)
    assert all(isinstance(t, IndexedTraceId) for t in got)
    assert [tuple(t) for t in got] == rows, (service, name, end_ts, limit)
    assert idx.matched == matched, (service, name, end_ts, limit)
    return rows


def some_ids(seed, n):
    """n distinct traceIds spread over 64 bits, 0 and 2^64 - 1 among them."""
    ids = np.unique(np.random.default_rng(seed).integers(1, 2 ** 64 - 1, 2 * n, dtype=np.uint64))[:n]
    np.random.default_rng(seed + 1).shuffle(ids)
    ids[0], ids[1] = 0, U64
    return ids


# ---- 1. the validator's vectors ------------------------------------------------------------------------
@pytest.mark.parametrize("device", (True, False), ids=("device_batches", "host_batches"))
def test_golden_vectors(make, device):
    g = ixref.golden()
    b, services, names = ixref.golden_batch(g)
    idx = make(len(services), services=services, span_names=names)
    observe_all(idx, [b], device=device)
    for q in g["trace_ids_by_name"]:
        got = idx.getTraceIdsByName(q["service"], q["span_name"], q["end_ts"], q["limit"])
        if q["head_trace_id"] is None:
            assert got == []
        else:
            assert got[0].trace_id == q["head_trace_id"] and got[0].timestamp == max(g["spans"]["span1"]["timestamps"])
    for svc, want in g["span_names"].items():
        assert idx.getSpanNames(svc) == set(want)
    assert idx.getSpanNames("SERVICE") == set(g["span_names"]["service"])
    assert idx.getAllServiceNames() == set(g["service_names"])
    assert [tuple(t) for t in idx.getTraceIdsByName("Service", "MethodCall", 100, 3)] == [(123, 20)]


# ---- 2. empty index, empty service, one record ----------------------------------------------------------
def test_empty_index_and_one_record(make):
    idx = make(5)
    assert idx.info() == {"entries": 0, "segments": 0, "bytes": 0}
    assert idx.getTraceIdsByName(3, None, INT64_MAX, 10) == [] and idx.matched == 0
    assert idx.getSpanNames(3) == set() and idx.getAllServiceNames() == set()
    assert idx.service_counts().tolist() == [0] * 5
    b = ixref.batch([3], [9], [T0], [77])
    observe_all(idx, [b])
    info = idx.info()
    assert (info["entries"], info["segments"]) == (1, 1) and info["bytes"] >= 18
    e = ixref.entries_of(b, 5)
    assert ask(idx, e, 3, ANY, INT64_MAX, 10) == [(77, T0)]
    assert ask(idx, e, 3, 9, T0, 1) == [(77, T0)]
    assert ask(idx, e, 2, ANY, INT64_MAX, 10) == []  # an empty service beside a full one
    assert idx.getSpanNames(3) == {9} and idx.getSpanNames(2) == set() and idx.getAllServiceNames() == {3}
    # a batch none of whose records is indexed adds nothing
    observe_all(idx, [ixref.batch([3, 3], [1, 1], [T0, T0], [5, 6], timed=False)])
    assert idx.info() == info


# ---- 3. the predicate ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", (True, False), ids=("device_batches", "host_batches"))
def test_predicate(make, device):
    CL = 2  # the service called "client"
    #                 not indexed: untimed, no SVC bit, client cs, client cr | indexed: client sr/ss only, other svc cs, both sides
    b = ixref.batch([1, 1, CL, CL, CL, 1, 1], [4] * 7, T0 + np.arange(7), [10, 11, 12, 13, 14, 15, 16],
                    timed=[False, True, True, True, True, True, True],
                    svc=[SVC_SERVER, 0, SVC_CLIENT, SVC_CLIENT, SVC_SERVER, SVC_CLIENT, SVC_CLIENT | SVC_SERVER],
                    cs=[0, 0, 1, 0, 0, 2, 1], cr=[0, 0, 0, 3, 0, 0, 1], sr=[0, 0, 0, 0, 1, 0, 0], ss=[0, 0, 0, 0, 2, 0, 0])
    idx = make(4, client_service=CL)
    observe_all(idx, [b], device=device)
    e = ixref.entries_of(b, 4, client_service=CL)
    assert sorted(x[3] for x in e) == [14, 15, 16]
    assert idx.info()["entries"] == 3
    for s in range(4):
        ask(idx, e, s, ANY, INT64_MAX, 10)
    assert idx.service_counts().tolist() == [0, 2, 1, 0]
    off = make(4, client_service=None)  # the rule switched off: the client's cs and cr spans are indexed too
    observe_all(off, [b], device=device)
    e_off = ixref.entries_of(b, 4)
    assert sorted(x[3] for x in e_off) == [12, 13, 14, 15, 16]
    for s in range(4):
        ask(off, e_off, s, ANY, INT64_MAX, 10)


# ---- 4. extremes ----------------------------------------------------------------------------------------------
def test_extremes(make):
    S = 4096
    svc = [0, 0, 0, 0, 4095, 4095, 4095, 4095, 0, 4095]
    name = [1, 65535, 1, 65535, 1, 65535, 65535, 1, 1, 65535]
    ts = [INT64_MIN, INT64_MAX, -1, 0, INT64_MIN, INT64_MAX, 7, 7, INT64_MAX, INT64_MIN]
    tid = [0, U64, U64, 0, U64, 0, 0, U64, 0, 0]
    b = ixref.batch(svc, name, ts, tid)
    idx = make(S)
    observe_all(idx, [b])
    e = ixref.entries_of(b, S)
    assert len(e) == 10
    for s in (0, 4095, 1, 4094):
        for nm in (ANY, 1, 65535, 2):
            for end in (INT64_MIN, INT64_MIN + 1, -2, -1, 0, 6, 7, 8, INT64_MAX - 1, INT64_MAX):
                for limit in (1, 4096):
                    ask(idx, e, s, nm, end, limit)
    # end_ts equal to an entry's ts takes it, one below does not
    assert (U64, 7) in ask(idx, e, 4095, ANY, 7, 10) and (U64, 7) not in ask(idx, e, 4095, ANY, 6, 10)
    assert ask(idx, e, 0, ANY, INT64_MIN, 10) == [(0, INT64_MIN)]
    assert ask(idx, e, 0, ANY, INT64_MAX, 2) == [(0, INT64_MAX), (U64, INT64_MAX)]
    assert idx.getSpanNames(0) == {1, 65535} and idx.getAllServiceNames() == {0, 4095}


# ---- 5. service range -------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", (True, False), ids=("device_batches", "host_batches"))
def test_service_range(make, device):
    S = 6
    good = ixref.batch(np.arange(300) % S, np.arange(300) % 3, T0 + np.arange(300), some_ids(50, 300))
    idx = make(S, client_service=1)
    observe_all(idx, [good], device=device)
    e = ixref.entries_of(good, S, client_service=1)
    info, counts = idx.info(), idx.service_counts().tolist()
    svc = (np.arange(200) % S).astype(np.uint32)
    svc[137] = S  # one bad indexed record among good ones
    bad = ixref.batch(svc, 1, T0, some_ids(51, 200))
    for worst in (S, 4096, 0xFFFFFFFF):
        bad.service_id[137] = worst
        with pytest.raises(ZkError) as err:
            observe_all(idx, [bad], device=device)
        assert err.value.status == _abi.ZK_ERR_SERVICE_RANGE
        assert idx.info() == info and idx.service_counts().tolist() == counts
        for s in range(S):
            ask(idx, e, s, ANY, INT64_MAX, 4096)
    # a bad service id on records that are not indexed is accepted
    ok = ixref.batch([S, 0xFFFFFFFF, 1, 0, 77], 1, T0 + 5, [1, 2, 3, 4, 5], timed=[False, True, True, True, True],
                     svc=[SVC_SERVER, 0, SVC_CLIENT, SVC_SERVER, 0], cs=[0, 0, 1, 0, 1])
    observe_all(idx, [ok], device=device)
    e2 = e + ixref.entries_of(ok, S, client_service=1)
    assert len(e2) == len(e) + 1 and idx.info()["entries"] == len(e2)
    for s in range(S):
        ask(idx, e2, s, ANY, INT64_MAX, 4096)


# ---- 6. argument refusals ------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_as_they_were(make):
    S = 3
    b = ixref.batch(np.arange(60) % S, 1 + np.arange(60) % 2, T0 + np.arange(60), some_ids(52, 60))
    idx = make(S)
    observe_all(idx, [b])
    e = ixref.entries_of(b, S)
    L = _abi.lib()
    ids = (C.c_uint64 * 8)(*[0x5A5A5A5A5A5A5A5A] * 8)
    ts = (C.c_int64 * 8)(*[0x5A5A5A5A] * 8)
    nm = (C.c_uint16 * 8)(*[0x5A5A] * 8)
    n, m = C.c_uint32(99), C.c_uint64(99)
    #      service, name, limit
    bad = [(0, 0, 8), (S, 1, 8), (0xFFFFFFFF, _abi.ZK_IX_ANY_NAME, 8), (0, 1, 0), (0, 1, _abi.ZK_IX_MAX_LIMIT + 1),
           (0, 65536, 8), (0, 0xFFFFFFFE, 8)]
    for service, name, limit in bad:
        assert L.zk_ix_trace_ids(idx._h, service, name, INT64_MAX, limit, ids, ts, C.byref(n), C.byref(m)) == _abi.ZK_ERR_INVALID_ARG
        assert L.zk_ix_last_error(idx._h)
    assert L.zk_ix_trace_ids(idx._h, 0, 1, 0, 8, None, ts, C.byref(n), None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_trace_ids(idx._h, 0, 1, 0, 8, ids, None, C.byref(n), None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_trace_ids(idx._h, 0, 1, 0, 8, ids, ts, None, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_span_names(idx._h, S, nm, 8, C.byref(n)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_span_names(idx._h, 0, None, 8, C.byref(n)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_span_names(idx._h, 0, nm, 8, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_observe(idx._h, None, 0) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_service_counts(idx._h, None) == _abi.ZK_ERR_INVALID_ARG
    assert list(ids) == [0x5A5A5A5A5A5A5A5A] * 8 and list(ts) == [0x5A5A5A5A] * 8 and list(nm) == [0x5A5A] * 8
    assert (n.value, m.value) == (99, 99)
    for service, name, limit in ((0, 0, 5), (S, None, 5), (0, None, 0), (0, None, 4097)):
        with pytest.raises(ZkError) as err:
            idx.getTraceIdsByName(service, name, INT64_MAX, limit)
        assert err.value.status == _abi.ZK_ERR_INVALID_ARG
    # matched may be NULL, and the handle still answers
    assert L.zk_ix_trace_ids(idx._h, 1, _abi.ZK_IX_ANY_NAME, INT64_MAX, 8, ids, ts, C.byref(n), None) == _abi.ZK_OK
    assert [(ids[i], ts[i]) for i in range(n.value)] == ixref.trace_ids(e, 1, ANY, INT64_MAX, 8)[0]


def test_observe_flags_and_empty_batches(make):
    b = ixref.batch(np.arange(100) % 4, 1, T0 + np.arange(100), some_ids(53, 100))
    d = DeviceColumns.from_host(b)
    idx = make(4)
    ab, empty = d.abi(), d.abi(0)
    L = _abi.lib()
    assert L.zk_ix_observe(idx._h, C.byref(ab), 1 << 20) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_observe(idx._h, C.byref(empty), _abi.ZK_BATCH_DEVICE_PTRS) == _abi.ZK_OK
    assert idx.info() == {"entries": 0, "segments": 0, "bytes": 0}
    big = d.abi(2 ** 32)
    assert L.zk_ix_observe(idx._h, C.byref(big), _abi.ZK_BATCH_DEVICE_PTRS) == _abi.ZK_ERR_UNSUPPORTED
    assert L.zk_ix_observe(idx._h, C.byref(ab), _abi.ZK_BATCH_DEVICE_PTRS | _abi.ZK_BATCH_TRACE_CLUSTERED) == _abi.ZK_OK
    e = ixref.entries_of(b, 4)
    for s in range(4):
        ask(idx, e, s, ANY, INT64_MAX, 100)


# ---- 7. slice and tile edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("device", (True, False), ids=("device_batches", "host_batches"))
def test_slice_and_tile_edges(make, device):
    sizes = [0, 1, 63, 64, 65, 1023, 1024, 1025]
    S = len(sizes) + 2  # (an empty service on either side)
    rng = np.random.default_rng(54)
    svc = np.repeat(np.arange(1, 1 + len(sizes)), sizes)
    n = len(svc)
    perm = rng.permutation(n)
    b = ixref.batch(svc[perm], rng.integers(0, 4, n), T0 + rng.integers(0, 50, n), some_ids(54, n))
    idx = make(S)
    observe_all(idx, [b], device=device)
    e = ixref.entries_of(b, S)
    assert idx.service_counts().tolist() == [0] + sizes + [0] == ixref.service_counts(e, S).tolist()
    assert idx.info()["entries"] == n
    for s in range(S):
        ask(idx, e, s, ANY, INT64_MAX, 4096)
        ask(idx, e, s, ANY, T0 + 25, 5)
        ask(idx, e, s, 2, INT64_MAX, 70)
        assert idx.getSpanNames(s) == set(ixref.span_names(e, s))


# ---- 8. histogram skew ----------------------------------------------------------------------------------------
def test_one_hot_service(make):
    n, S = 50_000, 4
    rng = np.random.default_rng(55)
    b = ixref.batch(2, rng.integers(0, 3, n), T0 + rng.integers(0, 10 ** 9, n), some_ids(55, n))
    idx = make(S)
    observe_all(idx, [b])
    e = ixref.entries_of(b, S)
    assert idx.service_counts().tolist() == [0, 0, n, 0]
    for limit in (1, 100, 4096):
        ask(idx, e, 2, ANY, INT64_MAX, limit)
    ask(idx, e, 2, 1, T0 + 5 * 10 ** 8, 100)
    assert idx.getTraceIdsByName(1, None, INT64_MAX, 5) == [] and idx.getTraceIdsByName(3, None, INT64_MAX, 5) == []


def test_one_record_in_each_of_4096_services(make):
    S = 4096
    rng = np.random.default_rng(56)
    b = ixref.batch(rng.permutation(S), 1 + np.arange(S) % 9, T0 + rng.integers(0, 99, S), some_ids(56, S))
    idx = make(S)
    observe_all(idx, [b])
    assert idx.service_counts().tolist() == [1] * S
    by_service = {x[0]: x for x in ixref.entries_of(b, S)}
    for s in list(range(0, S, 37)) + [1, 4094, 4095]:
        ask(idx, [by_service[s]], s, ANY, INT64_MAX, 4096)
        assert idx.getSpanNames(s) == {by_service[s][1]}
    assert idx.getAllServiceNames() == set(range(S))


# ---- 9. segments ------------------------------------------------------------------------------------------------
def random_batch(seed, n, S, ids=None, names=4, span=10 ** 6):
    rng = np.random.default_rng(seed)
    ids = some_ids(seed, n) if ids is None else ids
    return ixref.batch(rng.integers(0, S, n), rng.integers(0, names, n), T0 + rng.integers(0, span, n), ids,
                       timed=rng.integers(0, 8, n) != 0, seed=seed)


def ask_all(idx, e, S, limits=(7, 4096)):
    for s in range(S):
        for limit in limits:
            ask(idx, e, s, ANY, INT64_MAX, limit)
        ask(idx, e, s, 1, T0 + 500_000, 50)
        assert idx.getSpanNames(s) == set(ixref.span_names(e, s))
    assert idx.service_counts().tolist() == ixref.service_counts(e, S).tolist()


def test_three_batches_then_compact_and_reset(make):
    S = 5
    batches = [random_batch(60 + k, n, S) for k, n in enumerate((3000, 10, 7000))]
    idx = make(S)
    observe_all(idx, batches[:2])
    observe_all(idx, batches[2:], device=False)
    e = ixref.entries_of(batches, S)
    assert idx.info()["segments"] == 3 and idx.info()["entries"] == len(e)
    ask_all(idx, e, S)
    before = [idx.getTraceIdsByName(s, None, INT64_MAX, 4096) for s in range(S)]
    idx.compact()
    assert idx.info()["segments"] == 1 and idx.info()["entries"] == len(e)
    assert [idx.getTraceIdsByName(s, None, INT64_MAX, 4096) for s in range(S)] == before
    ask_all(idx, e, S)
    idx.compact()  # one segment: nothing to do
    assert idx.info()["segments"] == 1
    idx.reset()
    assert idx.info() == {"entries": 0, "segments": 0, "bytes": 0} and idx.service_counts().tolist() == [0] * S
    assert idx.getTraceIdsByName(0, None, INT64_MAX, 5) == [] and idx.getSpanNames(0) == set()
    observe_all(idx, batches[1:2])
    ask_all(idx, ixref.entries_of(batches[1], S), S)


def test_the_same_batch_twice(make):
    S = 3
    b = random_batch(63, 2000, S)
    d = DeviceColumns.from_host(b)
    idx = make(S)
    idx.observe(d)
    idx.observe(d)
    e = ixref.entries_of([b, b], S)
    assert idx.info()["entries"] == len(e) and idx.info()["segments"] == 2
    for s in range(S):
        rows = ask(idx, e, s, ANY, INT64_MAX, 4096)
        assert rows[0::2] == rows[1::2]  # every pair appears twice
    idx.compact()
    ask_all(idx, e, S)


def test_seventy_small_observes_stay_within_the_segment_bound(make):
    S = 4
    idx = make(S)
    batches = []
    for k in range(70):
        batches.append(random_batch(100 + k, 30 + k, S))
        observe_all(idx, batches[-1:], device=k % 2 == 0)
        info = idx.info()
        assert 1 <= info["segments"] <= _abi.ZK_IX_MAX_SEGMENTS
        if k == 63:
            assert info["segments"] == 64
        if k == 64:
            assert info["segments"] == 2  # the 65th observe merged the 64 first
        if k >= 60:
            e = ixref.entries_of(batches, S)
            assert info["entries"] == len(e)
            ask_all(idx, e, S, limits=(4096,))


# ---- 10. the select beyond 4096 matches ---------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ("eight_timestamps", "low_ten_bits"))
def test_select_beyond_the_cap(make, pattern):
    n, S = 20_000, 2
    rng = np.random.default_rng(70)
    if pattern == "eight_timestamps":  # the rounds must go on into the traceId bits
        values = T0 + np.array([0, 1, 2, 3, 1 << 20, 1 << 30, 1 << 40, -T0 - 5])
        ts = values[rng.integers(0, 8, n)]
        few_end = int(values.min())      # matches one value's 2500 or so: fewer than the limit
    else:                                # ts share all but their low 10 bits
        ts = (T0 & ~1023) + rng.integers(0, 1024, n)
        few_end = int(T0 & ~1023) + 100
    b = ixref.batch(1, rng.integers(1, 3, n), ts, some_ids(71, n))
    idx = make(S)
    observe_all(idx, [b])
    e = ixref.entries_of(b, S)
    for limit in (1, 100, 4096):
        ask(idx, e, 1, ANY, INT64_MAX, limit)
    rows = ask(idx, e, 1, ANY, few_end, 4096)
    assert 0 < len(rows) == idx.matched < 4096  # limit > matched
    ask(idx, e, 1, 2, INT64_MAX, 4096)


# ---- 11. equal keys ---------------------------------------------------------------------------------------------
def test_nine_thousand_equal_keys(make):
    b = ixref.batch(0, 3, T0, np.full(3000, 0xABCDEF, np.uint64))
    idx = make(2)
    d = DeviceColumns.from_host(b)
    for _ in range(3):
        idx.observe(d)
    got = idx.getTraceIdsByName(0, None, INT64_MAX, 4096)
    assert got == [IndexedTraceId(0xABCDEF, T0)] * 4096 and idx.matched == 9000
    assert idx.getTraceIdsByName(0, 3, T0, 1) == [IndexedTraceId(0xABCDEF, T0)] and idx.matched == 9000
    assert idx.getTraceIdsByName(0, 3, T0 - 1, 1) == [] and idx.matched == 0


def test_a_block_of_equal_keys_straddles_the_limit(make):
    """3000 distinct newer entries, 5000 equal ones, 3000 distinct older ones: limit 4096 ends inside the
    equal block, whose candidates differ in no bit -- the termination case."""
    rng = np.random.default_rng(72)
    ids = some_ids(72, 6000)
    ts = np.concatenate([T0 + 1 + rng.integers(0, 1000, 3000), np.full(5000, T0), T0 - 1 - rng.integers(0, 1000, 3000)])
    tid = np.concatenate([ids[:3000], np.full(5000, 1 << 63, np.uint64), ids[3000:]])
    perm = rng.permutation(len(ts))
    b = ixref.batch(1, 1, ts[perm], tid[perm])
    idx = make(2)
    observe_all(idx, [b])
    e = ixref.entries_of(b, 2)
    rows = ask(idx, e, 1, ANY, INT64_MAX, 4096)
    assert rows[2999] != (1 << 63, T0) and rows[3000:] == [(1 << 63, T0)] * 1096
    for limit in (1, 3000, 3001, 4095):
        ask(idx, e, 1, ANY, INT64_MAX, limit)
    rows = ask(idx, e, 1, ANY, T0, 4096)  # the equal block first, 5000 of it
    assert rows == [(1 << 63, T0)] * 4096 and idx.matched == 8000
    # the equal block wholly inside the answer is not enough entries to reach the cap's rounds
    ask(idx, e, 1, ANY, T0 - 1, 4096)


# ---- 12. the name filter ------------------------------------------------------------------------------------------
def test_name_filter(make):
    n, S = 20_000, 3
    rng = np.random.default_rng(73)
    names = np.array([0, 5, 6, 65535])[rng.integers(0, 4, n)]
    b = ixref.batch(rng.integers(1, 3, n), names, T0 + rng.integers(0, 3000, n), some_ids(73, n))
    other = ixref.batch(0, 9, T0, [4, 5, 6])  # another service's name must not show
    idx = make(S)
    observe_all(idx, [b, other])
    e = ixref.entries_of([b, other], S)
    for nm in (ANY, 5, 6, 65535):
        for limit in (1, 4096):
            ask(idx, e, 1, nm, INT64_MAX, limit)
        ask(idx, e, 2, nm, T0 + 1500, 300)
    assert ixref.trace_ids(e, 1, ANY, INT64_MAX, 1)[1] > 2 * 4096  # (more than the cap under ANY ...)
    assert ask(idx, e, 1, 7, INT64_MAX, 10) == [] and idx.matched == 0  # an absent name
    assert ask(idx, e, 1, 9, INT64_MAX, 10) == []
    assert idx.getSpanNames(1) == {5, 6, 65535} == set(ixref.span_names(e, 1))  # id 0 is not a name
    assert idx.getSpanNames(0) == {9}
    assert idx.span_name_ids(1) == [5, 6, 65535]
    L = _abi.lib()
    out = (C.c_uint16 * 4)(*[0x5A5A] * 4)
    k = C.c_uint32(99)
    assert L.zk_ix_span_names(idx._h, 1, out, 2, C.byref(k)) == _abi.ZK_ERR_CAPACITY
    assert k.value == 3 and list(out) == [0x5A5A] * 4
    assert L.zk_ix_span_names(idx._h, 1, None, 0, C.byref(k)) == _abi.ZK_ERR_CAPACITY and k.value == 3
    assert L.zk_ix_span_names(idx._h, 1, out, 3, C.byref(k)) == _abi.ZK_OK
    assert k.value == 3 and list(out) == [5, 6, 65535, 0x5A5A]


def test_more_than_the_cap_under_a_name_filter(make):
    n = 12_000
    rng = np.random.default_rng(74)
    b = ixref.batch(0, np.where(np.arange(n) % 4 == 0, 2, 1), T0 + rng.integers(0, 500, n), some_ids(74, n))
    idx = make(1)
    observe_all(idx, [b])
    e = ixref.entries_of(b, 1)
    for limit in (1, 4096):
        ask(idx, e, 0, 1, INT64_MAX, limit)
    assert idx.matched == 9000
    ask(idx, e, 0, 1, T0 + 250, 4096)
    ask(idx, e, 0, 2, INT64_MAX, 4096)


def test_names_as_strings_fold_over_several_ids(make):
    services = ["Web", "db", "WEB"]
    span_names = ["GET", "get", "put"]
    rng = np.random.default_rng(75)
    n = 600
    b = ixref.batch(rng.integers(0, 3, n), rng.integers(0, 4, n), T0 + rng.integers(0, 40, n), some_ids(75, n))
    idx = make(3, services=services, span_names=span_names)
    observe_all(idx, [b])
    e = ixref.entries_of(b, 3)
    fold = lambda svcs, nms, end, limit: sorted(
        [r for s in svcs for nm in nms for r in ixref.trace_ids(e, s, nm, end, 10 ** 9)[0]], key=lambda r: (-r[1], r[0]))[:limit]
    assert [tuple(t) for t in idx.getTraceIdsByName("web", None, INT64_MAX, 50)] == fold((0, 2), (ANY,), INT64_MAX, 50)
    assert [tuple(t) for t in idx.getTraceIdsByName("WEB", "Get", T0 + 20, 4096)] == fold((0, 2), (1, 2), T0 + 20, 4096)
    assert idx.matched == len(fold((0, 2), (1, 2), T0 + 20, 10 ** 9))
    assert [tuple(t) for t in idx.getTraceIdsByName("db", "PUT", INT64_MAX, 5)] == fold((1,), (3,), INT64_MAX, 5)
    assert idx.getTraceIdsByName("cache", None, INT64_MAX, 5) == [] and idx.getTraceIdsByName("db", "post", INT64_MAX, 5) == []
    assert idx.getSpanNames("web") == {"get", "put"} and idx.getSpanNames("cache") == set()
    assert idx.getAllServiceNames() == {"web", "db"}


# ---- 13. the query service -----------------------------------------------------------------------------------------
def test_query_service(make, gpu):
    S = 3
    rng = np.random.default_rng(76)
    n = 4000
    tids = some_ids(76, 700)
    batches = []
    for k in range(2):
        b = ixref.batch(rng.integers(0, S, n), rng.integers(0, 3, n), 0, tids[rng.integers(0, 700, n)], seed=k)
        b.first_ts[:] = T0 + rng.integers(0, 1000, n)
        b.last_ts[:] = b.first_ts + rng.integers(0, 300, n)
        batches.append(b)
    idx = make(S)
    observe_all(idx, batches)
    e = ixref.entries_of(batches, S)
    with TraceDurationIndex(device=gpu) as dur:
        for b in batches:
            dur.observe(DeviceColumns.from_host(b))
        table = tdref.table_of(batches)

        def by_hand(service, name, end, limit, order):
            ids = [r[0] for r in ixref.trace_ids(e, service, name, end, limit)[0]]
            if order is None:
                return ids
            found = tdref.entries(table, ids)  # (traceId, duration, start) in asked order
            col = 1 if order.startswith("duration") else 2
            found.sort(key=lambda r: r[col], reverse=order.endswith("desc"))  # stable, like the query service
            return [r[0] for r in found[:limit]]

        for order in tdref.ORDERS + (None,):
            for limit in (1, 10, 500):
                assert idx.getTraceIdsByServiceName(1, T0 + 800, limit, order, dur) == by_hand(1, ANY, T0 + 800, limit, order)
                assert idx.getTraceIdsBySpanName(2, 1, T0 + 1200, limit, order, dur) == by_hand(2, 1, T0 + 1200, limit, order)
        assert idx.getTraceIdsBySpanName(2, "", T0 + 1200, 10, None, dur) == by_hand(2, ANY, T0 + 1200, 10, None)
        with pytest.raises(ValueError):
            idx.getTraceIdsByServiceName(None, T0, 10, None, dur)


# ---- timing ---------------------------------------------------------------------------------------------------
def test_timing(make):
    b = random_batch(77, 6000, 4)
    t = make(4, timing=True)
    with pytest.raises(ZkError):
        t.query_ms()
    with pytest.raises(ZkError):
        t.observe_ms()
    t.observe(DeviceColumns.from_host(b))
    ms = t.observe_ms()
    assert set(ms) == {"count", "size", "scatter"} and all(v >= 0 for v in ms.values())
    t.getTraceIdsByName(1, None, INT64_MAX, 10)
    assert t.query_ms() > 0
    plain = make(4)
    plain.observe(DeviceColumns.from_host(b))
    with pytest.raises(ZkError):
        plain.observe_ms()


# ---- 14. the job ------------------------------------------------------------------------------------------------
def test_job_observes_its_batches(make, gpu):
    from tests.bulkfrag import service_name
    from zipkin_amd import tracegen_host
    from zipkin_amd.aggregates import Dictionary, ZipkinAggregateJob

    S = 23
    cols = tracegen_host(71, 600, max_depth=5, num_services=S)
    cols.set_name_ids(1 + (cols.span_id % np.uint64(5)).astype(np.int64))
    part = (cols.trace_id % np.uint64(3)).astype(np.int64)
    rng = np.random.default_rng(71)
    parts = [cols.take(rng.permutation(np.flatnonzero(part == k))) for k in range(3)]
    names = Dictionary([service_name(i) for i in range(S)])
    plain = ZipkinAggregateJob(names, device=gpu, clock=lambda: 10 ** 15)
    want = plain.run(parts, S)
    plain.close()
    idx, direct = make(S), make(S)
    job = ZipkinAggregateJob(names, device=gpu, clock=lambda: 10 ** 15, names=idx)
    got = job.run(parts, S)
    job.close()
    assert want is not None and got == want
    observe_all(direct, parts)
    e = ixref.entries_of(parts, S)
    assert len(e) > 0 and idx.info() == direct.info() and idx.info()["entries"] == len(e)
    assert idx.service_counts().tolist() == direct.service_counts().tolist() == ixref.service_counts(e, S).tolist()
    end = int(np.median(cols.last_ts))
    for s in range(S):
        for nm, limit in ((ANY, 4096), (2, 20)):
            rows = ask(idx, e, s, nm, end, limit)
            assert [tuple(t) for t in direct.getTraceIdsByName(s, nm, end, limit)] == rows
        assert idx.getSpanNames(s) == direct.getSpanNames(s) == set(ixref.span_names(e, s))
