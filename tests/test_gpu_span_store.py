"""The span store by trace id on the device (include/zkspans.h, zipkin_amd/spanstore.py) against
tests/spref.py and the reference's vectors (tests/golden/trace_summaries.json). Every comparison is exact
equality; nothing depends on the order inside a bucket's slice."""
import ctypes as C

import numpy as np
import pytest

from tests import spref as R
from zipkin_amd import (DeviceColumns, SpanColumns, TraceDurationIndex, TraceNameIndex, TraceSpanStore, ZkError, _abi,
                        tracegen_host)
from zipkin_amd.columns import COLUMNS

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
COUNT_TILE = 1024      # k_sp_count's tile: 256 threads x 4 records
SCATTER_ROW = 256      # k_sp_scatter's row: one record per thread
SCATTER_CHUNK = 16384  # k_sp_scatter's stretch per workgroup: one more makes a second workgroup
FIND_PART = 4096       # the lookups split a slice longer than this over several workgroups
SENTINEL = 0xA5


@pytest.fixture()
def make(gpu):
    made = []

    def factory(**kw):
        made.append(TraceSpanStore(device=gpu, **kw))
        return made[-1]

    yield factory
    for s in made:
        s.close()


def observe_all(store, batches, device=True):
    for b in batches:
        store.observe(DeviceColumns.from_host(b) if device else b)


def batch(trace_id, seed=0) -> SpanColumns:
    """A batch with the given trace ids; every other column is noise over its whole range, a few span ids
    per trace so that fragments share spans."""
    trace_id = np.asarray(trace_id, np.uint64)
    n = len(trace_id)
    rng = np.random.default_rng(seed + 7 * n)
    c = SpanColumns.empty(n)
    c.trace_id[:] = trace_id
    c.span_id[:] = rng.integers(0, 4, n, dtype=np.uint64) * np.uint64(2 ** 62 + 1)
    c.parent_id[:] = rng.integers(0, 4, n, dtype=np.uint64) * np.uint64(2 ** 62 + 1)
    c.first_ts[:] = rng.integers(-2 ** 63, 2 ** 63, n, dtype=np.int64)
    c.last_ts[:] = rng.integers(-2 ** 63, 2 ** 63, n, dtype=np.int64)
    c.service_id[:] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    c.flags[:] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    return c


def check(store, model, extra_ids=()):
    """Everything the store answers about every trace of the model (and the extra ids) equals the model."""
    ids = sorted({r[0] for r in model}) + list(extra_ids)
    assert store.info()["entries"] == len(model)
    assert store.tracesExist(ids) == {i for i, f in zip(ids, R.exist(model, ids)) if f}
    assert store.getSpansByTraceIds(ids) == R.spans_by_trace_ids(model, ids)


def raw_gather(store, ids, cap, flags=0, ptr=None):
    """zk_sp_gather into sentinel-filled columns of `cap` entries: (status, n_out, counts, columns)."""
    ids = np.ascontiguousarray(np.asarray(ids, np.uint64))
    counts = np.full(len(ids), 0xDEADBEEF, np.uint32)
    cols = {k: np.frombuffer(bytes([SENTINEL]) * (max(cap, 1) * np.dtype(dt).itemsize), dt).copy() for k, dt in COLUMNS}
    rows = _abi.zk_sp_rows(*[cols[k].ctypes.data for k, _ in COLUMNS])
    total = C.c_uint64(12345)
    st = store._L.zk_sp_gather(store._h, ids.ctypes.data if ptr is None else ptr, len(ids), flags,
                               counts.ctypes.data_as(_abi._U32P), C.byref(rows), cap, C.byref(total))
    return st, int(total.value), counts.tolist(), cols


# ---- 1. the reference's vectors --------------------------------------------------------------------------
@pytest.mark.parametrize("device", (True, False), ids=("device_batches", "host_batches"))
def test_golden_vectors(make, device):
    g = R.golden()
    store = make(services=g["services"], span_names=g["span_names"])
    for case in g["cases"]:
        store.reset()
        rows = R.golden_rows(case, g["services"])
        observe_all(store, [R.cols_of(rows)], device=device)
        e, tid = case["expect"], case["trace_id"]
        assert store.tracesExist([tid]) == ({tid} if rows else set())
        assert store.getSpansByTraceId(tid) == sorted(rows, key=lambda r: r[1:])
        traces = store.getTracesByIds([tid])
        assert len(traces) == (1 if rows else 0)
        if rows:
            t = traces[0]
            assert [s.id for s in t.spans] == e["span_order"]
            se = t.getStartAndEndTimestamp()
            assert (None if se is None else list(se)) == e["start_end"]
            if "depths" in e:
                assert t.toSpanDepths() == {int(k): v for k, v in e["depths"].items()}
            if "services" in e:
                assert sorted(t.services) == e["services"]
        sm = store.getTraceSummariesByIds([tid])
        if e["start_end"] is None:
            assert sm == []
        else:
            assert (sm[0].trace_id, sm[0].start, sm[0].end, sm[0].duration_micro, sm[0].endpoints) == \
                (tid, e["start_end"][0], e["start_end"][1], e["duration_micro"], [])
            assert [tuple(x) for x in sm[0].span_timestamps] == R.span_timestamps(rows, g["services"])


# ---- 2. an empty store, one record -------------------------------------------------------------------------
def test_empty_store_and_one_record(make):
    store = make()
    assert store.info() == {"entries": 0, "segments": 0, "bytes": 0}
    assert store.exist([0, 5, U64]).tolist() == [False] * 3 and store.tracesExist([0, 5, U64]) == set()
    st, total, counts, cols = raw_gather(store, [0, 5, U64], 4)
    assert (st, total, counts) == (_abi.ZK_OK, 0, [0, 0, 0]) and all((c.view(np.uint8) == SENTINEL).all() for c in cols.values())
    assert store.getSpansByTraceIds([0, 5, U64]) == [] and store.getSpansByTraceId(5) == []
    counts, cols = store.gather([])
    assert len(counts) == 0 and len(cols["trace_id"]) == 0
    observe_all(store, [SpanColumns.empty(0)])
    assert store.info() == {"entries": 0, "segments": 0, "bytes": 0}
    for tid in (0, U64):
        store.reset()
        b = batch([tid], seed=tid & 3)
        b.first_ts[0], b.last_ts[0] = R.INT64_MIN, R.INT64_MAX
        observe_all(store, [b])
        info = store.info()
        assert (info["entries"], info["segments"]) == (1, 1) and info["bytes"] >= 48
        check(store, R.rows_of(b), extra_ids=[1, U64 - 1, U64 - tid])
        assert store.getSpansByTraceId(tid)[0][3:5] == (R.INT64_MIN, R.INT64_MAX)
    store.reset()
    assert store.info() == {"entries": 0, "segments": 0, "bytes": 0} and store.tracesExist([0, U64]) == set()


# ---- 3. batch sizes ----------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 255, 257, COUNT_TILE + 1, 4097, SCATTER_CHUNK + 1)


# (host batches differ from device batches only in the staging copy: three sizes of them)
@pytest.mark.parametrize("n,device", [(n, True) for n in SIZES] + [(n, False) for n in (1, 257, 4097)],
                         ids=lambda v: ("device" if v else "host") if isinstance(v, bool) else str(v))
def test_batch_sizes(make, n, device):
    assert SCATTER_ROW + 1 in SIZES
    rng = np.random.default_rng(n)
    pool = np.unique(rng.integers(0, 2 ** 64, max(1, n // 5), dtype=np.uint64))
    b = batch(pool[rng.integers(0, len(pool), n)], seed=n)
    store = make()
    observe_all(store, [b], device=device)
    assert store.info()["segments"] == 1
    check(store, R.rows_of(b), extra_ids=[int(pool[0]) ^ 1])


# ---- 4. buckets ----------------------------------------------------------------------------------------------------
def test_buckets(make):
    lo = [R.id_in_bucket(0, k) for k in range(5)]
    hi = [R.id_in_bucket(4095, k) for k in range(5)]
    assert {R.bucket(i) for i in lo} == {0} and {R.bucket(i) for i in hi} == {4095}
    store = make()
    b = batch(lo[:4] * 3 + hi[:4] * 2 + [R.id_in_bucket(2048, 0)], seed=4)
    observe_all(store, [b])
    check(store, R.rows_of(b), extra_ids=[lo[4], hi[4], R.id_in_bucket(2048, 1), R.id_in_bucket(1, 0)])
    counts, _ = store.gather([lo[4], hi[4], lo[0]])
    assert counts.tolist() == [0, 0, 3] and store.exist([lo[4], hi[4], lo[0]]).tolist() == [False, False, True]
    # every record in ONE bucket: the other 4095 are empty
    one = make()
    ids = [R.id_in_bucket(77, k) for k in range(40)]
    b1 = batch(np.repeat(np.array(ids[:39], np.uint64), 30), seed=5)
    observe_all(one, [b1])
    check(one, R.rows_of(b1), extra_ids=[ids[39], R.id_in_bucket(76, 0), R.id_in_bucket(78, 0)])


# ---- 5. a trace longer than a lookup's part ----------------------------------------------------------------
def test_long_trace(make):
    n = max(FIND_PART + 1, 5000)
    long_id, other, absent = (R.id_in_bucket(9, k) for k in range(3))
    tids = np.full(n + 700, long_id, np.uint64)
    tids[np.arange(700) * ((n + 700) // 700)] = other  # interleaved in the same bucket
    b = batch(tids, seed=6)
    b.span_id[:] = np.random.default_rng(6).integers(0, 50, len(b), dtype=np.uint64)  # many equal keys in the order
    store = make()
    observe_all(store, [b])
    model = R.rows_of(b)
    assert sum(r[0] == long_id for r in model) == n
    counts, cols = store.gather([long_id, absent, other])
    assert counts.tolist() == [n, 0, 700]
    assert list(zip(*[cols[k].tolist() for k, _ in COLUMNS])) == R.gather(model, [long_id, absent, other])[1]
    check(store, model, extra_ids=[absent])


# ---- 6. segments -------------------------------------------------------------------------------------------------
def test_segments_merge_and_compact(make):
    rng = np.random.default_rng(8)
    pool = np.unique(rng.integers(0, 2 ** 64, 40, dtype=np.uint64))
    spread = int(pool[0])
    store = make()
    batches = [batch([spread] * 3 + pool[rng.integers(0, len(pool), 20)].tolist(), seed=80 + k) for k in range(3)]
    observe_all(store, batches)
    model = R.rows_of(batches)
    assert store.info()["segments"] == 3 and len(store.getSpansByTraceId(spread)) >= 9
    check(store, model)
    for k in range(61):  # 64 segments: the bound
        batches.append(batch(pool[rng.integers(0, len(pool), 1 + k % 3)], seed=100 + k))
        observe_all(store, batches[-1:], device=k % 2 == 0)
    model = R.rows_of(batches)
    assert store.info()["segments"] == _abi.ZK_SP_MAX_SEGMENTS == 64
    check(store, model)
    batches.append(batch(pool[:2], seed=200))  # the 65th observe merges the 64 first
    observe_all(store, batches[-1:])
    model = R.rows_of(batches)
    info = store.info()
    assert (info["segments"], info["entries"]) == (2, len(model))
    before = store.getSpansByTraceIds(sorted(pool.tolist()))
    check(store, model)
    store.compact()
    after = store.info()
    assert (after["segments"], after["entries"]) == (1, info["entries"])
    assert store.getSpansByTraceIds(sorted(pool.tolist())) == before
    check(store, model)
    store.compact()  # one segment: nothing to do
    assert store.info() == after
    # the same batch again doubles every count
    c1, _ = store.gather(pool)
    observe_all(store, batches[:1])
    c2, _ = store.gather(pool)
    first = R.gather(R.rows_of(batches[0]), pool.tolist())[0]
    assert (c2 - c1).tolist() == first and sum(first) == len(batches[0])
    twice = make()
    observe_all(twice, [batches[0], batches[0]])
    assert twice.gather(pool)[0].tolist() == [2 * c for c in first]
    check(twice, R.rows_of([batches[0], batches[0]]))


# ---- 7. the ask --------------------------------------------------------------------------------------------------
def test_the_ask(make, gpu):
    import torch

    rng = np.random.default_rng(9)
    pool = np.unique(rng.integers(0, 2 ** 64, 3000, dtype=np.uint64))
    b = batch(pool[rng.integers(0, len(pool), 9000)], seed=9)
    model = R.rows_of(b)
    store = make()
    observe_all(store, [b])
    present = sorted({r[0] for r in model})
    absent = [int(x) for x in rng.integers(0, 2 ** 64, 50, dtype=np.uint64) if int(x) not in set(present)]
    ids = [present[0], absent[0], present[1], present[0], absent[1], present[0], U64, 0]
    counts, cols = store.gather(ids)
    want_counts, want_rows = R.gather(model, ids)
    assert counts.tolist() == want_counts and list(zip(*[cols[k].tolist() for k, _ in COLUMNS])) == want_rows
    assert store.exist(ids).tolist() == R.exist(model, ids)
    assert store.getSpansByTraceIds(ids) == R.spans_by_trace_ids(model, ids)
    # ZK_SP_MAX_IDS ids in one call, duplicates and absent ids among them; one more is refused
    big = (present + absent + present)[:_abi.ZK_SP_MAX_IDS]
    assert len(big) == _abi.ZK_SP_MAX_IDS == 4096
    counts, cols = store.gather(big)
    want_counts, want_rows = R.gather(model, big)
    assert counts.tolist() == want_counts and list(zip(*[cols[k].tolist() for k, _ in COLUMNS])) == want_rows
    assert store.exist(big).tolist() == R.exist(model, big)
    for call in (store.exist, store.gather):
        with pytest.raises(ZkError) as e:
            call(big + [1])
        assert e.value.status == _abi.ZK_ERR_INVALID_ARG and "ZK_SP_MAX_IDS" in e.value.message
    assert store.tracesExist(big + big) == {i for i in big if i in set(present)}  # (the Python call asks in parts)
    # device-pointer ids
    dev = torch.from_numpy(np.array(ids, np.uint64).view(np.int64)).to(f"cuda:{gpu}")
    assert store.exist(dev).tolist() == R.exist(model, ids)
    counts, cols = store.gather(dev)
    want_counts, want_rows = R.gather(model, ids)
    assert counts.tolist() == want_counts and list(zip(*[cols[k].tolist() for k, _ in COLUMNS])) == want_rows


# ---- 8. capacity -------------------------------------------------------------------------------------------------
def test_capacity(make):
    b = batch([5] * 7 + [6] * 3 + [9], seed=10)
    model = R.rows_of(b)
    store = make()
    observe_all(store, [b])
    ids = [6, 404, 5, 6]
    want_counts, want_rows = R.gather(model, ids)
    total = sum(want_counts)
    assert total == 13
    for cap in (total - 1, 0):
        st, n_out, counts, cols = raw_gather(store, ids, cap)
        assert (st, n_out, counts) == (_abi.ZK_ERR_CAPACITY, total, want_counts)
        assert all((c.view(np.uint8) == SENTINEL).all() for c in cols.values())
    st, n_out, counts, cols = raw_gather(store, ids, total)
    assert (st, n_out, counts) == (_abi.ZK_OK, total, want_counts)
    assert list(zip(*[cols[k].tolist() for k, _ in COLUMNS])) == want_rows
    st, n_out, counts, cols = raw_gather(store, ids, total + 2)  # the rows past the total stay as they were
    assert st == _abi.ZK_OK and list(zip(*[cols[k][:total].tolist() for k, _ in COLUMNS])) == want_rows
    assert all((c[total:].view(np.uint8) == SENTINEL).all() for c in cols.values())


# ---- 9. summaries end to end ---------------------------------------------------------------------------------
def test_summaries_end_to_end(make, gpu):
    S = 11
    cols = tracegen_host(seed=21, num_traces=300, max_depth=5, num_services=S)
    cols.set_name_ids((cols.span_id % np.uint64(6)).astype(np.int64))
    untimed = batch([R.id_in_bucket(3, 1)] * 4, seed=11)
    untimed.flags[:] &= ~np.uint32(R.TIMED)
    untimed.service_id[:] %= np.uint32(S)  # (the store below has a dictionary of S names)
    parts = R.shuffled_batches(SpanColumns.concat([cols, untimed]), 4, seed=21)
    names = [f"Service{i}" for i in range(S)]
    store = make(services=names)
    plain = make()
    observe_all(store, parts)
    observe_all(plain, parts, device=False)
    model = R.rows_of(parts)
    ids = sorted({r[0] for r in model})
    assert len(ids) == 301 and store.info()["segments"] == 4
    ask = ids[::-1] + [ids[0] ^ 1]
    assert store.tracesExist(ask) == set(ids)
    by_id = {rows[0][0]: rows for rows in R.spans_by_trace_ids(model, ids)}
    want = [s for s in (R.summary(by_id[i], names) for i in ask if i in by_id) if s is not None]
    got = store.getTraceSummariesByIds(ask)
    assert len(want) == 300
    assert [(s.trace_id, s.start, s.end, s.duration_micro, [tuple(x) for x in s.span_timestamps], s.endpoints) for s in got] == want
    assert [tuple(s[:4]) for s in want] == [tuple(s[:4]) for s in plain.getTraceSummariesByIds(ask)]
    for t in plain.getTracesByIds(ask):
        assert t.toSpanDepths() == R.span_depths(by_id[t.id])
        assert t.serviceCounts() == R.service_counts(by_id[t.id])
    # only untimed fragments: the trace exists and has no summary
    u = int(untimed.trace_id[0])
    assert store.tracesExist([u]) == {u} and len(store.getSpansByTraceId(u)) == 4 and store.getTraceSummariesByIds([u]) == []
    # the duration index over the same batches agrees on (start, end - start)
    with TraceDurationIndex(device=gpu) as td:
        for p in parts:
            td.observe(DeviceColumns.from_host(p))
        d = {x.trace_id: (x.start_timestamp, x.duration) for x in td.getTracesDuration(ask)}
    assert u not in d and set(d) == {s.trace_id for s in got}
    assert all(d[s.trace_id] == (s.start, s.end - s.start) for s in got)


# ---- 10. the job ---------------------------------------------------------------------------------------------------
def test_job_observes_its_batches(make, gpu):
    from tests.bulkfrag import service_name
    from zipkin_amd.aggregates import Dictionary, ZipkinAggregateJob

    S = 23
    cols = tracegen_host(71, 400, max_depth=5, num_services=S)
    part = (cols.trace_id % np.uint64(3)).astype(np.int64)
    rng = np.random.default_rng(71)
    parts = [cols.take(rng.permutation(np.flatnonzero(part == k))) for k in range(3)]
    names = Dictionary([service_name(i) for i in range(S)])
    plain = ZipkinAggregateJob(names, device=gpu, clock=lambda: 10 ** 15)
    want = plain.run(parts, S)
    plain.close()
    store = make()
    job = ZipkinAggregateJob(names, device=gpu, clock=lambda: 10 ** 15, spans=store)
    got = job.run(parts, S)
    job.close()
    assert want is not None and got == want
    assert store.info()["segments"] == 3
    check(store, R.rows_of(parts))


# ---- 11. composition with the trace-id index ------------------------------------------------------------
def test_ids_of_the_name_index_have_summaries(make, gpu):
    S = 9
    cols = tracegen_host(seed=31, num_traces=200, max_depth=5, num_services=S)
    cols.set_name_ids(1 + (cols.span_id % np.uint64(4)).astype(np.int64))
    parts = R.shuffled_batches(cols, 3, seed=31)
    store = make()
    with TraceNameIndex(S, device=gpu) as idx:
        for p in parts:
            d = DeviceColumns.from_host(p)
            idx.observe(d)
            store.observe(d)
        asked = 0
        for s in range(S):
            for nm in (None, 2):
                ids = [t.trace_id for t in idx.getTraceIdsByName(s, nm, R.INT64_MAX, 4096)]
                asked += len(ids)
                uniq = sorted(set(ids))
                assert store.tracesExist(uniq) == set(uniq)
                assert [x.trace_id for x in store.getTraceSummariesByIds(uniq)] == uniq  # an indexed fragment is timed
    assert asked > 200


# ---- timing ----------------------------------------------------------------------------------------------------------
def test_timing(make):
    b = batch(np.arange(3000) % 100, seed=12)
    store = make(timing=True)
    with pytest.raises(ZkError):
        store.observe_ms()
    with pytest.raises(ZkError):
        store.query_ms()
    observe_all(store, [b])
    ms = store.observe_ms()
    assert tuple(ms) == TraceSpanStore.OBSERVE_PHASES and all(v >= 0 for v in ms.values())
    store.exist([1, 2])
    assert store.query_ms() >= 0
    store.gather([1, 2])
    assert store.query_ms() >= 0
    plain = make()
    observe_all(plain, [b])
    with pytest.raises(ZkError):
        plain.observe_ms()
