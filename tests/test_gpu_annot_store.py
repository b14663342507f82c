"""The annotation store by trace id on the device (include/zkannots.h, zipkin_amd/annotstore.py) against
tests/anref.py, and the adjusted summaries and timelines of a TraceSpanStore with a TraceAnnotationStore against
tests/tsaref.py on the hand-worked vectors (tests/golden/time_skew.json). Every comparison is exact equality;
nothing depends on the order inside a bucket's slice."""
import ctypes as C

import numpy as np
import pytest

from tests import anref as R
from tests import spref as S
from tests import tsaref as T
from zipkin_amd import AnnotationRows, DeviceAnnotationRows, DeviceColumns, TraceAnnotationStore, TraceSpanStore, ZkError, _abi
from zipkin_amd.annotstore import ROW_COLUMNS

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
COUNT_TILE = 1024      # k_an_count's tile: 256 threads x 4 rows
SCATTER_ROW = 256      # k_an_scatter's row: one row per thread
SCATTER_CHUNK = 16384  # k_an_scatter's stretch per workgroup: one more makes a second workgroup
FIND_PART = 4096       # the lookups split a slice longer than this over several workgroups
SENTINEL = 0xA5


@pytest.fixture()
def make(gpu):
    made = []

    def factory(**kw):
        made.append(TraceAnnotationStore(device=gpu, **kw))
        return made[-1]

    yield factory
    for s in made:
        s.close()


def batch(trace_id, seed=0) -> AnnotationRows:
    return AnnotationRows(*R.noise(trace_id, seed))


def observe_all(store, batches, device=True):
    for b in batches:
        store.observe(DeviceAnnotationRows.from_host(b, store.device) if device else b)


def check(store, model, extra_ids=()):
    """Everything the store answers about every trace of the model (and the extra ids) equals the model."""
    ids = sorted({r[0] for r in model}) + list(extra_ids)
    assert store.info()["entries"] == len(model)
    assert store.getAnnotationsByTraceIds(ids) == R.by_trace_ids(model, ids)


def raw_gather(store, ids, cap, flags=0, ptr=None):
    """zk_an_gather into sentinel-filled columns of `cap` entries: (status, n_out, counts, columns)."""
    ids = np.ascontiguousarray(np.asarray(ids, np.uint64))
    counts = np.full(len(ids), 0xDEADBEEF, np.uint32)
    cols = {k: np.frombuffer(bytes([SENTINEL]) * (max(cap, 1) * np.dtype(dt).itemsize), dt).copy() for k, dt in ROW_COLUMNS}
    out = _abi.zk_an_cols(*[cols[k].ctypes.data for k, _ in ROW_COLUMNS])
    total = C.c_uint64(12345)
    st = store._L.zk_an_gather(store._h, ids.ctypes.data if ptr is None else ptr, len(ids), flags,
                               counts.ctypes.data_as(_abi._U32P), C.byref(out), cap, C.byref(total))
    return st, int(total.value), counts.tolist(), cols


def listed(cols):
    return list(zip(*[cols[k].tolist() for k, _ in ROW_COLUMNS]))


# ---- 1. one row, the bounds of every column -----------------------------------------------------------------
def test_one_row_and_the_columns_bounds(make):
    store = make()
    assert store.info() == {"entries": 0, "segments": 0, "bytes": 0}
    for tid in (0, U64):
        for ts in (R.INT64_MIN, R.INT64_MAX):
            store.reset()
            b = AnnotationRows.of_rows([(tid, U64 - tid, ts, U64, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)])
            observe_all(store, [b], device=ts < 0)
            info = store.info()
            assert (info["entries"], info["segments"]) == (1, 1) and info["bytes"] >= 44
            check(store, R.rows_of(b), extra_ids=[1, U64 - 1, U64 - tid])
            assert store.getAnnotationsByTraceIds([tid])[0] == [(tid, U64 - tid, ts, U64, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)]
    # every bit of ipv4 and bits, both bounds of ts, in one trace: the order's keys at their extremes
    rows = [(7, s, ts, v, ip, svc, bits) for s in (0, U64) for ts in (R.INT64_MIN, -1, 0, R.INT64_MAX) for v in (0, U64)
            for ip in (0, 0x80000000, 0xFFFFFFFF) for svc in (0, 0xFFFFFFFF) for bits in (0, 7, 8, 0xFFFF0000, 0xFFFFFFFF, 0x0000FFF0)]
    store.reset()
    b = AnnotationRows.of_rows(rows)
    observe_all(store, [b.take(np.random.default_rng(1).permutation(len(b)))])
    assert store.getAnnotationsByTraceIds([7])[0] == sorted(rows, key=R.key)
    store.reset()
    assert store.info() == {"entries": 0, "segments": 0, "bytes": 0} and store.getAnnotationsByTraceIds([7]) == [[]]


# ---- 2. batch sizes ------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, SCATTER_ROW - 1, SCATTER_ROW, SCATTER_ROW + 1, COUNT_TILE - 1, COUNT_TILE, COUNT_TILE + 1,
         SCATTER_CHUNK - 1, SCATTER_CHUNK, SCATTER_CHUNK + 1)


# (host batches differ from device batches only in the staging copy: three sizes of them)
@pytest.mark.parametrize("n,device", [(n, True) for n in SIZES] + [(n, False) for n in (1, 257, COUNT_TILE + 1)],
                         ids=lambda v: ("device" if v else "host") if isinstance(v, bool) else str(v))
def test_batch_sizes(make, n, device):
    rng = np.random.default_rng(n)
    pool = np.unique(rng.integers(0, 2 ** 64, max(1, n // 5), dtype=np.uint64))
    b = batch(pool[rng.integers(0, len(pool), n)], seed=n)
    store = make()
    observe_all(store, [b], device=device)
    assert store.info()["segments"] == 1
    check(store, R.rows_of(b), extra_ids=[int(pool[0]) ^ 1])


# ---- 3. buckets ----------------------------------------------------------------------------------------------
def test_buckets(make):
    # every row in ONE bucket: the other 4095 are empty
    one = make()
    ids = [R.id_in_bucket(77, k) for k in range(40)]
    assert {R.bucket(i) for i in ids} == {77}
    b1 = batch(np.repeat(np.array(ids[:39], np.uint64), 30), seed=5)
    observe_all(one, [b1])
    check(one, R.rows_of(b1), extra_ids=[ids[39], R.id_in_bucket(76, 0), R.id_in_bucket(78, 0)])
    # 4096 distinct buckets, the first and the last with several traces
    every = [R.id_in_bucket(b, 0) for b in range(4096)] + [R.id_in_bucket(0, k) for k in (1, 2)] + [R.id_in_bucket(4095, 1)] * 2
    store = make()
    b = batch(np.random.default_rng(4).permutation(np.array(every, np.uint64)), seed=4)
    observe_all(store, [b])
    check(store, R.rows_of(b), extra_ids=[R.id_in_bucket(0, 3), R.id_in_bucket(4095, 2), R.id_in_bucket(2048, 1)])


# ---- 4. a trace longer than a lookup's part ------------------------------------------------------------------
def test_long_trace(make):
    n = FIND_PART + 1
    long_id, other, absent = (R.id_in_bucket(9, k) for k in range(3))
    tids = np.full(n + 700, long_id, np.uint64)
    tids[np.arange(700) * ((n + 700) // 700)] = other  # interleaved in the same bucket
    b = batch(tids, seed=6)
    store = make()
    observe_all(store, [b])
    model = R.rows_of(b)
    assert sum(r[0] == long_id for r in model) == n
    counts, rows = store.gather([long_id, absent, other])
    assert counts.tolist() == [n, 0, 700] and rows.rows() == R.gather(model, [long_id, absent, other])[1]
    # the same trace spread over two segments: parts of both are walked
    observe_all(store, [b.take(slice(0, 900))], device=False)
    check(store, model + R.rows_of(b.take(slice(0, 900))), extra_ids=[absent])


# ---- 5. segments ---------------------------------------------------------------------------------------------
def test_segments_merge_compact_and_reset(make):
    rng = np.random.default_rng(8)
    pool = np.unique(rng.integers(0, 2 ** 64, 40, dtype=np.uint64))
    spread = int(pool[0])
    store = make()
    batches = [batch([spread] * 3 + pool[rng.integers(0, len(pool), 20)].tolist(), seed=80 + k) for k in range(2)]
    observe_all(store, batches[:1])
    assert store.info()["segments"] == 1
    check(store, R.rows_of(batches[:1]))
    observe_all(store, batches[1:])
    assert store.info()["segments"] == 2 and len(store.getAnnotationsByTraceIds([spread])[0]) >= 6
    check(store, R.rows_of(batches))
    for k in range(62):  # 64 segments: the bound
        batches.append(batch(pool[rng.integers(0, len(pool), 1 + k % 3)], seed=100 + k))
        observe_all(store, batches[-1:], device=k % 2 == 0)
    model = R.rows_of(batches)
    assert store.info()["segments"] == _abi.ZK_AN_MAX_SEGMENTS == 64
    check(store, model)
    batches.append(batch(pool[:2], seed=200))  # the 65th observe merges the 64 first
    observe_all(store, batches[-1:])
    model = R.rows_of(batches)
    info = store.info()
    assert (info["segments"], info["entries"]) == (2, len(model))
    check(store, model)
    store.compact()
    after = store.info()
    assert (after["segments"], after["entries"]) == (1, info["entries"])
    check(store, model)
    store.compact()  # one segment: nothing to do
    assert store.info() == after
    observe_all(store, batches[:1])  # an observe after the compact; the same batch again adds it again
    check(store, model + R.rows_of(batches[0]))
    store.reset()
    assert store.info() == {"entries": 0, "segments": 0, "bytes": 0}
    observe_all(store, batches[1:2])  # an observe after the reset
    assert store.info()["segments"] == 1
    check(store, R.rows_of(batches[1]), extra_ids=[spread ^ 1])


# ---- 6. the ask ----------------------------------------------------------------------------------------------
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
    counts, rows = store.gather(present[:1])  # one id
    assert (counts.tolist(), rows.rows()) == R.gather(model, present[:1])
    ids = [present[0], absent[0], present[1], present[0], absent[1], present[0], U64, 0]
    counts, rows = store.gather(ids)
    assert (counts.tolist(), rows.rows()) == R.gather(model, ids)
    # ZK_AN_MAX_IDS ids in one call, duplicates and absent ids among them; one more is refused
    big = (present + absent + present)[:_abi.ZK_AN_MAX_IDS]
    assert len(big) == _abi.ZK_AN_MAX_IDS == 4096
    counts, rows = store.gather(big)
    assert (counts.tolist(), rows.rows()) == R.gather(model, big)
    with pytest.raises(ZkError) as e:
        store.gather(big + [1])
    assert e.value.status == _abi.ZK_ERR_INVALID_ARG and "ZK_AN_MAX_IDS" in e.value.message
    assert store.getAnnotationsByTraceIds(big + [1]) == R.by_trace_ids(model, big + [1])  # (the Python call asks in parts)
    # device-pointer ids
    dev = torch.from_numpy(np.array(ids, np.uint64).view(np.int64)).to(f"cuda:{gpu}")
    counts, rows = store.gather(dev)
    assert (counts.tolist(), rows.rows()) == R.gather(model, ids)


# ---- 7. capacity ---------------------------------------------------------------------------------------------
def test_capacity(make):
    b = batch([5] * 7 + [6] * 3 + [9], seed=10)
    model = R.rows_of(b)
    store = make()
    observe_all(store, [b])
    ids = [6, 404, 5, 6]
    want_counts, want_rows = R.gather(model, ids)
    total = sum(want_counts)
    assert total == 13
    counts, n_out = np.zeros(4, np.uint32), C.c_uint64()  # the sizing call: NULL columns
    st = store._L.zk_an_gather(store._h, np.array(ids, np.uint64).ctypes.data, 4, 0, counts.ctypes.data_as(_abi._U32P), None, 0, C.byref(n_out))
    assert (st, n_out.value, counts.tolist()) == (_abi.ZK_ERR_CAPACITY, total, want_counts)
    for cap in (total - 1, 0):
        st, n_out, counts, cols = raw_gather(store, ids, cap)
        assert (st, n_out, counts) == (_abi.ZK_ERR_CAPACITY, total, want_counts)
        assert all((c.view(np.uint8) == SENTINEL).all() for c in cols.values())
    st, n_out, counts, cols = raw_gather(store, ids, total)
    assert (st, n_out, counts) == (_abi.ZK_OK, total, want_counts) and listed(cols) == want_rows
    st, n_out, counts, cols = raw_gather(store, ids, total + 2)  # the rows past the total stay as they were
    assert st == _abi.ZK_OK and listed({k: v[:total] for k, v in cols.items()}) == want_rows
    assert all((c[total:].view(np.uint8) == SENTINEL).all() for c in cols.values())


# ---- 8. both stores: adjusted summaries and timelines on the hand-worked vectors -----------------------------
def test_adjusted_summaries_and_timelines_of_the_golden_traces(make, gpu):
    cases = T.golden()["cases"]
    rows = [T.golden_rows(c) for c in cases]
    span_rows = [r for s, _ in rows for r in s]
    ann_rows = [r for _, a in rows for r in a]
    rng = np.random.default_rng(12)
    annots = make()
    with TraceSpanStore(device=gpu) as spans:
        for part in np.array_split(rng.permutation(len(span_rows)), 3):  # the same fragments, shuffled, in three batches each
            spans.observe(DeviceColumns.from_host(S.cols_of([span_rows[i] for i in part])))
        for part in np.array_split(rng.permutation(len(ann_rows)), 3):
            annots.observe(DeviceAnnotationRows.from_host(AnnotationRows.of_rows([ann_rows[i] for i in part]), gpu))
        ids = [c["trace_id"] for c in cases][::-1] + [404]
        want = [T.adjust(T.annotated(s, a)) for s, a in rows][::-1]
        sums = spans.getTraceSummariesByIds(ids, adjust=("TIME_SKEW",), annotations=annots)
        assert [(s.trace_id, s.start, s.end, s.duration_micro, [tuple(x) for x in s.span_timestamps], s.endpoints) for s in sums] == \
            [T.summary(w, i) for w, i in zip(want, ids)]
        assert [[s.start, s.end] for s in sums] == [c["expect"]["start_end"] for c in cases][::-1]
        lines = spans.getTraceTimelinesByIds(ids, adjust=("TIME_SKEW",), annotations=annots)
        assert [(t.trace_id, t.root_span_id, [tuple(a) for a in t.annotations]) for t in lines] == [T.timeline(w, i) for w, i in zip(want, ids)]
        raw = spans.getTraceTimelinesByIds(ids, annotations=annots)
        assert [(t.trace_id, t.root_span_id, [tuple(a) for a in t.annotations]) for t in raw] == \
            [T.timeline(T.annotated(s, a), i) for (s, a), i in zip(rows[::-1], ids)]
        # without adjust= and annotations= the answers are today's
        assert [tuple(s[:4]) for s in spans.getTraceSummariesByIds(ids)] == [S.summary(s)[:4] for s, _ in rows[::-1]]
        assert spans.getTraceSummariesByIds(ids) == spans.getTraceSummariesByIds(ids, on_device=True)
        assert all(c.timeline is None for c in spans.getTraceCombosByIds(ids))
        combos = spans.getTraceCombosByIds(ids, adjust=("TIME_SKEW",), annotations=annots)
        assert [c.timeline for c in combos] == lines and [c.summary for c in combos] == sums


# ---- timing ----------------------------------------------------------------------------------------------------
def test_timing(make):
    b = batch(np.arange(3000) % 100, seed=12)
    store = make(timing=True)
    with pytest.raises(ZkError):
        store.observe_ms()
    with pytest.raises(ZkError):
        store.query_ms()
    observe_all(store, [b])
    ms = store.observe_ms()
    assert tuple(ms) == TraceAnnotationStore.OBSERVE_PHASES and all(v >= 0 for v in ms.values())
    store.gather([1, 2])
    assert store.query_ms() >= 0
    plain = make()
    observe_all(plain, [b])
    with pytest.raises(ZkError):
        plain.observe_ms()
