"""Trace summaries on the device (zk_sp_summaries, TraceSpanStore.summaries, getTraceSummariesByIds with
on_device=True) against the model of the call's output (tests/spsumref.py, built on tests/spref.py) and
against the default host path. Every comparison is exact equality; nothing depends on the order in which
the device appended a trace's rows."""
import ctypes as C

import numpy as np
import pytest

from tests import spref as R
from tests import spsumref as M
from zipkin_amd import SUMMARY_HEAD, DeviceColumns, TraceSpanStore, ZkError, _abi

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
MAX_ROWS = _abi.ZK_SP_SUM_MAX_ROWS   # the longest trace merged on the device
WAVE = _abi.ZK_SP_SUM_WAVE_ROWS      # up to here a wave takes the trace, above it a workgroup
SPAN_POOL = (0, 1, 2 ** 63, U64)     # the unsigned order's corners
TIMES = (-5, 0, 7, 1000)
SENTINEL = 0xA5
ENTRY = (("service_id", np.uint32), ("first", np.int64), ("last", np.int64))


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
        b = R.cols_of(b) if isinstance(b, list) else b
        store.observe(DeviceColumns.from_host(b) if device else b)


def gen_trace(rng, tid, n, n_spans=None, n_services=3, times=TIMES):
    """n rows of one trace: few span ids (the pool's corners first), few services, every combination of the
    four low flag bits with non-zero name bits, times from four values, every fifth row a copy of the one
    before it."""
    k = int(rng.integers(1, 9)) if n_spans is None else n_spans
    spans = [int(x) for x in rng.permutation(np.array(SPAN_POOL, np.uint64))][:k]
    spans += [int(x) for x in rng.integers(2, 2 ** 63, max(0, k - len(spans)), dtype=np.uint64)]
    rows = []
    for i in range(n):
        fl = ((i + int(rng.integers(0, 16))) % 16) | (int(rng.integers(1, 2 ** 16)) << R.NAME_SHIFT)
        rows.append((tid, spans[int(rng.integers(len(spans)))], int(rng.integers(0, 3)), times[int(rng.integers(4))],
                     times[int(rng.integers(4))], int(rng.integers(n_services)), fl))
        if i % 5 == 4:
            rows[i] = rows[i - 1]
    return rows


def entries_of(cols):
    return list(zip(*[cols[k].tolist() for k, _ in ENTRY]))


def check(store, model, ids):
    """summaries() against the model, and the device path of getTraceSummariesByIds against the host path."""
    heads, cols = store.summaries(ids)
    want_heads, want_entries = M.summaries(model, ids, MAX_ROWS)
    assert heads.dtype == SUMMARY_HEAD and heads.tolist() == want_heads
    assert entries_of(cols) == want_entries
    host = store.getTraceSummariesByIds(ids)
    assert store.getTraceSummariesByIds(ids, on_device=True) == host
    return heads, host


def raw(store, ids, cap, flags=0, ptr=None):
    """zk_sp_summaries into sentinel-filled heads and columns of `cap` entries: (status, n_out, heads, columns)."""
    ids = np.ascontiguousarray(np.asarray(ids, np.uint64))
    heads = np.frombuffer(bytes([SENTINEL]) * (max(len(ids), 1) * 40), SUMMARY_HEAD).copy()
    cols = {k: np.frombuffer(bytes([SENTINEL]) * (max(cap, 1) * np.dtype(dt).itemsize), dt).copy() for k, dt in ENTRY}
    out = _abi.zk_sp_span_ts(*[cols[k].ctypes.data for k, _ in ENTRY])
    total = C.c_uint64(12345)
    st = store._L.zk_sp_summaries(store._h, ids.ctypes.data if ptr is None else ptr, len(ids), flags, heads.ctypes.data,
                                  C.byref(out), cap, C.byref(total))
    return st, int(total.value), heads, cols


def untouched(a):
    return bool((a.view(np.uint8) == SENTINEL).all())


# ---- 1. the reference's vectors --------------------------------------------------------------------------
@pytest.mark.parametrize("device", (True, False), ids=("device_batches", "host_batches"))
def test_golden_vectors(make, device):
    g = R.golden()
    store = make(services=g["services"], span_names=g["span_names"])
    for case in g["cases"]:
        store.reset()
        rows = R.golden_rows(case, g["services"])
        observe_all(store, [rows], device=device)
        tid = case["trace_id"]
        heads, host = check(store, rows, [tid])
        want = R.summary(rows, g["services"])
        got = store.getTraceSummariesByIds([tid], on_device=True)
        assert [(s.trace_id, s.start, s.end, s.duration_micro, [tuple(x) for x in s.span_timestamps], s.endpoints)
                for s in got] == ([] if want is None else [want])
        if rows:
            assert heads[0]["spans"] == len(case["expect"]["span_order"])


# ---- 2. sizes ------------------------------------------------------------------------------------------------
def plan_bounds():
    """Every row count at which the plan takes another path: the wave / workgroup switch, and the powers of
    two between it and the bound (the sort's length and the workgroups' LDS are sized by the next power)."""
    out, b = [], WAVE
    while b < MAX_ROWS:
        out.append(b)
        b *= 2
    return out


SMALL = sorted({1, 2, 63, 64, 65, 255, 256, 257} | {b + d for b in plan_bounds() for d in (-1, 0, 1)} | {WAVE // 2 + 1})


def test_sizes_up_to_the_bound(make):
    assert {WAVE - 1, WAVE, WAVE + 1} <= set(SMALL) and max(SMALL) < MAX_ROWS - 1
    rng = np.random.default_rng(2)
    store = make()
    model, ids = [], []
    for k, n in enumerate(SMALL):
        ids.append(R.id_in_bucket(k % 7, 100 + k))  # (several traces share a bucket)
        model += gen_trace(rng, ids[-1], n, n_spans=max(1, min(n // 3, 300)))
    perm = rng.permutation(len(model))
    observe_all(store, [[model[i] for i in perm]])
    heads, _ = check(store, model, ids)
    assert heads["fragments"].tolist() == SMALL and not (heads["state"] & M.OVERFLOW).any()
    # one trace per call: the workgroups' LDS is then sized by that trace alone
    for i in ids:
        h, c = store.summaries([i])
        assert (h.tolist(), entries_of(c)) == M.summaries(model, [i], MAX_ROWS)


@pytest.mark.parametrize("n", (MAX_ROWS - 1, MAX_ROWS, MAX_ROWS + 1))
def test_sizes_at_the_bound(make, n):
    rng = np.random.default_rng(n)
    tid, small = R.id_in_bucket(5, 1), R.id_in_bucket(5, 2)
    model = gen_trace(rng, tid, n, n_spans=700) + gen_trace(rng, small, 3)
    store = make()
    observe_all(store, [[model[i] for i in rng.permutation(len(model))]])
    heads, host = check(store, model, [small, tid, small])
    over = n > MAX_ROWS
    assert heads["fragments"].tolist() == [3, n, 3]
    assert [bool(s & M.OVERFLOW) for s in heads["state"].tolist()] == [False, over, False]
    if over:
        se = R.start_end([r for r in model if r[0] == tid])
        assert heads[1].tolist() == (tid, se[0], se[1], n, 0, 0, M.FOUND | M.TIMED | M.OVERFLOW)
    assert [s.trace_id for s in host] == [small, tid, small]


# ---- 3. random traces ----------------------------------------------------------------------------------------
def test_random_traces(make):
    rng = np.random.default_rng(3)
    T, S = R.TIMED, R.SVC_CLIENT
    model, ids = [], []
    for k in range(60):
        ids.append(int(rng.integers(0, 2 ** 64, dtype=np.uint64)))
        model += gen_trace(rng, ids[-1], int(rng.integers(1, 150)))
    assert {r[6] & 15 for r in model} == set(range(16)) and all(r[6] >> R.NAME_SHIFT for r in model)
    assert len(set(model)) < len(model)
    wide, untimed, bare = (R.id_in_bucket(11, k) for k in range(3))
    model += [(wide, 1, 0, R.INT64_MIN, 5, 1, T | S), (wide, 2, 1, 6, R.INT64_MAX, 2, T | S), (wide, 2, 1, R.INT64_MAX, R.INT64_MIN, 0, S)]
    model += [(untimed, s, 0, R.INT64_MIN, R.INT64_MAX, s, S | (R.HAS_PARENT if s else 0)) for s in (0, 1, 1, 2)]
    model += [(bare, 9, 0, 3, 4, 7, T), (bare, 9, 0, 1, 2, 7, T | R.HAS_PARENT), (bare, 8, 9, 0, 9, 7, S)]
    ids += [wide, untimed, bare]
    store = make()
    batches = [[model[i] for i in part] for part in np.array_split(rng.permutation(len(model)), 3)]
    observe_all(store, batches)
    heads, host = check(store, model, ids)
    by = {h[0]: h for h in heads.tolist()}
    assert by[wide] == (wide, R.INT64_MIN, R.INT64_MAX, 3, 2, 3, M.FOUND | M.TIMED)
    assert by[untimed] == (untimed, 0, 0, 4, 3, 0, M.FOUND)
    assert by[bare] == (bare, 1, 4, 3, 2, 0, M.FOUND | M.TIMED)
    got = {s.trace_id: s for s in host}
    assert got[wide].duration_micro == -1 and untimed not in got and got[bare].span_timestamps == []
    # the append order does not show: the same multiset observed in another order and cut
    again = make()
    observe_all(again, [[model[i] for i in part] for part in np.array_split(rng.permutation(len(model)), 5)], device=False)
    h2, c2 = again.summaries(ids)
    h1, c1 = store.summaries(ids)
    assert h1.tolist() == h2.tolist() and entries_of(c1) == entries_of(c2)


# ---- 4. one bucket -------------------------------------------------------------------------------------------
def test_traces_of_one_bucket_do_not_merge(make):
    rng = np.random.default_rng(4)
    ids = [R.id_in_bucket(2047, k) for k in range(4)]
    assert {R.bucket(i) for i in ids} == {2047}
    model = []
    for i, n in zip(ids[:3], (40, 70, 9)):
        model += gen_trace(np.random.default_rng(44), i, n, n_spans=4)[:n]  # (the same spans and rows but the id)
        model += gen_trace(rng, i, 5, n_spans=4)
    store = make()
    observe_all(store, [[model[i] for i in rng.permutation(len(model))]])
    heads, host = check(store, model, ids + ids[:1])
    assert heads["fragments"].tolist() == [45, 75, 14, 0, 45] and len(host) == 4


# ---- 5. segments and expiry ------------------------------------------------------------------------------
def test_segments_compact_and_expire(make):
    rng = np.random.default_rng(5)
    spread, old, other = R.id_in_bucket(77, 0), R.id_in_bucket(77, 1), R.id_in_bucket(78, 0)
    parts = []
    for k in range(3):
        part = gen_trace(rng, spread, 30 + k, n_spans=6) + gen_trace(rng, other, 4)
        part += [(old, 1, 0, 0, 10, 1, R.TIMED | R.SVC_SERVER)] * 2
        parts.append(part)
    parts[1].append((spread, 1, 0, 2000, 3000, 2, R.TIMED | R.SVC_CLIENT))
    parts[2].append((other, 1, 0, 2000, 3000, 2, R.TIMED | R.SVC_CLIENT))
    model = parts[0] + parts[1] + parts[2]
    ids = [spread, old, other]
    store = make()
    observe_all(store, parts)
    assert store.info()["segments"] == 3
    before, _ = check(store, model, ids)
    assert before["fragments"].tolist() == [94, 6, 13]
    store.compact()
    assert store.info()["segments"] == 1
    after, _ = check(store, model, ids)
    assert after.tolist() == before.tolist()
    observe_all(store, [parts[0]])  # two segments again, then the neighbour in the bucket goes
    model += parts[0]
    assert store.expire(2500) == 8
    model = [r for r in model if r[0] != old]
    heads, _ = check(store, model, ids)
    assert heads.tolist()[1] == M.ZERO and heads["fragments"].tolist() == [94 + 30, 0, 13 + 4]


# ---- 6. the ask ------------------------------------------------------------------------------------------------
def test_the_ask(make, gpu):
    import torch

    rng = np.random.default_rng(6)
    model = []
    for tid in (0, U64, 5, 6):
        model += gen_trace(rng, tid, 20)
    store = make()
    assert store.getTraceSummariesByIds([0, 5], on_device=True) == []  # the empty store: no device pass
    st, total, heads, cols = raw(store, [0, 5, U64], 4)
    assert (st, total) == (_abi.ZK_OK, 0) and not heads.view(np.uint8).any() and all(untouched(c) for c in cols.values())
    observe_all(store, [model])
    ids = [5, 404, 0, 5, U64, 405, 5, 6]
    heads, host = check(store, model, ids)
    assert heads.tolist()[1] == heads.tolist()[5] == M.ZERO and heads.tolist()[0] == heads.tolist()[3] == heads.tolist()[6]
    assert [s.trace_id for s in host if s.trace_id == 5] == [5, 5, 5]
    # n == 0
    h0, c0 = store.summaries([])
    assert len(h0) == 0 and all(len(c) == 0 for c in c0.values())
    st, total, heads, cols = raw(store, [], 4)
    assert (st, total) == (_abi.ZK_OK, 0) and untouched(heads) and all(untouched(c) for c in cols.values())
    assert store.getTraceSummariesByIds([], on_device=True) == []
    # device-pointer ids
    dev = torch.from_numpy(np.array(ids, np.uint64).view(np.int64)).to(f"cuda:{gpu}")
    hd, cd = store.summaries(dev)
    want_heads, want_entries = M.summaries(model, ids, MAX_ROWS)
    assert hd.tolist() == want_heads and entries_of(cd) == want_entries
    # NULL arguments and one id too many, with a live handle
    a, t = np.array(ids, np.uint64), C.c_uint64()
    L, h = store._L, store._h
    assert L.zk_sp_summaries(h, None, 8, 0, hd.ctypes.data, None, 0, C.byref(t)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_sp_summaries(h, a.ctypes.data, 8, 0, None, None, 0, C.byref(t)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_sp_summaries(h, a.ctypes.data, 8, 0, hd.ctypes.data, None, 0, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_sp_summaries(h, a.ctypes.data, 8, 0, hd.ctypes.data, None, 3, C.byref(t)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_sp_summaries(h, a.ctypes.data, 8, 2, hd.ctypes.data, None, 0, C.byref(t)) == _abi.ZK_ERR_INVALID_ARG
    with pytest.raises(ZkError) as e:
        store.summaries(list(range(_abi.ZK_SP_MAX_IDS + 1)))
    assert e.value.status == _abi.ZK_ERR_INVALID_ARG and "ZK_SP_MAX_IDS" in e.value.message


def test_an_ask_of_the_most_ids_and_one_more(make):
    n = _abi.ZK_SP_MAX_IDS + 1
    rng = np.random.default_rng(7)
    tids = np.unique(rng.integers(0, 2 ** 64, n + 50, dtype=np.uint64))[:n].tolist()
    model = [(t, k % 3, 0, k, k + 1, k % 5, (k % 16) | (1 << R.NAME_SHIFT)) for k, t in enumerate(tids)]
    store = make()
    observe_all(store, [model])
    heads, cols = store.summaries(tids[:n - 1])  # exactly ZK_SP_MAX_IDS one-row traces in one call
    want_heads, want_entries = M.summaries(model, tids[:n - 1], MAX_ROWS)
    assert len(heads) == _abi.ZK_SP_MAX_IDS == 4096 and heads.tolist() == want_heads and entries_of(cols) == want_entries
    got = store.getTraceSummariesByIds(tids, on_device=True)  # 4097: the Python call asks in parts
    assert got == store.getTraceSummariesByIds(tids)
    assert [s.trace_id for s in got] == [r[0] for r in model if r[6] & R.TIMED]


# ---- 7. capacity -----------------------------------------------------------------------------------------------
def test_capacity(make):
    rng = np.random.default_rng(8)
    model = gen_trace(rng, 5, 30, n_spans=5) + gen_trace(rng, 6, 80, n_spans=5) + [(9, 1, 0, 1, 2, 3, R.TIMED | R.SVC_CLIENT)]
    store = make()
    observe_all(store, [model])
    ids = [6, 404, 5, 6, 9]
    want_heads, want_entries = M.summaries(model, ids, MAX_ROWS)
    total = len(want_entries)
    assert total > 10
    for cap in (0, total - 1):  # the sizing call, and one entry short
        st, n_out, heads, cols = raw(store, ids, cap)
        assert (st, n_out) == (_abi.ZK_ERR_CAPACITY, total) and heads.tolist() == want_heads
        assert all(untouched(c) for c in cols.values())
    st, n_out, heads, cols = raw(store, ids, total)
    assert (st, n_out) == (_abi.ZK_OK, total) and heads.tolist() == want_heads and entries_of(cols) == want_entries
    st, n_out, heads, cols = raw(store, ids, total + 2)  # the entries past the total stay as they were
    assert st == _abi.ZK_OK and entries_of({k: c[:total] for k, c in cols.items()}) == want_entries
    assert all(untouched(c[total:]) for c in cols.values())
    t = C.c_uint64()
    st = store._L.zk_sp_summaries(store._h, np.array(ids, np.uint64).ctypes.data, 5, 0, heads.ctypes.data, None, 0, C.byref(t))
    assert (st, t.value) == (_abi.ZK_ERR_CAPACITY, total)  # cap == 0 with NULL columns


# ---- 8. dictionaries -------------------------------------------------------------------------------------------
def test_dictionaries(make):
    rng = np.random.default_rng(9)
    model = gen_trace(rng, 5, 40) + gen_trace(rng, 6, 100)
    names = ["Alpha", "BETA", "gamma"]
    store = make(services=names)
    observe_all(store, [model])
    got = store.getTraceSummariesByIds([6, 5], on_device=True)
    assert got == store.getTraceSummariesByIds([6, 5])
    rows = {i: [r for r in model if r[0] == i] for i in (5, 6)}
    assert [[tuple(x) for x in s.span_timestamps] for s in got] == [R.span_timestamps(rows[i], names) for i in (6, 5)]
    assert {x.name for s in got for x in s.span_timestamps} == {"alpha", "beta", "gamma"}
    short = make(services=names[:2])
    observe_all(short, [model])
    for on_device in (False, True):
        with pytest.raises(ValueError):
            short.getTraceSummariesByIds([5, 6], on_device=on_device)


# ---- timing ----------------------------------------------------------------------------------------------------------
def test_timing(make):
    rng = np.random.default_rng(10)
    store = make(timing=True)
    observe_all(store, [gen_trace(rng, 5, 40) + gen_trace(rng, 6, 100)])
    with pytest.raises(ZkError):
        store.query_ms()
    store.summaries([5, 6, 7])
    assert store.query_ms() > 0
