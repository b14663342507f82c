"""The host side of the trace-id index by service and span name (include/zkindex.h,
zipkin_amd/nameindex.py): the reference of the GPU tests against the validator's vectors, the host
merge of per-shard results, the resolution of names given as strings and the refusals that touch no
device. No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import ixref
from zipkin_amd import IndexedTraceId, TraceNameIndex, ZkError, _abi, merge_trace_ids
from zipkin_amd.nameindex import _fold_ids


def test_reference_reproduces_the_validators_vectors():
    g = ixref.golden()
    b, services, names = ixref.golden_batch(g)
    entries = ixref.entries_of(b, len(services))
    assert entries == [(0, 1, 20, 123)]
    sid = {s: i for i, s in enumerate(services)}
    nid = {n: i + 1 for i, n in enumerate(names)}
    for q in g["trace_ids_by_name"]:
        if q["service"] not in sid or (q["span_name"] is not None and q["span_name"] not in nid):
            assert q["head_trace_id"] is None  # (a name no dictionary holds: nothing to ask)
            continue
        name = ixref.ANY if q["span_name"] is None else nid[q["span_name"]]
        rows, matched = ixref.trace_ids(entries, sid[q["service"]], name, q["end_ts"], q["limit"])
        assert rows[0][0] == q["head_trace_id"] and matched == 1
    for svc, want in g["span_names"].items():
        assert [names[i - 1] for i in ixref.span_names(entries, sid[svc])] == want
    assert [services[s] for s in sorted(ixref.service_counts(entries))] == g["service_names"]


def test_reference_predicate_and_order():
    b = ixref.batch([0, 0, 0, 0, 1, 0], [1, 1, 2, 0, 1, 1], [5, 9, 9, 9, 9, 7], [8, 2 ** 64 - 1, 0, 3, 4, 6],
                    timed=[True, True, True, True, True, False])
    e = ixref.entries_of(b, 2)
    assert len(e) == 5
    assert ixref.trace_ids(e, 0, ixref.ANY, 9, 10) == ([(0, 9), (3, 9), (2 ** 64 - 1, 9), (8, 5)], 4)
    assert ixref.trace_ids(e, 0, 1, 8, 10) == ([(8, 5)], 1)
    assert ixref.span_names(e, 0) == [1, 2]
    with pytest.raises(ValueError):
        ixref.entries_of(b, 1)
    client = ixref.batch([3, 3, 3, 2], [1] * 4, [1] * 4, [1, 2, 3, 4], cs=[1, 0, 0, 1], cr=[0, 1, 0, 0], sr=[0, 0, 2, 0])
    assert [x[3] for x in ixref.entries_of(client, 4, client_service=3)] == [3, 4]
    assert len(ixref.entries_of(client, 4)) == 4


def test_merge_trace_ids():
    a = [IndexedTraceId(7, 30), IndexedTraceId(7, 30), IndexedTraceId(1, 10)]
    b = [IndexedTraceId(2 ** 64 - 1, 30), IndexedTraceId(0, 30), IndexedTraceId(7, 30), IndexedTraceId(5, 20)]
    want = [(0, 30), (7, 30), (7, 30), (7, 30), (2 ** 64 - 1, 30), (5, 20), (1, 10)]
    got = merge_trace_ids([a, b, []], 100)  # limit larger than the union: all of it, duplicates kept
    assert [tuple(t) for t in got] == want and all(isinstance(t, IndexedTraceId) for t in got)
    assert [tuple(t) for t in merge_trace_ids([a, b], 4)] == want[:4]
    assert merge_trace_ids([], 5) == [] and merge_trace_ids([a], 0) == []
    # the split of a whole: the limit best of the union are among each shard's limit best
    rng = np.random.default_rng(5)
    rows = [(int(t), int(ts)) for t, ts in zip(rng.integers(0, 50, 400), rng.integers(0, 9, 400))]
    shards = [[r for r in rows if r[0] % 3 == k] for k in range(3)]
    order = lambda l: sorted(l, key=lambda r: (-r[1], r[0]))
    for limit in (1, 17, 1000):
        got = merge_trace_ids([order(s)[:limit] for s in shards], limit)
        assert [tuple(t) for t in got] == order(rows)[:limit]


def bare(services=None, span_names=None, S=8):
    """A TraceNameIndex without a handle: only its name resolution is used."""
    idx = object.__new__(TraceNameIndex)
    idx._h = None
    idx.num_services, idx.services, idx.span_names = S, services, span_names
    return idx


def test_names_given_as_strings():
    idx = bare(services=["Web", "db", "WEB", "client"], span_names=["GET", "get", "Put"])
    assert idx._service_ids("web") == [0, 2] and idx._service_ids("DB") == [1] and idx._service_ids("cache") == []
    assert idx._name_ids("Get") == [1, 2] and idx._name_ids("put") == [3] and idx._name_ids("post") == []
    assert idx._name_ids(None) == [_abi.ZK_IX_ANY_NAME] and idx._name_ids(7) == [7] and idx._service_ids(5) == [5]
    assert _fold_ids(["a", "A"], "a", 1) == [1, 2]
    # an unknown string asks nothing of the device: [] and set() without a handle
    assert idx.getTraceIdsByName("cache", None, 100, 3) == [] and idx.matched == 0
    assert idx.getTraceIdsByName("web", "post", 100, 3) == []
    assert idx.getSpanNames("cache") == set()
    with pytest.raises(ValueError):
        bare()._service_ids("web")
    with pytest.raises(ValueError):
        bare(services=["web"])._name_ids("get")
    with pytest.raises(ValueError):
        idx.getTraceIdsByServiceName("", 100, 3, None, None)
    # a dictionary longer than num_services: ids the handle cannot hold are not asked
    assert bare(services=["a", "b", "A"], S=2)._service_ids("a") == [0]


def test_every_call_refuses_null_without_touching_a_device():
    L = _abi.lib()
    h = C.c_void_p()
    cfg = _abi.zk_ix_config()
    cfg.num_services = 4
    n, m = C.c_uint32(), C.c_uint64()
    ids, ts, names, d = (C.c_uint64 * 4)(), (C.c_int64 * 4)(), (C.c_uint16 * 4)(), C.c_double()
    assert L.zk_ix_create(None, C.byref(h)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_create(C.byref(cfg), None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_destroy(None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_observe(None, None, 0) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_reset(None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_compact(None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_info(None, None, None, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_service_counts(None, ids) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_trace_ids(None, 0, 1, 0, 1, ids, ts, C.byref(n), C.byref(m)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_span_names(None, 0, names, 4, C.byref(n)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_observe_ms(None, C.byref(d)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_query_ms(None, C.byref(d)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ix_last_error(None) == b"null handle"


@pytest.mark.parametrize("S", (0, 4097, 2 ** 32 - 1))
def test_create_refuses_a_service_count_out_of_range(S):
    L = _abi.lib()
    h = C.c_void_p(1)
    cfg = _abi.zk_ix_config()
    cfg.num_services = S
    assert L.zk_ix_create(C.byref(cfg), C.byref(h)) == _abi.ZK_ERR_INVALID_ARG
    assert not h.value
    with pytest.raises(ZkError) as e:
        TraceNameIndex(S)
    assert e.value.status == _abi.ZK_ERR_INVALID_ARG


def test_constants():
    assert (_abi.ZK_IX_MAX_LIMIT, _abi.ZK_IX_MAX_SEGMENTS, _abi.ZK_IX_MAX_SERVICES) == (4096, 64, 4096)
    assert _abi.ZK_IX_NO_CLIENT == _abi.ZK_IX_ANY_NAME == 0xFFFFFFFF
    assert (ixref.TIMED, ixref.SVC_CLIENT, ixref.SVC_SERVER) == (_abi.ZK_F_HAS_ANNOTATIONS, _abi.ZK_F_SVC_CLIENT, _abi.ZK_F_SVC_SERVER)
    assert (ixref.CS, ixref.CR, ixref.SR, ixref.SS, ixref.NAME_SHIFT) == (
        _abi.ZK_F_CS_SHIFT, _abi.ZK_F_CR_SHIFT, _abi.ZK_F_SR_SHIFT, _abi.ZK_F_SS_SHIFT, _abi.ZK_F_NAME_SHIFT)
