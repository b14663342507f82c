"""The host side of the trace duration index (include/zkduration.h, zipkin_amd/durations.py): the
reference of the GPU tests against the validator's vectors, the refusals that touch no device, the
host merge of per-shard results and the order names. No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import tdref
from tests.wincases import INT64_MAX, INT64_MIN, Ids
from zipkin_amd import TraceIdDuration, _abi, merge_top
from zipkin_amd.durations import ORDERS


def test_reference_reproduces_the_validators_vectors():
    g = tdref.golden()
    for store in g["stores"]:
        batches = []
        for step in store["steps"]:
            batches.append(tdref.golden_batch(g, step["add"]))
            got = tdref.entries(tdref.table_of(batches), step["ask"])
            assert got == [tuple(e) for e in step["expect"]]


def test_reference_duration_wraps_like_a_long():
    assert tdref.duration(INT64_MIN, INT64_MAX) == -1
    assert tdref.duration(INT64_MAX, INT64_MIN) == 1
    assert tdref.duration(-5, 7) == 12 and tdref.duration(7, 7) == 0
    assert tdref.duration(0, INT64_MIN) == INT64_MIN


def test_order_names_are_the_thrift_enums_ordinals():
    enum = tdref.golden()["order_enum"]
    assert {name.upper().replace("-", "_"): v for name, v in ORDERS.items()} == {
        n: i for i, n in enumerate(enum) if n != "NONE"}
    assert (_abi.ZK_TD_TIMESTAMP_DESC, _abi.ZK_TD_TIMESTAMP_ASC, _abi.ZK_TD_DURATION_ASC, _abi.ZK_TD_DURATION_DESC) == (
        0, 1, 2, 3)
    assert sorted(ORDERS) == sorted(tdref.ORDERS)
    assert _abi.ZK_TD_TABLE_SALT != _abi.ZK_WIN_TABLE_SALT and _abi.ZK_TD_MAX_TOP == 4096


def test_create_refuses_null_without_touching_a_device():
    L = _abi.lib()
    h = C.c_void_p()
    cfg = _abi.zk_td_config()
    assert L.zk_td_create(None, C.byref(h)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_td_create(C.byref(cfg), None) == _abi.ZK_ERR_INVALID_ARG
    n = C.c_uint32()
    assert L.zk_td_destroy(None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_td_observe(None, None, 0) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_td_reset(None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_td_reserve(None, 5) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_td_info(None, None, None, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_td_lookup(None, None, 1, 0, None, None, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_td_top(None, 0, 0, 1, 1, None, None, None, C.byref(n), None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_td_observe_ms(None, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_td_top_ms(None, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_td_last_error(None) == b"null handle"


def tied_table(n=600, seed=3):
    """n traces whose durations and starts come from a handful of values, so most keys are tied."""
    rng = np.random.default_rng(seed)
    ids = Ids(seed)
    table = {}
    for _ in range(n):
        s = int(rng.integers(0, 6)) * 1000
        table[ids()] = (s, s + int(rng.integers(0, 5)) * 10)
    table[0] = (0, 0)
    table[2 ** 64 - 1] = (0, 0)
    return table


@pytest.mark.parametrize("order", tdref.ORDERS)
@pytest.mark.parametrize("k", (1, 50, 1000))
def test_merge_top_of_a_split_equals_top_of_the_whole(order, k):
    table = tied_table()
    shards = [{}, {}, {}]
    for i, v in table.items():
        shards[i % 3][i] = v
    lists = [[TraceIdDuration(*r) for r in tdref.top(s, order, k)] for s in shards]
    got = merge_top(lists, k, order)
    assert [tuple(t) for t in got] == tdref.top(table, order, k)


def test_merge_top_refuses_an_unknown_order():
    with pytest.raises(ValueError):
        merge_top([[]], 3, "duration")
