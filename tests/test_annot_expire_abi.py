"""The annotation store's expiry in the C ABI (include/zkannots.h): NULL arguments, too many pins and a
duplicated pin are refused, a store that never opened a device answers without one, and the header's constants
are the binding's. No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from zipkin_amd import TraceAnnotationStore, ZkError, _abi

HEADER = (Path(__file__).resolve().parent.parent / "include" / "zkannots.h").read_text()
BAD = _abi.ZK_ERR_INVALID_ARG
MIN, MAX = -(2 ** 63), 2 ** 63 - 1


def raw_expire(store, min_end, ids, cuts, null_ids=False, null_cuts=False, n=None):
    ids, cuts, removed = np.array(ids, np.uint64), np.array(cuts, np.int64), C.c_uint64(77)
    st = store._L.zk_an_expire(store._h, min_end, None if null_ids else ids.ctypes.data, None if null_cuts else cuts.ctypes.data,
                               len(ids) if n is None else n, C.byref(removed))
    return st, int(removed.value)


def test_the_new_entry_points_refuse_null():
    L = _abi.lib()
    removed = C.c_uint64(77)
    assert L.zk_an_expire(None, 0, None, None, 0, C.byref(removed)) == BAD
    assert L.zk_an_expire(None, 0, None, None, 0, None) == BAD
    assert removed.value == 77
    out = (C.c_double * 3)()
    assert L.zk_an_expire_ms(None, out) == BAD
    assert L.zk_an_expire_ms(None, None) == BAD
    with TraceAnnotationStore() as store:
        assert L.zk_an_expire(store._h, 0, None, None, 0, None) == BAD          # NULL removed
        assert L.zk_an_expire_ms(store._h, None) == BAD
        one = np.array([5], np.uint64), np.array([0], np.int64)
        assert raw_expire(store, 0, *one, null_ids=True) == (BAD, 0)             # n_pins > 0 with a NULL array
        assert raw_expire(store, 0, *one, null_cuts=True) == (BAD, 0)
        assert raw_expire(store, 0, [], [], null_ids=True, null_cuts=True) == (_abi.ZK_OK, 0)  # n_pins == 0 allows NULL


def test_too_many_pins_and_a_duplicated_pin_are_refused():
    with TraceAnnotationStore() as store:
        n = _abi.ZK_AN_MAX_PINS + 1
        assert raw_expire(store, 0, np.arange(n), np.zeros(n)) == (BAD, 0)
        assert "ZK_AN_MAX_PINS" in store._L.zk_an_last_error(store._h).decode()
        assert raw_expire(store, 0, np.arange(n - 1), np.zeros(n - 1)) == (_abi.ZK_OK, 0)  # the bound itself is allowed
        assert raw_expire(store, 0, [7, 9, 7], [1, 2, 3]) == (BAD, 0)
        assert raw_expire(store, 0, [0, 2 ** 64 - 1, 0], [1, 2, 3]) == (BAD, 0)
        with pytest.raises(ValueError):
            store.expire(0, {i: 0 for i in range(n)})
        assert store.info() == {"entries": 0, "segments": 0, "bytes": 0}


@pytest.mark.parametrize("min_end", [MIN, MIN + 1, -1, 0, 12345, MAX])
def test_a_never_opened_store_answers_without_a_device(min_end):
    with TraceAnnotationStore() as store:
        assert store.expire(min_end) == 0
        assert store.expire(min_end, {}) == 0
        assert store.expire(min_end, {0: MIN, 2 ** 64 - 1: MAX, 5: 7}) == 0
        assert store.info() == {"entries": 0, "segments": 0, "bytes": 0}
        assert store.getAnnotationsByTraceIds([0, 5]) == [[], []]


def test_expire_ms_is_an_error_without_timing_and_before_a_pass():
    for timing in (False, True):
        with TraceAnnotationStore(timing=timing) as store:
            with pytest.raises(ZkError) as e:
                store.expire_ms()
            assert e.value.status == BAD
            assert store.expire(5, {1: 2}) == 0  # an empty store: no pass ran
            with pytest.raises(ZkError) as e:
                store.expire_ms()
            assert e.value.status == BAD and "zk_an_config.timing" in e.value.message


def test_constants_match_the_header():
    m = re.search(r"#define\s+ZK_AN_MAX_PINS\s+(\d+)u", HEADER)
    assert m and int(m.group(1)) == _abi.ZK_AN_MAX_PINS == _abi.ZK_SP_MAX_PINS == 4096
    assert C.sizeof(_abi.zk_an_config) == 48
    assert _abi.zk_an_config.expire_chunk.offset == 16 and _abi.zk_an_config.expire_chunk.size == 4
    assert _abi.zk_an_config.reserved.offset == 20 and _abi.zk_an_config.reserved.size == 28
    assert _abi.zk_an_config.expire_chunk.offset == _abi.zk_sp_config.expire_chunk.offset
    assert re.search(r"uint32_t\s+expire_chunk;", HEADER) and re.search(r"uint32_t\s+reserved\[7\];", HEADER)
    for word in ("A trace goes or stays WHOLE", "end == cutoff stays", "INVARIANT", "zk_an_expire_ms",
                 "zk_mix64(trace_id ^ ZK_SP_END_SALT) & (slots - 1)", "the segment count never grows"):
        assert word in HEADER, word
    assert "No expiry yet" not in HEADER
    assert TraceAnnotationStore.EXPIRE_PHASES == ("ends", "size", "rewrite")
