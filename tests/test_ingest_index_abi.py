"""The indexed calls of the device decoder without a device (include/zkingest.h,
zk_ingest_dev_spans_indexed / zk_ingest_dev_spans_multi_indexed): the symbols are bound, and a NULL
handle, a NULL ix or any NULL column of ix is ZK_ERR_INVALID_ARG before any device is touched."""
import ctypes as C

import pytest

from zipkin_amd import AnnotationItems, _abi

COLUMNS = ("service", "key", "val", "ts", "trace_id")
FAKE = C.c_void_p(0x1000)  # stands for a decoder handle: the argument check comes before any use of it


def test_symbols_are_bound():
    L = _abi.lib()
    names = list(_abi.SYMBOLS)
    for sym in ("zk_ingest_dev_spans_indexed", "zk_ingest_dev_spans_multi_indexed", "zk_ingest_dev_index_stats"):
        assert sym in names
        assert getattr(L, sym) is not None
    assert int(L.zk_abi_version()) == 3


def calls(L, handle, ix):
    n, r = C.c_uint64(), C.c_uint64()
    yield L.zk_ingest_dev_spans_indexed(handle, None, None, 0, 0, 0, None, C.byref(n), C.byref(r), None, ix)
    yield L.zk_ingest_dev_spans_multi_indexed(handle, 0, None, None, None, 0, 0, None, C.byref(n), C.byref(r), None, ix)


def test_null_handle_and_null_ix():
    L = _abi.lib()
    ok = AnnotationItems.empty(4)
    ab = ok.abi(cap=4, n=0)
    for st in calls(L, None, C.byref(ab)):
        assert st == _abi.ZK_ERR_INVALID_ARG
    for st in calls(L, FAKE, None):
        assert st == _abi.ZK_ERR_INVALID_ARG


@pytest.mark.parametrize("missing", COLUMNS)
def test_any_null_column(missing):
    L = _abi.lib()
    ok = AnnotationItems.empty(4)
    ab = ok.abi(cap=4, n=0)
    setattr(ab, missing, None)
    for st in calls(L, FAKE, C.byref(ab)):
        assert st == _abi.ZK_ERR_INVALID_ARG


def test_index_stats_refuses_nulls():
    L = _abi.lib()
    ms, sl = C.c_double(), C.c_uint64()
    assert L.zk_ingest_dev_index_stats(None, C.byref(ms), C.byref(sl)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_dev_index_stats(FAKE, None, C.byref(sl)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_dev_index_stats(FAKE, C.byref(ms), None) == _abi.ZK_ERR_INVALID_ARG
