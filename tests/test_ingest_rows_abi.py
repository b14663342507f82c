"""The annotated calls of the device decoder without a device (include/zkingest.h,
zk_ingest_dev_spans_annotated / zk_ingest_dev_spans_multi_annotated / zk_ingest_dev_rows_stats): the
symbols are bound, and a NULL handle, a NULL `an` or any NULL column of it is ZK_ERR_INVALID_ARG before
any device is touched. The one case that needs a live decoder (the statistics before the first annotated
call) is marked gpu."""
import ctypes as C

import pytest

from zipkin_amd import AnnotationRows, _abi
from zipkin_amd.annotstore import ROW_COLUMNS
from zipkin_amd.ingest import DeviceSpanDecoder

FAKE = C.c_void_p(0x1000)  # stands for a decoder handle: the argument check comes before any use of it


def test_symbols_are_bound():
    L = _abi.lib()
    names = list(_abi.SYMBOLS)
    for sym in ("zk_ingest_dev_spans_annotated", "zk_ingest_dev_spans_multi_annotated", "zk_ingest_dev_rows_stats"):
        assert sym in names
        assert getattr(L, sym) is not None
    assert _abi.ZK_INGEST_NO_ROW_STRINGS == 16
    # the flag is a bit of its own
    others = (_abi.ZK_INGEST_STRICT, _abi.ZK_INGEST_ONE_THREAD, _abi.ZK_INGEST_SPAN_NAMES, _abi.ZK_INGEST_NO_CLIENT_RULE)
    assert all(_abi.ZK_INGEST_NO_ROW_STRINGS & f == 0 for f in others)


def calls(L, handle, an):
    n, r = C.c_uint64(), C.c_uint64()
    yield L.zk_ingest_dev_spans_annotated(handle, None, None, 0, 0, 0, None, C.byref(n), C.byref(r), None, an)
    yield L.zk_ingest_dev_spans_multi_annotated(handle, 0, None, None, None, 0, 0, None, C.byref(n), C.byref(r), None, an)


def test_null_handle():
    L = _abi.lib()
    an = AnnotationRows.empty(4).ingest_abi(cap=4, n=0)
    for st in calls(L, None, C.byref(an)):
        assert st == _abi.ZK_ERR_INVALID_ARG


def test_null_an():
    L = _abi.lib()
    for st in calls(L, FAKE, None):
        assert st == _abi.ZK_ERR_INVALID_ARG


@pytest.mark.parametrize("missing", [k for k, _ in ROW_COLUMNS])
def test_any_null_column(missing):
    L = _abi.lib()
    rows = AnnotationRows.empty(4)
    an = rows.ingest_abi(cap=4, n=0)
    setattr(an, missing, None)
    for st in calls(L, FAKE, C.byref(an)):
        assert st == _abi.ZK_ERR_INVALID_ARG


def test_rows_stats_refuses_nulls():
    L = _abi.lib()
    ms, sl = C.c_double(), C.c_uint64()
    assert L.zk_ingest_dev_rows_stats(None, C.byref(ms), C.byref(sl)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_dev_rows_stats(FAKE, None, C.byref(sl)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_dev_rows_stats(FAKE, C.byref(ms), None) == _abi.ZK_ERR_INVALID_ARG


@pytest.mark.gpu
def test_rows_stats_before_any_annotated_call(gpu):
    dd = DeviceSpanDecoder(16)
    try:
        assert dd.rows_stats() == {"pass_ms": 0.0, "slices": 0}
    finally:
        dd.close()


@pytest.mark.parametrize("method", ("decode", "decode_device", "decode_device_many"))
def test_annotated_with_indexed_is_a_value_error_before_any_library_call(method):
    dd = DeviceSpanDecoder.__new__(DeviceSpanDecoder)  # no handle, no library: the check must come first
    args = {"decode": ([b""],), "decode_device": (None, None, 1), "decode_device_many": ([],)}[method]
    with pytest.raises(ValueError):
        getattr(dd, method)(*args, annotated=True, indexed=True)
