"""The span store's C ABI (include/zkspans.h): NULL arguments and an oversized ask are refused before any
device is touched, and the header's constants are the binding's. No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import spref as R
from tests.conftest import gpu_available
from zipkin_amd import SpanColumns, _abi

HEADER = (Path(__file__).resolve().parent.parent / "include" / "zkspans.h").read_text()
BAD = _abi.ZK_ERR_INVALID_ARG


def test_every_entry_point_refuses_null():
    L = _abi.lib()
    h, cfg = C.c_void_p(), _abi.zk_sp_config()
    assert L.zk_sp_create(None, C.byref(h)) == BAD
    assert L.zk_sp_create(C.byref(cfg), None) == BAD
    assert L.zk_sp_destroy(None) == BAD
    assert L.zk_sp_last_error(None) == b"null handle"
    ab = SpanColumns.empty(1).abi()
    assert L.zk_sp_observe(None, C.byref(ab), 0) == BAD
    assert L.zk_sp_reset(None) == BAD
    assert L.zk_sp_compact(None) == BAD
    a = C.c_uint64()
    assert L.zk_sp_info(None, C.byref(a), C.byref(a), C.byref(a)) == BAD
    ids = np.zeros(4, np.uint64)
    found = np.zeros(4, np.uint8)
    counts = np.zeros(4, np.uint32)
    assert L.zk_sp_exist(None, ids.ctypes.data, 4, 0, found.ctypes.data_as(C.POINTER(C.c_uint8))) == BAD
    assert L.zk_sp_gather(None, ids.ctypes.data, 4, 0, counts.ctypes.data_as(_abi._U32P), None, 0, C.byref(a)) == BAD
    out = (C.c_double * 3)()
    assert L.zk_sp_observe_ms(None, out) == BAD
    assert L.zk_sp_query_ms(None, C.cast(out, C.POINTER(C.c_double))) == BAD


def test_an_ask_above_the_limit_is_refused():
    """No handle can be made without a device, so here the refusal is the NULL handle's; with a live
    handle tests/test_gpu_span_store.py checks the same ask's status and message."""
    L = _abi.lib()
    n = _abi.ZK_SP_MAX_IDS + 1
    ids, found, counts, total = np.zeros(n, np.uint64), np.zeros(n, np.uint8), np.zeros(n, np.uint32), C.c_uint64()
    assert L.zk_sp_exist(None, ids.ctypes.data, n, 0, found.ctypes.data_as(C.POINTER(C.c_uint8))) == BAD
    assert L.zk_sp_gather(None, ids.ctypes.data, n, 0, counts.ctypes.data_as(_abi._U32P), None, 0, C.byref(total)) == BAD
    assert not found.any() and not counts.any()


@pytest.mark.skipif(gpu_available(), reason="checks the no-device path")
def test_create_without_a_device_fails_loudly():
    from zipkin_amd import TraceSpanStore, ZkError

    with pytest.raises(ZkError) as e:
        TraceSpanStore()
    assert e.value.status == _abi.ZK_ERR_NO_DEVICE


def test_constants_match_the_header():
    m = re.search(r"#define\s+ZK_SP_SALT\s+0x([0-9A-Fa-f]+)ull", HEADER)
    assert m and int(m.group(1), 16) == _abi.ZK_SP_SALT == R.SALT
    for name in ("ZK_SP_BUCKETS", "ZK_SP_MAX_SEGMENTS", "ZK_SP_MAX_IDS"):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)u", HEADER)
        assert m and int(m.group(1)) == getattr(_abi, name), name
    assert (_abi.ZK_SP_BUCKETS, _abi.ZK_SP_MAX_SEGMENTS, _abi.ZK_SP_MAX_IDS) == (4096, 64, 4096)
    assert len({_abi.ZK_SP_SALT, _abi.ZK_TD_TABLE_SALT, _abi.ZK_WIN_TABLE_SALT}) == 3
    assert C.sizeof(_abi.zk_sp_config) == 48 and C.sizeof(_abi.zk_sp_rows) == 56
    for word in ("MEMBERSHIP", "CANONICAL ORDER", "WIDER than zkduration.h", "zk_mix64(trace_id ^ ZK_SP_SALT) >> 52",
                 "no endpoints"):
        assert word in HEADER, word
