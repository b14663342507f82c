"""zk_sp_summaries' C ABI (include/zkspans.h): NULL arguments and an oversized ask are refused before any
device is touched, the head is 40 bytes, and the header's constants are the binding's. No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

from zipkin_amd import SUMMARY_HEAD, _abi

HEADER = (Path(__file__).resolve().parent.parent / "include" / "zkspans.h").read_text()
BAD = _abi.ZK_ERR_INVALID_ARG
SENTINEL = 0xA5


def buffers(n, cap):
    heads = np.frombuffer(bytes([SENTINEL]) * (n * 40), SUMMARY_HEAD).copy()
    cols = [np.full(cap, SENTINEL, np.uint32), np.full(cap, SENTINEL, np.int64), np.full(cap, SENTINEL, np.int64)]
    return heads, cols, _abi.zk_sp_span_ts(*[c.ctypes.data for c in cols])


def untouched(heads, cols):
    return (heads.view(np.uint8) == SENTINEL).all() and all((c == SENTINEL).all() for c in cols)


def test_summaries_refuses_null():
    """No handle can be made without a device: the NULL handle is refused whatever else is passed, NULL
    arguments among it; with a live handle tests/test_gpu_span_summary.py checks each NULL argument."""
    L = _abi.lib()
    ids, total = np.zeros(4, np.uint64), C.c_uint64(77)
    heads, cols, out = buffers(4, 8)
    assert L.zk_sp_summaries(None, ids.ctypes.data, 4, 0, heads.ctypes.data, C.byref(out), 8, C.byref(total)) == BAD
    assert L.zk_sp_summaries(None, None, 4, 0, heads.ctypes.data, C.byref(out), 8, C.byref(total)) == BAD
    assert L.zk_sp_summaries(None, ids.ctypes.data, 4, 0, None, C.byref(out), 8, C.byref(total)) == BAD
    assert L.zk_sp_summaries(None, ids.ctypes.data, 4, 0, heads.ctypes.data, None, 8, C.byref(total)) == BAD
    assert L.zk_sp_summaries(None, ids.ctypes.data, 4, 0, heads.ctypes.data, C.byref(out), 8, None) == BAD
    assert L.zk_sp_summaries(None, None, 0, 0, None, None, 0, None) == BAD
    assert untouched(heads, cols) and total.value == 77
    ms = C.c_double()
    assert L.zk_sp_query_ms(None, C.byref(ms)) == BAD


def test_an_ask_above_the_limit_is_refused():
    L = _abi.lib()
    n = _abi.ZK_SP_MAX_IDS + 1
    ids, total = np.zeros(n, np.uint64), C.c_uint64(77)
    heads, cols, out = buffers(n, 8)
    assert L.zk_sp_summaries(None, ids.ctypes.data, n, 0, heads.ctypes.data, C.byref(out), 8, C.byref(total)) == BAD
    assert untouched(heads, cols) and total.value == 77


def test_layouts_and_constants_match_the_header():
    assert C.sizeof(_abi.zk_sp_summary) == 40 == SUMMARY_HEAD.itemsize
    assert [(f[0], C.sizeof(f[1])) for f in _abi.zk_sp_summary._fields_] == \
        [(k, SUMMARY_HEAD[k].itemsize) for k in SUMMARY_HEAD.names]
    assert [getattr(_abi.zk_sp_summary, k).offset for k in SUMMARY_HEAD.names] == \
        [SUMMARY_HEAD.fields[k][1] for k in SUMMARY_HEAD.names] == [0, 8, 16, 24, 28, 32, 36]
    assert C.sizeof(_abi.zk_sp_span_ts) == 24
    assert C.sizeof(_abi.zk_sp_config) == 48
    for name in ("ZK_SP_SUM_MAX_ROWS", "ZK_SP_SUM_WAVE_ROWS", "ZK_SP_SUM_FOUND", "ZK_SP_SUM_TIMED", "ZK_SP_SUM_OVERFLOW"):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)u", HEADER)
        assert m and int(m.group(1)) == getattr(_abi, name), name
    assert _abi.ZK_SP_SUM_MAX_ROWS >= 2048
    bits = (_abi.ZK_SP_SUM_FOUND, _abi.ZK_SP_SUM_TIMED, _abi.ZK_SP_SUM_OVERFLOW)
    assert all(b and b & (b - 1) == 0 for b in bits) and len(set(bits)) == 3
    m = re.search(r"typedef struct zk_sp_summary \{(.*?)\} zk_sp_summary;", HEADER, re.S)
    assert m and re.findall(r"^\s*u?int\d+_t\s+(\w+);", m.group(1), re.M) == list(SUMMARY_HEAD.names)
    assert "zk_status   zk_sp_summaries(zk_sp* sp, const uint64_t* ids, uint32_t n, uint32_t flags, zk_sp_summary* heads," in HEADER
