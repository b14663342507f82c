"""The span store's expiry in the C ABI (include/zkspans.h): NULL arguments and too many pins are refused
before any device is touched, and the header's constants are the binding's. No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

from zipkin_amd import _abi

HEADER = (Path(__file__).resolve().parent.parent / "include" / "zkspans.h").read_text()
BAD = _abi.ZK_ERR_INVALID_ARG


def test_the_new_entry_points_refuse_null():
    L = _abi.lib()
    removed = C.c_uint64(77)
    assert L.zk_sp_expire(None, 0, None, None, 0, C.byref(removed)) == BAD
    assert L.zk_sp_expire(None, 0, None, None, 0, None) == BAD
    assert removed.value == 77
    out = (C.c_double * 3)()
    assert L.zk_sp_expire_ms(None, out) == BAD
    assert L.zk_sp_expire_ms(None, None) == BAD


def test_too_many_pins_are_refused():
    """No handle can be made without a device, so here the refusal is the NULL handle's; with a live
    handle tests/test_gpu_span_expire.py checks the same call's status."""
    L = _abi.lib()
    n = _abi.ZK_SP_MAX_PINS + 1
    ids, cuts, removed = np.arange(n, dtype=np.uint64), np.zeros(n, np.int64), C.c_uint64(77)
    assert L.zk_sp_expire(None, 0, ids.ctypes.data, cuts.ctypes.data, n, C.byref(removed)) == BAD
    assert removed.value == 77


def test_constants_match_the_header():
    m = re.search(r"#define\s+ZK_SP_MAX_PINS\s+(\d+)u", HEADER)
    assert m and int(m.group(1)) == _abi.ZK_SP_MAX_PINS == 4096
    m = re.search(r"#define\s+ZK_SP_END_SALT\s+0x([0-9A-Fa-f]+)ull", HEADER)
    assert m and int(m.group(1), 16) == _abi.ZK_SP_END_SALT
    # the salts differ: the four hash apart
    assert len({_abi.ZK_SP_END_SALT, _abi.ZK_SP_SALT, _abi.ZK_TD_TABLE_SALT, _abi.ZK_WIN_TABLE_SALT}) == 4
    assert C.sizeof(_abi.zk_sp_config) == 48
    assert _abi.zk_sp_config.expire_chunk.offset == 16 and _abi.zk_sp_config.expire_chunk.size == 4
    assert re.search(r"uint32_t\s+expire_chunk;", HEADER) and re.search(r"uint32_t\s+reserved\[7\];", HEADER)
    for word in ("A trace goes or stays WHOLE", "end == cutoff stays", "INVARIANT", "zk_mix64(trace_id ^ ZK_SP_END_SALT) & (slots - 1)"):
        assert word in HEADER, word
    assert "Nothing expires" not in HEADER
