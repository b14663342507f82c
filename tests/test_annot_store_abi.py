"""The annotation store's C ABI (include/zkannots.h): NULL arguments and an oversized ask are refused before any
device is touched, the header's constants and layouts are the binding's, and an empty store answers without a
device: zk_an_create opens none. No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import anref as R
from tests.conftest import gpu_available
from zipkin_amd import AnnotationRows, TraceAnnotationStore, ZkError, _abi
from zipkin_amd.annotstore import ROW_COLUMNS, annotation_key, row_bits

HEADER = (Path(__file__).resolve().parent.parent / "include" / "zkannots.h").read_text()
BAD = _abi.ZK_ERR_INVALID_ARG
SENTINEL = 0xA5


def test_every_entry_point_refuses_null():
    L = _abi.lib()
    h, cfg = C.c_void_p(), _abi.zk_an_config()
    assert L.zk_an_create(None, C.byref(h)) == BAD
    assert L.zk_an_create(C.byref(cfg), None) == BAD
    assert L.zk_an_destroy(None) == BAD
    assert L.zk_an_last_error(None) == b"null handle"
    ab = AnnotationRows.empty(1).abi()
    assert L.zk_an_observe(None, C.byref(ab), 1, 0) == BAD
    assert L.zk_an_reset(None) == BAD
    assert L.zk_an_compact(None) == BAD
    a = C.c_uint64()
    assert L.zk_an_info(None, C.byref(a), C.byref(a), C.byref(a)) == BAD
    ids, counts = np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    assert L.zk_an_gather(None, ids.ctypes.data, 4, 0, counts.ctypes.data_as(_abi._U32P), None, 0, C.byref(a)) == BAD
    out = (C.c_double * 3)()
    assert L.zk_an_observe_ms(None, out) == BAD
    assert L.zk_an_query_ms(None, C.cast(out, C.POINTER(C.c_double))) == BAD


def test_a_live_handle_refuses_null_arguments_and_bad_asks():
    L = _abi.lib()
    with TraceAnnotationStore() as store:  # (no device is opened: nothing below reaches one)
        h = store._h
        total, ids, counts = C.c_uint64(7), np.zeros(_abi.ZK_AN_MAX_IDS + 1, np.uint64), np.full(_abi.ZK_AN_MAX_IDS + 1, 9, np.uint32)
        cp = counts.ctypes.data_as(_abi._U32P)
        assert L.zk_an_observe(h, None, 1, 0) == BAD and L.zk_an_last_error(h) == b"null argument"
        rows = AnnotationRows.empty(2)
        for k, _ in ROW_COLUMNS:
            ab = rows.abi()
            setattr(ab, k, None)
            assert L.zk_an_observe(h, C.byref(ab), 2, 0) == BAD and L.zk_an_last_error(h) == b"null column"
        ab = rows.abi()
        assert L.zk_an_observe(h, C.byref(ab), 2, 2) == BAD  # ZK_BATCH_TRACE_CLUSTERED is no flag of this call
        assert L.zk_an_observe(h, C.byref(ab), 2 ** 32, 0) == _abi.ZK_ERR_UNSUPPORTED
        assert L.zk_an_gather(h, ids.ctypes.data, 4, 0, cp, None, 0, None) == BAD
        assert L.zk_an_gather(h, None, 4, 0, cp, None, 0, C.byref(total)) == BAD
        assert L.zk_an_gather(h, ids.ctypes.data, 4, 0, None, None, 0, C.byref(total)) == BAD
        assert L.zk_an_gather(h, ids.ctypes.data, 4, 2, cp, None, 0, C.byref(total)) == BAD
        assert L.zk_an_gather(h, ids.ctypes.data, 4, 0, cp, None, 1, C.byref(total)) == BAD  # cap without columns
        ab = rows.abi()
        ab.bits = None
        assert L.zk_an_gather(h, ids.ctypes.data, 4, 0, cp, C.byref(ab), 2, C.byref(total)) == BAD
        assert L.zk_an_gather(h, ids.ctypes.data, len(ids), 0, cp, None, 0, C.byref(total)) == BAD
        assert b"ZK_AN_MAX_IDS" in L.zk_an_last_error(h)
        assert total.value == 7 and (counts == 9).all()  # a refused ask writes nothing
        assert L.zk_an_observe_ms(h, None) == BAD and L.zk_an_query_ms(h, None) == BAD
        with pytest.raises(ZkError):
            store.observe_ms()
        with pytest.raises(ZkError):
            store.query_ms()
        with pytest.raises(ZkError) as e:
            store.gather(ids)
        assert e.value.status == BAD


def test_an_empty_store_answers_without_a_device():
    L = _abi.lib()
    with TraceAnnotationStore() as store:
        assert store.info() == {"entries": 0, "segments": 0, "bytes": 0}
        store.observe(AnnotationRows.empty(0))  # n == 0 is ZK_OK
        ab = _abi.zk_an_cols()
        assert L.zk_an_observe(store._h, C.byref(ab), 0, 0) == _abi.ZK_OK  # ... whatever the columns are
        store.reset()
        store.compact()
        assert store.info() == {"entries": 0, "segments": 0, "bytes": 0}
        assert L.zk_an_info(store._h, None, None, None) == _abi.ZK_OK
        # the sizing call, and a call with sentinel-filled columns: counts of zeros, no row written
        ids = np.array([0, 5, 2 ** 64 - 1], np.uint64)
        counts, total = np.full(3, 0xDEADBEEF, np.uint32), C.c_uint64(12345)
        assert L.zk_an_gather(store._h, ids.ctypes.data, 3, 0, counts.ctypes.data_as(_abi._U32P), None, 0, C.byref(total)) == _abi.ZK_OK
        assert total.value == 0 and counts.tolist() == [0, 0, 0]
        cols = [np.frombuffer(bytes([SENTINEL]) * (4 * np.dtype(dt).itemsize), dt).copy() for _, dt in ROW_COLUMNS]
        out = _abi.zk_an_cols(*[c.ctypes.data for c in cols])
        counts[:] = 7
        assert L.zk_an_gather(store._h, ids.ctypes.data, 3, 0, counts.ctypes.data_as(_abi._U32P), C.byref(out), 4, C.byref(total)) == _abi.ZK_OK
        assert total.value == 0 and counts.tolist() == [0, 0, 0] and all((c.view(np.uint8) == SENTINEL).all() for c in cols)
        total.value = 5
        assert L.zk_an_gather(store._h, None, 0, 0, None, None, 0, C.byref(total)) == _abi.ZK_OK and total.value == 0
        got, rows = store.gather([1, 2])
        assert got.tolist() == [0, 0] and len(rows) == 0
        assert store.getAnnotationsByTraceIds(list(range(5000))) == [[]] * 5000  # (the Python call asks in parts)
        assert store.getAnnotationsByTraceIds([]) == []
    store.close()  # twice is fine


@pytest.mark.skipif(gpu_available(), reason="checks the no-device path")
def test_the_first_rows_need_a_device():
    with TraceAnnotationStore() as store:
        with pytest.raises(ZkError) as e:
            store.observe(AnnotationRows.of_rows([(1, 2, 3, 4, 5, 6, 7)]))
        assert e.value.status == _abi.ZK_ERR_NO_DEVICE
        assert store.info() == {"entries": 0, "segments": 0, "bytes": 0}


def test_create_checks_its_config():
    L = _abi.lib()
    h, cfg = C.c_void_p(), _abi.zk_an_config()
    cfg.device = -1
    assert L.zk_an_create(C.byref(cfg), C.byref(h)) == BAD and not h.value


def test_constants_and_layouts_match_the_header():
    for name in ("ZK_AN_BUCKETS", "ZK_AN_MAX_SEGMENTS", "ZK_AN_MAX_IDS", "ZK_AN_ROW_BYTES", "ZK_AN_KIND_MASK", "ZK_AN_KIND_OTHER",
                 "ZK_AN_KIND_CS", "ZK_AN_KIND_CR", "ZK_AN_KIND_SR", "ZK_AN_KIND_SS", "ZK_AN_HAS_HOST", "ZK_AN_PORT_SHIFT"):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)u", HEADER)
        assert m and int(m.group(1)) == getattr(_abi, name), name
    assert (_abi.ZK_AN_BUCKETS, _abi.ZK_AN_MAX_SEGMENTS, _abi.ZK_AN_MAX_IDS) == (_abi.ZK_SP_BUCKETS, 64, 4096)
    assert C.sizeof(_abi.zk_an_config) == 48 and C.sizeof(_abi.zk_an_cols) == 56
    assert sum(np.dtype(dt).itemsize for _, dt in ROW_COLUMNS) == _abi.ZK_AN_ROW_BYTES == 44
    m = re.search(r"typedef struct zk_an_cols \{(.*?)\} zk_an_cols;", HEADER, re.S)
    assert re.findall(r"\*\s*(\w+);", m.group(1)) == [k for k, _ in ROW_COLUMNS] == list(R.COLS)
    assert [f[0] for f in _abi.zk_an_cols._fields_] == list(R.COLS)
    assert [f[0] for f in _abi.zk_ingest_annotation_rows._fields_][:7] == list(R.COLS)
    for word in ("CANONICAL ORDER", "MULTISET", "zk_mix64(trace_id ^ ZK_SP_SALT) >> 52", "touches no device"):
        assert word in HEADER, word


def test_the_canonical_key_is_the_models():
    cols = R.noise(np.zeros(300, np.uint64), seed=3)
    rows = AnnotationRows(*cols).rows()
    assert sorted(rows, key=annotation_key) == sorted(rows, key=R.key)
    assert row_bits(3, True, 0xFFFF) == 3 | 8 | (0xFFFF << 16) and row_bits(4, False) == 4
