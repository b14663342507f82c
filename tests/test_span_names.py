"""Span names as a key of the realtime link store, on CPU: the host decoder's span-name dictionary
(ZK_INGEST_SPAN_NAMES, include/zkingest.h) and the name-id half of the record's flags (include/zkagg.h
ZK_F_NAME_SHIFT), the rpcName rules of the GpuRealtimeAggregates twin over a CPU window, the new ABI
calls' argument checks, and the join-with-names helper (tests/rpc_rows.py) against the oracle."""
import ctypes as C

import numpy as np
import pytest

from oracle.spans import Annotation, Endpoint, Span
from tests import rpc_rows, thriftenc
from tests.bulkfrag import service_name
from zipkin_amd import SpanColumns, ZkError, _abi, tracegen_host
from zipkin_amd.aggregates import Dictionary, GpuRealtimeAggregates
from zipkin_amd.ingest import SpanDecoder

WEB, APP = Endpoint(1, 80, "web"), Endpoint(2, 81, "app")


def _span(i, name, parent=None):
    anns = (Annotation(100 + i, "sr", APP), Annotation(200 + i, "ss", APP)) if i % 2 else \
        (Annotation(90 + i, "cs", WEB), Annotation(210 + i, "cr", WEB))
    return Span(1000 + i // 6, name, 50 + i // 2, parent, anns)


# the names, in input order: "" and "Unknown" are no names; "get" and "put" repeat across fragments
NAMES = ["get", "", "put", "get", "Unknown", "post", "put", "unknown", "get", "", "delete", "post"]
FIRST_SEEN = ["get", "put", "post", "unknown", "delete"]


def _blobs(names):
    return [thriftenc.snappy(thriftenc.span(_span(i, nm, parent=7 if i % 3 else None))) for i, nm in enumerate(names)]


def test_host_decoder_writes_span_name_ids():
    blobs = _blobs(NAMES)
    dec = SpanDecoder()
    cols, rej = dec.decode(blobs, span_names=True)
    assert rej == 0 and len(cols) == len(NAMES)
    assert dec.span_names() == FIRST_SEEN  # ids in order of first appearance, names byte for byte
    want = [0 if nm in ("", "Unknown") else FIRST_SEEN.index(nm) + 1 for nm in NAMES]
    assert cols.name_ids().tolist() == want
    assert (cols.flags >> np.uint32(16)).tolist() == want
    # without the flag: zero high halves, and every column equal once the high half is masked
    plain, _ = SpanDecoder().decode(blobs)
    assert not (plain.flags >> np.uint32(16)).any()
    masked = cols.without_names()
    for k in ("trace_id", "span_id", "parent_id", "first_ts", "last_ts", "service_id", "flags"):
        assert np.array_equal(getattr(masked, k), getattr(plain, k)), k
    # a decoder used without the flag keeps no names
    d2 = SpanDecoder()
    d2.decode(blobs)
    assert d2.num_span_names == 0
    # the dictionary carries over to the next batch; the accessors mirror the service ones
    more, _ = dec.decode(_blobs(["head", "put"]), span_names=True)
    assert more.name_ids().tolist() == [6, 2] and dec.num_span_names == 6
    assert dec.span_name_id("post") == 2 and dec.span_name_id("brand-new") == 6 and dec.span_name(6) == "brand-new"
    with pytest.raises(ZkError) as e:
        dec.span_name(7)
    assert e.value.status == _abi.ZK_ERR_INVALID_ARG


def test_span_name_ids_do_not_depend_on_the_thread_count():
    # enough fragments for the decoder to split the batch over its threads (>= 2048 per thread)
    rng = np.random.default_rng(3)
    pool = ["rpc-%d" % k for k in range(40)] + ["", "Unknown"]
    names = [pool[k] for k in rng.integers(0, len(pool), 9000)]
    blobs = _blobs(names)
    a, b = SpanDecoder(), SpanDecoder()
    many, _ = a.decode(blobs, span_names=True)
    one, _ = b.decode(blobs, span_names=True, one_thread=True)
    assert a.span_names() == b.span_names()
    seen = list(dict.fromkeys(n for n in names if n not in ("", "Unknown")))
    assert a.span_names() == seen
    for k in ("trace_id", "span_id", "parent_id", "first_ts", "last_ts", "service_id", "flags"):
        assert np.array_equal(getattr(many, k), getattr(one, k)), k
    assert many.name_ids().tolist() == [0 if n in ("", "Unknown") else seen.index(n) + 1 for n in names]


def test_span_name_dictionary_is_full_at_65535_names():
    dec = SpanDecoder()
    for k in range(65535):
        assert dec.span_name_id("n%d" % k) == k
    assert dec.num_span_names == 65535
    cols, _ = dec.decode(_blobs(["n65534", "n0"]), span_names=True)
    assert cols.name_ids().tolist() == [65535, 1]
    with pytest.raises(ZkError) as e:
        dec.decode(_blobs(["n1", "one-too-many"]), span_names=True)
    assert e.value.status == _abi.ZK_ERR_CAPACITY
    with pytest.raises(ZkError) as e:
        dec.span_name_id("another")
    assert e.value.status == _abi.ZK_ERR_CAPACITY


def test_name_id_half_of_flags():
    cols = tracegen_host(11, 50, max_depth=4, num_services=5)
    low = cols.flags.copy()
    assert not cols.name_ids().any()  # every batch that exists today has zeros there
    ids = np.arange(len(cols)) % 65536
    ids[:3] = (0, 1, 65535)
    cols.set_name_ids(ids)
    assert np.array_equal(cols.name_ids(), ids.astype(np.uint32))
    assert np.array_equal(cols.flags & np.uint32(0xFFFF), low)
    assert np.array_equal(cols.without_names().flags, low) and cols.name_ids().any()
    with pytest.raises(ValueError):
        cols.set_name_ids(np.full(len(cols), 65536))
    with pytest.raises(ValueError):
        cols.set_name_ids(ids[:-1])


def test_new_calls_reject_null_handles():
    L = _abi.lib()
    n, n32, n64 = C.c_uint64(), C.c_uint32(), C.c_uint64()
    assert L.zk_rl_server_rpc_links(None, 0, 0, None, None, None, None, 0, C.byref(n)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_rl_server_rpc_links(None, 0, _abi.ZK_RL_ANY_RPC, None, None, None, None, 0, C.byref(n)) == \
        _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_num_span_names(None, C.byref(n32)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_span_name_id(None, b"x", 1, C.byref(n32)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_span_name(None, 0, None, 0, C.byref(n64)) == _abi.ZK_ERR_INVALID_ARG
    dec = SpanDecoder()
    assert L.zk_ingest_num_span_names(dec._h, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_span_name_id(dec._h, b"x", 1, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_span_name_id(dec._h, None, 1, C.byref(n32)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_ingest_span_name(dec._h, 0, None, 0, None) == _abi.ZK_ERR_INVALID_ARG


# ---- the trait twin over a CPU window ------------------------------------------------------------
class HelperWindow:
    """A GpuRealtimeAggregates window answering from tests/rpc_rows.py (the device's is
    _DeviceLinkWindow): server_links(server) and the rpc-filtered call."""

    calls = []

    def __init__(self, S):
        self.S = S
        self.parts = []

    def add(self, cols, clustered):
        self.parts.append(cols)
        self._cache = None

    def _rows(self):
        if self._cache is None:  # (computed once per window content)
            self._cache = rpc_rows.rpc_rows(SpanColumns.concat(self.parts), self.S)
        return self._cache

    @staticmethod
    def _arrays(sel):
        return (np.array(sel[0], np.uint32), np.array(sel[1], np.int64), np.array(sel[2], np.uint64))

    def server_links(self, server):
        HelperWindow.calls.append(("server_links", server))
        return self._arrays(rpc_rows.server_rows(self._rows(), server))

    def server_rpc_links(self, server, rpc):
        HelperWindow.calls.append(("server_rpc_links", server, rpc))
        return self._arrays(rpc_rows.server_rows(self._rows(), server, rpc))

    def close(self):
        pass


def _answers(rows, names, server, rpc):
    durs, tids = {}, {}
    for p, c, d, t, n in rows:
        if c != server or (rpc is not None and n != rpc):
            continue
        durs.setdefault(names.name(p), []).append(d)
        tids.setdefault(names.name(p), set()).add(t - (1 << 64) if t >= 1 << 63 else t)
    return {k: sorted(v) for k, v in durs.items()}, {k: sorted(v) for k, v in tids.items()}


def test_twin_answers_by_rpc_name():
    S = 11
    names = Dictionary([service_name(i) for i in range(S)])
    rpcs = Dictionary(["rpc-%d" % k for k in range(rpc_rows.R)])
    cols = rpc_rows.assign_names(tracegen_host(21, 800, max_depth=6, num_services=S), 21)
    rows = rpc_rows.rpc_rows(cols, S)
    rpc_rows.assert_tied_to_oracle(rows, cols, S)
    assert {r[4] for r in rows} == set(range(rpc_rows.R + 1))  # every id, and spans without a name
    hour = 3_600_000_000
    store = GpuRealtimeAggregates(names, window_factory=HelperWindow, rpcs=rpcs)
    plain = GpuRealtimeAggregates(names, window_factory=HelperWindow)
    store.accumulate(cols, hour)
    plain.accumulate(cols, hour)
    for server in range(S):
        sname = names.name(server)
        every = _answers(rows, names, server, None)
        # "": every rpc, through server_links(server) exactly as without a dictionary
        HelperWindow.calls.clear()
        assert store.getSpanDurations(hour, sname, "") == every[0]
        assert store.getServiceNamesToTraceIds(hour, sname, "") == every[1]
        assert HelperWindow.calls == [("server_links", server)] * 2
        assert plain.getSpanDurations(hour, sname, "") == every[0]
        assert plain.getSpanDurations(hour, sname, "rpc-1") == every[0]  # no dictionary: not a key
        # "Unknown": the rows without a name
        none = _answers(rows, names, server, 0)
        assert store.getSpanDurations(hour, sname, "Unknown") == none[0]
        assert store.getServiceNamesToTraceIds(hour, sname, "Unknown") == none[1]
        total = sum(len(v) for v in none[0].values())
        for k in range(rpc_rows.R):
            HelperWindow.calls.clear()
            want = _answers(rows, names, server, k + 1)
            assert store.getSpanDurations(hour, sname, rpcs.name(k)) == want[0]
            assert store.getServiceNamesToTraceIds(hour, sname, rpcs.name(k)) == want[1]
            assert HelperWindow.calls == [("server_rpc_links", server, k + 1)] * 2
            total += sum(len(v) for v in want[0].values())
        assert total == sum(len(v) for v in every[0].values())
        # a name the dictionary does not hold: empty, and the dictionary stays as it was
        assert store.getSpanDurations(hour, sname, "no-such-rpc") == {}
        assert store.getServiceNamesToTraceIds(hour, sname, "no-such-rpc") == {}
    assert len(rpcs) == rpc_rows.R
    assert any(_answers(rows, names, s, 0)[0] for s in range(S))
    # the service count is fixed when the store is constructed: a later name answers {} (no raise)
    late = names.id("added-later")
    assert late == S and store.getSpanDurations(hour, "added-later", "") == {}
    assert store.getServiceNamesToTraceIds(hour, "added-later", "rpc-0") == {}
    store.close()
    plain.close()


def test_helper_rows_equal_the_oracle_and_take_the_largest_name():
    from tests.test_gpu_parity import CLIENT, SERVER, cols_from_rows

    S = 5
    cols = tracegen_host(22, 300, max_depth=5, num_services=S)
    rows = rpc_rows.rpc_rows(cols, S)
    rpc_rows.assert_tied_to_oracle(rows, cols, S)
    assert rows and {r[4] for r in rows} == {0}
    rpc_rows.assign_names(cols, 22)
    rpc_rows.assert_tied_to_oracle(rpc_rows.rpc_rows(cols, S), cols, S)
    # one trace by hand: the merged span's id is the maximum over its fragments
    T, ROOT = 77, 1
    hand = cols_from_rows([
        (T, ROOT, 0, 100, 900, 0, SERVER | (9 << 16)),     # the root's own name is not the link's
        (T, 2, ROOT, 110, 120, 1, CLIENT | 1 | (3 << 16)),  # span 2: ids 3 and 5 -> 5
        (T, 2, ROOT, 112, 118, 1, SERVER | 1 | (5 << 16)),
        (T, 3, ROOT, 210, 230, 2, CLIENT | 1),              # span 3: only one fragment is named -> 2
        (T, 3, ROOT, 212, 228, 2, SERVER | 1 | (2 << 16)),
        (T, 4, ROOT, 310, 340, 3, CLIENT | 1),              # span 4: no name -> 0
        (T, 4, ROOT, 312, 338, 3, SERVER | 1),
    ])
    rows = rpc_rows.rpc_rows(hand, S)
    rpc_rows.assert_tied_to_oracle(rows, hand, S)
    assert rows == [(0, 1, 10, T, 5), (0, 2, 20, T, 2), (0, 3, 30, T, 0)]
    assert rpc_rows.server_rows(rows, 2, 2) == [[0], [20], [T], [2]] and rpc_rows.server_rows(rows, 2, 5) == [[], [], [], []]
