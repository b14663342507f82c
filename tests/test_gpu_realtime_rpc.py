"""rpcName as a key of the realtime link store, on the GPU: the span-name id in bits 16..31 of the
record's flags (include/zkagg.h ZK_F_NAME_SHIFT) travels through K1, the spill kernel, the carry path
and the clustering passes into the store's window, the merged span takes the largest id of its
fragments, and zk_rl_server_rpc_links selects rows by (server, rpc) on the device. Every answer is
compared exactly with tests/rpc_rows.py (tied to oracle/realtime.py joined_links on each input), and
the dependency table must not notice the name bits at all."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle
from oracle.realtime import joined_links, server_links
from tests import rpc_rows
from tests.bulkfrag import service_name
from tests.exactref import DMAX
from tests.rpc_rows import R, assign_names, server_rows
from tests.test_gpu_exact_bounds import star_batch
from tests.test_gpu_parity import CLIENT, SERVER, assert_parity, cols_from_rows, star_trace
from zipkin_amd import DepsContext, DeviceColumns, SpanColumns, ZkError, _abi, tracegen_host
from zipkin_amd.realtime import RealtimeLinks

pytestmark = pytest.mark.gpu


def check_rows_by_rpc(rl, cols, S, rpcs=range(R + 1)):
    """every (server, rpc) and (server, any rpc) answer of the store against the helper's rows"""
    rows = rpc_rows.rpc_rows(cols, S)
    rpc_rows.assert_tied_to_oracle(rows, cols, S)
    plain = joined_links(cols.without_names(), S)
    assert rl.count() == (len(rows), 0)
    per_server = {s: [] for s in range(S)}
    for r in rows:
        per_server[r[1]].append(r)
    for s, rows_s in per_server.items():
        par, dur, tid, ids = rl.server_rpc_links(s)
        want = server_rows(rows_s, s)
        assert [par.tolist(), dur.tolist(), tid.tolist(), ids.tolist()] == want, f"server {s}, any rpc"
        total = 0
        for rpc in rpcs:
            got = rl.server_rpc_links(s, rpc)
            assert [g.tolist() for g in got] == server_rows(rows_s, s, rpc), f"server {s}, rpc {rpc}"
            total += len(got[0])
        assert total == len(par), f"server {s}: the per-rpc counts do not sum to the any-rpc count"
        # zk_rl_server_links is unchanged: the any-rpc rows without the rpc column
        for g, w, name in zip(rl.server_links(s), server_links(plain, s), ("parent", "duration", "traceId")):
            assert g.tolist() == w.tolist(), f"server {s}: server_links {name}"
    return rows


def assert_same_table(a, b):
    for k in ("m0", "m1", "m2", "m3", "m4", "present"):
        x, y = getattr(a, k), getattr(b, k)
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                              y.view(np.uint64) if y.dtype == np.float64 else y), k


@pytest.mark.parametrize("clustered", [True, False])
def test_rows_by_server_and_rpc(gpu, clustered):
    S = 13
    cols = assign_names(tracegen_host(81, 5000, max_depth=6, num_services=S), 81)
    if not clustered:
        cols = cols.take(np.random.default_rng(81).permutation(len(cols)))
    masked = cols.without_names()
    with DepsContext(S) as ctx, RealtimeLinks(S) as rl:
        rl.bind(ctx)
        ctx.accumulate(cols, clustered=clustered, verify=clustered)
        got = ctx.finalize()
        st = ctx.stats()
        rows = check_rows_by_rpc(rl, cols, S)
    assert {r[4] for r in rows} == set(range(R + 1))
    assert_parity(got, st, oracle.aggregate(masked, S))
    # the same batch with every name bit zero and no store bound: the same table, the same counters
    with DepsContext(S) as ctx:
        ctx.accumulate(masked, clustered=clustered, verify=clustered)
        assert_same_table(got, ctx.finalize())
        st0 = ctx.stats()
    assert {k: v for k, v in st.items() if k != "spilled_traces"} == {k: v for k, v in st0.items() if k != "spilled_traces"}


def test_names_through_spill_continuation_and_window_growth(gpu):
    """Names from the spill kernel (a 12k-record trace), from held traces joined across batch edges
    (cuts at 5 random points, host and device columns in turn), over a window that grows past its
    first allocation and must keep its name column."""
    S = 9
    rows = []
    for t in range(40):
        rows += star_trace(100 + t, 1 + t % 6, svc_root=t % S, nsvc=S)
    rows += star_trace(7777, 6_000, nsvc=S)  # 12k records: longer than a K1 window -> spill kernel
    for t in range(40):
        rows += star_trace(900 + t, 1 + t % 5, svc_root=t % S, nsvc=S)
    cols = SpanColumns.concat([cols_from_rows(rows), tracegen_host(82, 6000, max_depth=6, num_services=S)])
    assign_names(cols, 82)
    cuts = sorted(np.random.default_rng(82).choice(np.arange(1, len(cols)), 5, replace=False).tolist())
    bounds = [0, *cuts, len(cols)]
    with DepsContext(S) as ctx, RealtimeLinks(S) as rl:
        rl.bind(ctx)
        for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            part = cols.take(slice(a, b))
            ctx.accumulate(DeviceColumns.from_host(part) if i % 2 else part, clustered=True, verify=True,
                           continues=i + 2 < len(bounds))
        got = ctx.finalize()
        st = ctx.stats()
        assert st["spilled_traces"] >= 1
        got_rows = check_rows_by_rpc(rl, cols, S)
        # the giant trace's children disagree on their names like everyone else
        assert len({r[4] for r in got_rows if r[3] == 7777}) == R + 1
        rl.reset()
        assert rl.count() == (0, 0)
        assert len(rl.server_rpc_links(0, 1)[0]) == 0
    assert_parity(got, st, oracle.aggregate(cols.without_names(), S))


def test_name_merges_across_waves(gpu):
    """One trace inside one 512-record K1 window; the two fragments of a span lie 260 records apart
    (different waves of the workgroup) and only one of them carries a name -- whichever of the two
    claims the span's hash slot, the other merges its name into it."""
    S, T, ROOT = 7, 4242, 1
    first = [(T, ROOT, 0, 1000, 9000, 0, SERVER)]
    # (span, client fragment's name id, server fragment's name id, duration) -> expected merged id
    special = [(10, 0, 4, 11, 4), (11, 6, 0, 12, 6), (12, 0, 0, 13, 0), (13, 3, 5, 14, 5), (14, 5, 3, 15, 5)]
    head = [(T, sid, ROOT, 2000, 2000 + d, 1 + sid % 6, CLIENT | 1 | (a << 16)) for sid, a, b, d, _ in special]
    filler = [(T, 100 + i, ROOT, 3000 + i, 3100 + i, 1 + i % 6, SERVER | 1 | (1 << 16)) for i in range(255)]
    tail = [(T, sid, ROOT, 2001, 2000 + d - 1, 1 + sid % 6, SERVER | 1 | (b << 16)) for sid, a, b, d, _ in special]
    cols = cols_from_rows(first + head + filler + tail)
    assert len(cols) <= 512 and (len(head) + len(filler)) >= 64
    with DepsContext(S) as ctx, RealtimeLinks(S) as rl:
        rl.bind(ctx)
        ctx.accumulate(cols, clustered=True, verify=True)
        ctx.finalize()
        assert ctx.stats()["spilled_traces"] == 0
        check_rows_by_rpc(rl, cols, S)
        for sid, _, _, d, want in special:
            par, dur, tid, ids = rl.server_rpc_links(1 + sid % 6)
            at = dur.tolist().index(d)
            assert (par[at], tid[at], ids[at]) == (0, T, want), f"span {sid}"
            sel = rl.server_rpc_links(1 + sid % 6, want)
            assert d in sel[1].tolist()


def test_rpc_bounds(gpu):
    """Ids 0, 1 and 65535 in one batch at S = 4096: the link (parent 4095, child 4095, d = 2^40 - 1,
    the all-ones key) named 65535 is found by (4095, 65535) and absent from (4095, 1); an rpc of
    65536 is an invalid argument; a capacity below the row count is ZK_ERR_CAPACITY."""
    S = 4096
    TOP = S - 1
    cols = star_batch([TOP], [3], [TOP, TOP, TOP], [DMAX, 0, 1 << 21])
    ids = np.zeros(len(cols), np.int64)
    child = cols.parent_id != 0
    ids[child] = np.where(cols.last_ts[child] - cols.first_ts[child] == DMAX, 65535,
                          np.where(cols.last_ts[child] - cols.first_ts[child] == 0, 0, 1))
    cols.set_name_ids(ids)
    tid = int(cols.trace_id[0])
    with DepsContext(S) as ctx, RealtimeLinks(S) as rl:
        rl.bind(ctx)
        ctx.accumulate(cols, clustered=True)
        ctx.sync()
        assert rl.count() == (3, 0)
        rows = rpc_rows.rpc_rows(cols, S)
        rpc_rows.assert_tied_to_oracle(rows, cols, S)
        assert rows == [(TOP, TOP, 0, tid, 0), (TOP, TOP, 1 << 21, tid, 1), (TOP, TOP, DMAX, tid, 65535)]
        assert [g.tolist() for g in rl.server_rpc_links(TOP)] == [[TOP] * 3, [0, 1 << 21, DMAX], [tid] * 3, [0, 1, 65535]]
        assert [g.tolist() for g in rl.server_rpc_links(TOP, 65535)] == [[TOP], [DMAX], [tid], [65535]]
        assert [g.tolist() for g in rl.server_rpc_links(TOP, 1)] == [[TOP], [1 << 21], [tid], [1]]
        assert [g.tolist() for g in rl.server_rpc_links(TOP, 0)] == [[TOP], [0], [tid], [0]]
        assert len(rl.server_rpc_links(TOP, 2)[0]) == 0 and len(rl.server_rpc_links(0, 65535)[0]) == 0
        assert [g.tolist() for g in rl.server_links(TOP)] == [[TOP] * 3, [0, 1 << 21, DMAX], [tid] * 3]
        with pytest.raises(ZkError) as e:
            rl.server_rpc_links(TOP, 65536)
        assert e.value.status == _abi.ZK_ERR_INVALID_ARG
        L, n = _abi.lib(), C.c_uint64()
        par = np.zeros(4, np.uint32)
        assert L.zk_rl_server_rpc_links(rl._h, TOP, _abi.ZK_RL_ANY_RPC, par.ctypes.data, None, None, None, 2,
                                        C.byref(n)) == _abi.ZK_ERR_CAPACITY
        assert n.value == 3
        assert L.zk_rl_server_rpc_links(rl._h, TOP, 65535, par.ctypes.data, None, None, None, 0,
                                        C.byref(n)) == _abi.ZK_ERR_CAPACITY
        # only some outputs wanted, capacity exact
        assert L.zk_rl_server_rpc_links(rl._h, TOP, 65535, par.ctypes.data, None, None, None, 1, C.byref(n)) == _abi.ZK_OK
        assert (n.value, int(par[0])) == (1, TOP)
        with pytest.raises(ZkError) as e:
            rl.server_rpc_links(S, 1)
        assert e.value.status == _abi.ZK_ERR_SERVICE_RANGE


def test_trait_answers_by_rpc_on_the_device(gpu):
    from zipkin_amd.aggregates import Dictionary, GpuRealtimeAggregates

    S = 11
    names = Dictionary([service_name(i) for i in range(S)])
    rpcs = Dictionary(["rpc-%d" % k for k in range(R)])
    a = assign_names(tracegen_host(83, 3000, max_depth=6, num_services=S), 83)
    b = assign_names(tracegen_host(84, 3000, max_depth=6, num_services=S), 84)
    hour = 3_600_000_000
    store = GpuRealtimeAggregates(names, rpcs=rpcs)
    plain = GpuRealtimeAggregates(names)
    store.accumulate(a.take(np.random.default_rng(2).permutation(len(a))), 10 * hour + 5)
    store.accumulate(b, 11 * hour, clustered=True)
    plain.accumulate(a, 10 * hour, clustered=True)

    def answers(rows, server, rpc):
        durs, tids = {}, {}
        for p, c, d, t, n in rows:
            if c == server and (rpc is None or n == rpc):
                durs.setdefault(names.name(p), []).append(d)
                tids.setdefault(names.name(p), set()).add(t - (1 << 64) if t >= 1 << 63 else t)
        return {k: sorted(v) for k, v in durs.items()}, {k: sorted(v) for k, v in tids.items()}

    for cols, t in ((a, 10 * hour), (b, 11 * hour + 17)):
        rows = rpc_rows.rpc_rows(cols, S)
        rpc_rows.assert_tied_to_oracle(rows, cols, S)
        for server in (0, 3, 10):
            sname = names.name(server)
            assert len({r[4] for r in rows if r[1] == server}) >= 3  # several rpcs per server
            every = answers(rows, server, None)
            assert store.getSpanDurations(t, sname, "") == every[0]
            assert store.getServiceNamesToTraceIds(t, sname, "") == every[1]
            if cols is a:  # "" answers as a store without a dictionary does
                assert plain.getSpanDurations(t, sname, "") == every[0]
                assert plain.getServiceNamesToTraceIds(t, sname, "rpc-2") == every[1]
            for rpc, rname in [(0, "Unknown")] + [(k + 1, rpcs.name(k)) for k in range(R)]:
                want = answers(rows, server, rpc)
                assert store.getSpanDurations(t, sname, rname) == want[0], (server, rname)
                assert store.getServiceNamesToTraceIds(t, sname, rname) == want[1], (server, rname)
            assert store.getSpanDurations(t, sname, "no-such-rpc") == {}
            assert store.getServiceNamesToTraceIds(t, sname, "no-such-rpc") == {}
    assert len(rpcs) == R
    store.close()
    plain.close()


def test_device_decoder_refuses_span_names(gpu):
    """zk_ingest_dev_* keeps no span-name dictionary: ZK_INGEST_SPAN_NAMES is ZK_ERR_UNSUPPORTED there
    (checked before any device work, so an empty batch shows it), on each of its three entry points."""
    from zipkin_amd.ingest import DeviceSpanDecoder

    dec = DeviceSpanDecoder(64)
    L, n_out, n_rej = _abi.lib(), C.c_uint64(), C.c_uint64()
    flags = _abi.ZK_INGEST_SPAN_NAMES
    assert L.zk_ingest_dev_spans(dec._h, None, None, 0, _abi.ZK_CODEC_THRIFT, flags, None, C.byref(n_out),
                                 C.byref(n_rej)) == _abi.ZK_ERR_UNSUPPORTED
    items = _abi.zk_ingest_items()
    assert L.zk_ingest_dev_spans_items(dec._h, None, None, 0, _abi.ZK_CODEC_THRIFT, flags | _abi.ZK_INGEST_STRICT, None,
                                       C.byref(n_out), C.byref(n_rej), C.byref(items)) == _abi.ZK_ERR_UNSUPPORTED
    assert L.zk_ingest_dev_spans_multi(dec._h, 0, None, None, None, _abi.ZK_CODEC_THRIFT, flags, None, C.byref(n_out),
                                       C.byref(n_rej), None) == _abi.ZK_ERR_UNSUPPORTED
    assert b"span-name" in L.zk_ingest_dev_last_error(dec._h)
    # without the flag the same empty calls are fine
    assert L.zk_ingest_dev_spans(dec._h, None, None, 0, _abi.ZK_CODEC_THRIFT, 0, None, C.byref(n_out),
                                 C.byref(n_rej)) == _abi.ZK_OK
    dec.close()
