"""max_trace_records and the held-trace plan (ZK_BATCH_CONTINUES) at their exact bounds, through the
C ABI on the GPU.

The contract (zkagg.h): the result equals the job over the whole stream wherever a reader cut it, and
a trace of more than max_trace_records records is counted once in trace_too_large and not aggregated.
tests/carryref.py holds the reference (`expected`: the oracle over the stream without its long runs),
the cases (targets of L - 1 .. 2L + 5 records cut around the plan's 256-record search rounds, around
both ends and so that held + leading records come to exactly L and L + 1) and the classifier that
tests/test_carry_cases.py uses to show which branch of k_carry_plan each case reaches.

Every comparison is exact: the decoded accumulator (read from a caller-owned table, so it is there
after finalize raised) equals the reference's power sums cell for cell, and every counter equals the
reference's."""
import functools

import numpy as np
import pytest

from oracle import oracle
from oracle.realtime import bins_of, joined_links, nbins, server_links
from tests import carryref
from tests.carryref import LS, TARGETS, expected, expected_cells, expected_of, family, reduced, trace_of
from tests.test_gpu_parity import assert_parity
from tests.test_gpu_sharded import Shard
from zipkin_amd import DepsContext, DeviceColumns, SpanColumns, ZkError, _abi, table, tracegen_host
from zipkin_amd.realtime import LinkHistogram, RealtimeLinks, RtSketch

pytestmark = pytest.mark.gpu

TILE = 512        # records of one K1 window: the least max_trace_records
GROUP_CAP = 2048  # records of one sub-bucket of the group join: it runs when max_trace_records >= this


def feed(ctx, parts, flags, device, verify, clustered=True):
    for p, cont in zip(parts, flags):
        b = DeviceColumns.from_host(p) if device and len(p) else p
        ctx.accumulate(b, clustered=clustered, verify=verify, continues=cont)


def read_table(sh, S):
    sh.ctx.sync()
    return table.decode(sh.table.cpu().numpy(), S)


def finish(sh, S):
    """finalize -> (table or None, status or None, the decoded accumulator, the counters)."""
    try:
        got, status = sh.ctx.finalize(), None
    except ZkError as e:
        got, status = None, e.status
    return got, status, read_table(sh, S), sh.ctx.stats()


def check(got, status, cells, st, ref, where):
    """Table, counters and status against the reference; a failure lists everything that differs."""
    want = expected_cells(ref)
    errs = []
    if cells.keys() != want.keys():
        errs.append(f"present cells differ: {sorted(cells.keys() ^ want.keys())[:6]}")
    bad = [k for k in want if k in cells and cells[k] != want[k]]
    if bad:
        errs.append(f"power sums differ in {len(bad)} cells, first {bad[0]}: {cells[bad[0]]} != {want[bad[0]]}")
    for k, v in ref.stats.items():
        if k != "spilled_traces" and st[k] != v:  # (a scheduling detail of the device path, not a result)
            errs.append(f"stat {k}: gpu {st[k]} != reference {v}")
    if st["not_clustered"]:
        errs.append(f"not_clustered {st['not_clustered']}")
    if status != (_abi.ZK_ERR_TRACE_TOO_LARGE if ref.stats["trace_too_large"] else None):
        errs.append(f"status {status}")
    assert not errs, f"{where}: " + "; ".join(errs)
    if status is None:
        assert_parity(got, st, ref)


def run_case(c, device, verify):
    sh = Shard(c.S, max_trace_records=c.L)
    try:
        feed(sh.ctx, c.parts, c.flags, device, verify)
        ref = expected_of(c)
        if c.end == "partial":
            sh.ctx.partial()
        if c.end in ("partial", "empty"):  # the held trace is joined by now, before finalize
            assert read_table(sh, c.S) == expected_cells(ref), f"{c.name}: the table before finalize"
            assert sh.ctx.stats()["records"] == ref.stats["records"], c.name
        out = finish(sh, c.S)
        check(*out, ref, f"{c.name} device={device} verify={verify}")
        return out[2], out[3]
    finally:
        sh.close()


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("L", LS)
def test_cases_equal_the_whole_stream_reference(gpu, L, target, device, verify):
    """Every case of one target length: table, counters, trace_too_large, not_clustered, status."""
    fam = family(L, target)
    assert len(fam) >= 20
    for c in fam:
        run_case(c, device, verify)


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("L", LS)
def test_cut_invariance(gpu, L, target):
    """The uncut stream as one plain batch, and every cut version of it, leave the same decoded table
    and the same counters (spilled_traces apart: how many windows a trace met is not a result)."""
    for tail in (True, False):
        key, cols, a, b = carryref.stream(L, carryref.S_OF[L], target, tail=tail)
        S = carryref.S_OF[L]
        sh = Shard(S, max_trace_records=L)
        try:
            sh.ctx.accumulate(cols, clustered=True, verify=True)
            _, status, cells0, st0 = finish(sh, S)
        finally:
            sh.close()
        st0.pop("spilled_traces")
        assert (status == _abi.ZK_ERR_TRACE_TOO_LARGE) == (b - a > L) and status in (None, _abi.ZK_ERR_TRACE_TOO_LARGE)
        for c in (c for c in family(L, target) if c.key == key):
            cells, st = run_case(c, False, True)
            st.pop("spilled_traces")
            assert cells == cells0, c.name
            assert st == st0, f"{c.name}: {st} != {st0}"


# ---------------------------------------------------------------------------------------------
# the bound on the paths without continuation
def bound_stream(L, k, S, odd):
    """short traces, (one record, so that the trace starts at an odd offset,) a trace of L + k
    records, short traces."""
    pre = carryref.short_traces(11, S)
    if (len(pre) % 2 == 1) != odd:
        pre = SpanColumns.concat([pre, trace_of(0x51, 1, S)])
    return SpanColumns.concat([pre, trace_of(carryref.TARGET_TID, L + k, S), carryref.short_traces(12, S)])


def run_plain(cols, S, L, clustered, device, where, **kw):
    ref = expected(cols, S, L)
    sh = Shard(S, max_trace_records=L, **kw)
    try:
        sh.ctx.accumulate(DeviceColumns.from_host(cols) if device else cols, clustered=clustered, verify=clustered)
        out = finish(sh, S)
        check(*out, ref, where)
        return ref, out[3]
    finally:
        sh.close()


@pytest.mark.parametrize("k", [-1, 0, 1])
@pytest.mark.parametrize("L", LS)
def test_clustered_batch_at_the_bound(gpu, L, k):
    """L = 512: a trace of L records fits one K1 window, L + 1 is spilled and refused; L = 1000: all
    three lengths go through the spill kernel. At an even and an odd offset, host and device."""
    S = carryref.S_OF[L]
    for odd in (False, True):
        cols = bound_stream(L, k, S, odd)
        for device in (False, True):
            ref, st = run_plain(cols, S, L, True, device, f"L={L} k={k} odd={odd} device={device}")
            assert ref.stats["trace_too_large"] == (1 if k > 0 else 0)
            if L > TILE:
                assert st["spilled_traces"] == 1


@pytest.mark.parametrize("k", [-1, 0, 1])
def test_unclustered_batch_on_the_trace_pass_at_the_bound(gpu, k):
    L, S = 1000, 41
    cols = bound_stream(L, k, S, False)
    cols = cols.take(np.random.default_rng(5 + k).permutation(len(cols)))
    ref = expected(bound_stream(L, k, S, False), S, L)
    sh = Shard(S, max_trace_records=L, trace_pass=True)
    try:
        sh.ctx.accumulate(cols, clustered=False, verify=True)
        check(*finish(sh, S), ref, f"trace pass k={k}")
    finally:
        sh.close()
    assert ref.stats["trace_too_large"] == (1 if k > 0 else 0)


@functools.lru_cache(maxsize=None)
def group_batch():
    S = 61
    base = tracegen_host(77, 15_000, max_depth=6, num_services=S)
    assert len(base) > 1 << 18
    return S, base


@pytest.mark.parametrize("longest", [GROUP_CAP, GROUP_CAP + 1])
def test_group_join_at_its_capacity(gpu, longest):
    """max_trace_records = the group join's capacity, a shuffled batch just over 2^18 records without
    the trace check: traces of 2047 and 2048 records are aggregated (through its fallback), one of
    2049 is refused, and the rest of the batch is untouched by it."""
    S, base = group_batch()
    big = [trace_of(0xB160 + n, n, S) for n in range(GROUP_CAP - 1, longest + 1)]
    cols = SpanColumns.concat([base, *big])
    ref = expected(cols, S, GROUP_CAP)
    assert ref.stats["trace_too_large"] == longest - GROUP_CAP
    shuffled = cols.take(np.random.default_rng(longest).permutation(len(cols)))
    sh = Shard(S, max_trace_records=GROUP_CAP)
    try:
        sh.ctx.accumulate(shuffled, clustered=False, verify=False)
        check(*finish(sh, S), ref, f"group join, longest {longest}")
    finally:
        sh.close()


def test_least_max_trace_records(gpu):
    """zk_ctx_create refuses a bound below one K1 window (K1 does not look at the bound, the held-trace
    plan does: the result would depend on the cuts); the least accepted bound is exact at 512 and 513
    records, uncut and cut."""
    for L in (1, TILE - 1):
        with pytest.raises(ZkError) as e:
            DepsContext(7, max_trace_records=L)
        assert e.value.status == _abi.ZK_ERR_INVALID_ARG
    S = 7
    for k in (0, 1):
        cols = bound_stream(TILE, k, S, False)
        ref, _ = run_plain(cols, S, TILE, True, False, f"L=512 k={k}")
        assert ref.stats["trace_too_large"] == k
        a = len(carryref.short_traces(11, S))
        for at in (a + 1, a + 256, a + TILE):
            sh = Shard(S, max_trace_records=TILE)
            try:
                feed(sh.ctx, carryref.cut(cols, [at]), [True, False], False, True)
                check(*finish(sh, S), ref, f"L=512 k={k} cut at {at - a}")
            finally:
                sh.close()


# ---------------------------------------------------------------------------------------------
# bound handles on the carry path
def boundary_family():
    """held_L and held_L_plus_1 (the target held whole: cut at its start and end) and
    append_to_L_plus_1 (cut inside the L + 1 target), at L = 512."""
    L = 512
    by = {c.name: c for c in carryref.cases() if c.L == L}
    names = ("L512-L:a+0_b-0", "L512-L+1:a+0_b-0", "L512-L+1:a+256", "L512-L:b-0", "L512-L+1:b-0",
             "L512-L-last:a:finalize", "L512-L+1-last:a:finalize")
    out = [by[n] for n in names]
    seen = set()
    for c in out:
        for cls in carryref.classify(L, c.parts, c.flags):
            seen |= cls
    assert {"held_L", "held_L_plus_1", "append_to_L_plus_1"} <= seen
    return out


@pytest.mark.parametrize("device", [False, True])
def test_realtime_links_on_the_carry_path(gpu, device):
    """A RealtimeLinks store bound: its rows are the join rows of the stream without its long trace."""
    for c in boundary_family():
        ref = expected_of(c)
        kept, _ = reduced(c.stream, c.L)
        links = joined_links(kept, c.S)
        sh = Shard(c.S, max_trace_records=c.L)
        try:
            with RealtimeLinks(c.S) as rl:
                rl.bind(sh.ctx)
                feed(sh.ctx, c.parts, c.flags, device, True)
                check(*finish(sh, c.S), ref, c.name)
                assert rl.count() == (len(links[0]), 0), c.name
                for s in range(c.S):
                    for g, w, name in zip(rl.server_links(s), server_links(links, s), ("parent", "duration", "traceId")):
                        dt = np.uint64 if name == "traceId" else np.int64
                        assert np.array_equal(g.astype(dt), w.astype(dt)), f"{c.name}: server {s}: {name}"
                rl.unbind()
        finally:
            sh.close()


def test_link_histogram_on_the_carry_path(gpu):
    """A link histogram bound: the cut stream leaves exactly the bins the uncut stream leaves, which
    are the bins of the join rows of the stream without its long trace."""
    for c in boundary_family():
        ref = expected_of(c)
        kept, _ = reduced(c.stream, c.L)
        p, ch, d, _ = joined_links(kept, c.S)
        reads = []
        for parts, flags in ((c.parts, c.flags), ([c.stream], [False])):
            sh = Shard(c.S, max_trace_records=c.L)
            try:
                with LinkHistogram(c.S) as lh:
                    lh.bind(sh.ctx)
                    feed(sh.ctx, parts, flags, False, True)
                    check(*finish(sh, c.S), ref, c.name)
                    reads.append((lh.read().copy(), lh.dropped()))
                    m = lh.m
                    lh.unbind()
            finally:
                sh.close()
        want = np.zeros((c.S * c.S, nbins(m)), np.uint32)
        np.add.at(want, (p * c.S + ch, bins_of(d, m)), 1)
        assert np.array_equal(reads[0][0], want), f"{c.name}: bins of the cut stream"
        assert np.array_equal(reads[1][0], want), f"{c.name}: bins of the uncut stream"
        assert reads[0][1] == reads[1][1] == 0, c.name


def test_sketch_on_the_carry_path(gpu):
    """An RtSketch bound beside the dependency join: the held trace goes through the spill kernel alone
    (K1 cannot append to the item lists). The cut stream leaves the registers, bins and drop counts of
    the uncut stream, and the table of the reference."""
    for c in boundary_family():
        ref = expected_of(c)
        reads = []
        for parts, flags in ((c.parts, c.flags), ([c.stream], [False])):
            sh = Shard(c.S, max_trace_records=c.L)
            try:
                with RtSketch(c.S) as rt:
                    rt.bind(sh.ctx, only=False)
                    feed(sh.ctx, parts, flags, False, True)
                    check(*finish(sh, c.S), ref, c.name)
                    regs, hist = rt.read()
                    reads.append((regs.copy(), hist.copy(), rt.dropped()))
                    rt.unbind()
            finally:
                sh.close()
        assert np.array_equal(reads[0][0], reads[1][0]), f"{c.name}: HLL registers differ"
        assert np.array_equal(reads[0][1], reads[1][1]), f"{c.name}: histogram bins differ"
        assert reads[0][2] == reads[1][2], c.name
        assert reads[0][0].any() and reads[0][1].any()
