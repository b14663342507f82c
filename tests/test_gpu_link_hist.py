"""The per-link duration histogram (include/zksketch.h zk_lh_*) on the GPU, through the C ABI: bound
to a dependency ctx, the histogram of every (parent, child) edge must equal, bin for bin and over ALL
S x S cells, the histogram of the oracle's join rows (oracle/realtime.py joined_links: the job's join
before its group.sum, ZipkinAggregateJob.scala:25-37) in zk_rt's log-linear layout (bins_of) --
clustered and shuffled batches (K1, the group join and its fallback, the trace pass), traces through
the spill kernel and across batch edges, durations at the layout's bounds, several batches, traceId
shards -- while the dependency table stays equal to the dependency oracle and every cell's count
equals the table's m0. Then the quantile queries, the binding rules, the job drivers' side output and
the world-1 all-reduce."""
import functools

import numpy as np
import pytest

from oracle import oracle
from oracle.realtime import bin_bounds, bins_of, exact_quantile, joined_links, nbins, nearest_rank, server_links
from tests.bulkfrag import batches, encode, service_name
from tests.test_gpu_parity import SERVER, assert_parity, cols_from_rows, star_trace
from zipkin_amd import DepsContext, DeviceColumns, SpanColumns, ZkError, _abi, tracegen_host
from zipkin_amd.realtime import LinkHistogram, RealtimeLinks, RtSketch

pytestmark = pytest.mark.gpu


def expected_hist(links, S, m):
    p, c, d, _ = links
    H = np.zeros((S * S, nbins(m)), np.uint32)
    np.add.at(H, (p * S + c, bins_of(d, m)), 1)
    return H


@functools.lru_cache(maxsize=None)
def generated(seed, traces, S):
    """(columns, their join rows, their dependency oracle): computed once per batch, never changed."""
    cols = tracegen_host(seed, traces, max_depth=6, num_services=S)
    return cols, joined_links(cols, S), oracle.aggregate(cols, S)


def check(ctx, lh, links, ref, S):
    """Table against the dependency oracle, histogram against the join rows over every cell, and each
    cell's count against the table's m0. Returns the histogram read."""
    got = ctx.finalize()
    assert_parity(got, ctx.stats(), ref)
    H = lh.read()
    want = expected_hist(links, S, lh.m)
    assert H.shape == want.shape
    assert np.array_equal(H, want), f"{np.count_nonzero((H != want).any(axis=1))} cells differ"
    _, _, cnt = lh.quantiles_all(())
    assert np.array_equal(cnt, got.m0)
    return H


@pytest.mark.parametrize("S,m", [(9, 0), (61, 0), (363, 0), (61, 2), (61, 7)])
def test_geometry(gpu, S, m):
    """S = 363: 258 cell buckets, every (bucket, tile) its own workgroup (plain adds); S = 61 and 9:
    few buckets, split over workgroups (atomic flush); m = 2 / 7: the largest / smallest tile."""
    cols, links, ref = generated(70 + S, 20_000, S)
    with DepsContext(S) as ctx, LinkHistogram(S, sub_bits=m) as lh:
        assert lh.bins == lh.geometry() == nbins(m or 4)
        lh.bind(ctx)
        ctx.accumulate(cols, clustered=True, verify=True)
        check(ctx, lh, links, ref, S)


def test_no_bucket_order(gpu):
    """S = 1025, the smallest table without cell buckets (the reduce is the atomic one): the handle
    reads the K1 lists themselves. 164 M counters (655 MB) at m = 2, compared in slices of cells."""
    S, m = 1025, 2
    cols = tracegen_host(91, 5_000, max_depth=6, num_services=S)
    p, c, d, _ = joined_links(cols, S)
    cell, b = p * S + c, bins_of(d, m)
    with DepsContext(S) as ctx, LinkHistogram(S, sub_bits=m) as lh:
        lh.bind(ctx)
        ctx.accumulate(cols, clustered=True, verify=True)
        got = ctx.finalize()
        assert_parity(got, ctx.stats(), oracle.aggregate(cols, S))
        step = 1 << 16
        for a in range(0, S * S, step):
            n = min(step, S * S - a)
            want = np.zeros((n, nbins(m)), np.uint32)
            sel = (cell >= a) & (cell < a + n)
            np.add.at(want, (cell[sel] - a, b[sel]), 1)
            assert np.array_equal(lh.read(a, n), want), f"cells [{a}, {a + n})"
        assert np.array_equal(lh.quantiles_all(())[2], got.m0)


def test_clustered_verified(gpu):
    S = 61
    cols, links, ref = generated(70 + S, 20_000, S)
    with DepsContext(S) as ctx, LinkHistogram(S) as lh:
        lh.bind(ctx)
        ctx.accumulate(DeviceColumns.from_host(cols), clustered=True, verify=True)
        check(ctx, lh, links, ref, S)


@pytest.mark.parametrize("trace_pass", [False, True])
def test_shuffled_batch(gpu, trace_pass):
    """More than 2^18 records in any order, unverified: the group join (and K1 as its fallback) write
    the links; with trace_pass the clustering pass and K1 do. The handle does not change the path."""
    S = 61
    cols, links, ref = generated(77, 15_000, S)
    assert len(cols) > 1 << 18
    shuffled = cols.take(np.random.default_rng(77).permutation(len(cols)))
    with DepsContext(S, trace_pass=trace_pass) as ctx, LinkHistogram(S) as lh:
        lh.bind(ctx)
        ctx.accumulate(shuffled, clustered=False, verify=False)
        check(ctx, lh, links, ref, S)


def test_spilled_and_continued_traces(gpu):
    """Links from the spill kernel (a 12k-record trace) and from held traces joined across batch
    edges, host and device batches alternating."""
    S = 9
    rows = []
    for t in range(40):
        rows += star_trace(100 + t, 1 + t % 6, svc_root=t % S, nsvc=S)
    rows += star_trace(7777, 6_000, nsvc=S)  # 12k records: longer than a K1 window -> spill kernel
    for t in range(40):
        rows += star_trace(900 + t, 1 + t % 5, svc_root=t % S, nsvc=S)
    big = cols_from_rows(rows)
    tg = tracegen_host(72, 6000, max_depth=6, num_services=S)
    cols = SpanColumns.concat([big, tg])
    cuts = sorted(np.random.default_rng(72).choice(np.arange(1, len(cols)), 5, replace=False).tolist())
    bounds = [0, *cuts, len(cols)]
    with DepsContext(S) as ctx, LinkHistogram(S) as lh:
        lh.bind(ctx)
        for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            part = cols.take(slice(a, b))
            ctx.accumulate(DeviceColumns.from_host(part) if i % 2 else part, clustered=True, verify=True,
                           continues=i + 2 < len(bounds))
        check(ctx, lh, joined_links(cols, S), oracle.aggregate(cols, S), S)
        assert ctx.stats()["spilled_traces"] >= 1
        assert lh.dropped() == 0


@pytest.mark.parametrize("m", [2, 4, 7])
def test_duration_bounds(gpu, m):
    """Child durations at the layout's bounds on the table's last and first cell; 2^40 us is dropped
    by the dependency path: counted by dropped() and zk_stats.duration_range, in no bin."""
    S = 5
    ds = [0, (1 << m) - 1, 1 << m, 1 << 21, (1 << 40) - 1]

    def traces(durations):
        rows, tid = [], 1
        for svc in (S - 1, 0):
            for d in durations:
                rows += [(tid, 10 * tid, 0, 1, 2**41, svc, SERVER), (tid, 10 * tid + 1, 10 * tid, 5, 5 + d, svc, SERVER | 1)]
                tid += 1
        return cols_from_rows(rows)

    good, every = traces(ds), traces(ds + [1 << 40])
    with DepsContext(S) as ctx, LinkHistogram(S, sub_bits=m) as lh:
        lh.bind(ctx)
        ctx.accumulate(every, clustered=True)
        with pytest.raises(ZkError) as e:
            ctx.finalize()
        assert e.value.status == _abi.ZK_ERR_DURATION_RANGE
        assert ctx.stats()["duration_range"] == 2 and lh.dropped() == 2
        want = expected_hist(joined_links(good, S), S, m)
        assert want.sum() == 2 * len(ds)
        for cell in ((S - 1) * S + S - 1, 0):
            assert np.array_equal(np.flatnonzero(want[cell]), np.unique(bins_of(ds, m)))
        assert np.array_equal(lh.read(), want)
        assert lh.quantiles(S - 1, S - 1, (0.0, 1.0)) == ([(0, 0), bin_bounds(nbins(m) - 1, m)], len(ds))
        # the same batch without the dropped links: the same histogram, and the table is the oracle's
        ctx.reset()
        lh.reset()
        ctx.accumulate(good, clustered=True)
        H = check(ctx, lh, joined_links(good, S), oracle.aggregate(good, S), S)
        assert np.array_equal(H, want) and lh.dropped() == 0


def test_quantiles(gpu):
    S = 61
    qs = (0.0, 0.5, 0.99, 1.0)
    cols, links, ref = generated(70 + S, 20_000, S)
    p, c, d, _ = links
    with DepsContext(S) as ctx, LinkHistogram(S) as lh:
        lh.bind(ctx)
        ctx.accumulate(cols, clustered=True)
        ctx.finalize()
        lo, hi, cnt = lh.quantiles_all(qs)
        cell = p * S + c
        order = np.argsort(cell, kind="stable")
        cs, dsort = cell[order], d[order]
        present = np.unique(cs)
        assert len(present) > 1000
        starts, ends = np.searchsorted(cs, present, "left"), np.searchsorted(cs, present, "right")
        for x, a, b in zip(present.tolist(), starts.tolist(), ends.tolist()):  # every present cell
            assert cnt[x] == b - a
            for i, q in enumerate(qs):
                exact = exact_quantile(dsort[a:b], q)
                assert lo[x, i] <= exact <= hi[x, i], (x, q)
                assert (lo[x, i], hi[x, i]) == bin_bounds(int(bins_of([exact], lh.m)[0]), lh.m), (x, q)
        absent = np.setdiff1d(np.arange(S * S), present)
        assert len(absent) and not cnt[absent].any() and not lo[absent].any() and not hi[absent].any()
        rng = np.random.default_rng(5)
        for x in np.r_[rng.choice(present, 45, replace=False), rng.choice(absent, 5, replace=False)].tolist():
            bounds, n = lh.quantiles(x // S, x % S, qs)
            assert n == cnt[x] and bounds == [(int(a), int(b)) for a, b in zip(lo[x], hi[x])]
        with pytest.raises(ZkError):
            lh.quantiles(S, 0, qs)
        with pytest.raises(ZkError):
            lh.quantiles_all((1.5,))
        # more quantiles than one device pass takes
        many = tuple(np.linspace(0, 1, 19))
        lo2, hi2, _ = lh.quantiles_all(many)
        x = int(present[0])
        assert lh.quantiles(x // S, x % S, many)[0] == [(int(a), int(b)) for a, b in zip(lo2[x], hi2[x])]


def test_monoid_shards_and_resets(gpu):
    from zipkin_amd.shards import split

    S = 61
    cols, links, ref = generated(70 + S, 20_000, S)
    want = expected_hist(links, S, 4)
    # three batches of whole traces: the same histogram as one batch
    tid = np.asarray(cols.trace_id)
    edges = np.flatnonzero(tid[1:] != tid[:-1]) + 1
    cuts = [0, int(edges[len(edges) // 3]), int(edges[2 * len(edges) // 3]), len(cols)]
    with DepsContext(S) as ctx, LinkHistogram(S) as lh:
        lh.bind(ctx)
        for a, b in zip(cuts[:-1], cuts[1:]):
            ctx.accumulate(cols.take(slice(a, b)), clustered=True, verify=True)
        check(ctx, lh, links, ref, S)
        # a handle kept bound across zk_deps_reset keeps counting; its own reset zeroes it
        ctx.reset()
        ctx.accumulate(cols, clustered=True)
        ctx.finalize()
        assert np.array_equal(lh.read(), 2 * want)
        assert np.array_equal(lh.read(7, 3), 2 * want[7:10])
        lh.reset()
        assert not lh.read().any() and lh.dropped() == 0
        with pytest.raises(ZkError):
            lh.read(S * S - 1, 2)
    # two traceId shards, each with its own ctx and handle: the sum is the whole set's, bit for bit
    parts = split(cols, 2)
    assert all(len(x) for x in parts)
    reads = []
    for part in parts:
        with DepsContext(S) as ctx, LinkHistogram(S) as lh:
            lh.bind(ctx)
            ctx.accumulate(part, clustered=True)
            ctx.finalize()
            reads.append(lh.read())
    assert np.array_equal(reads[0] + reads[1], want)


def test_binding_rules(gpu):
    S = 5
    with DepsContext(S) as ctx, LinkHistogram(S) as lh, LinkHistogram(S + 1) as other, RtSketch(S) as rt:
        with pytest.raises(ZkError) as e:
            other.bind(ctx)  # num_services differ
        assert e.value.status == _abi.ZK_ERR_INVALID_ARG
        rt.bind(ctx, only=True)  # ZK_RT_ONLY: no links
        with pytest.raises(ZkError) as e:
            lh.bind(ctx)
        assert e.value.status == _abi.ZK_ERR_UNSUPPORTED
        rt.unbind()
        lh.bind(ctx)
        with pytest.raises(ZkError) as e:
            rt.bind(ctx, only=True)
        assert e.value.status == _abi.ZK_ERR_UNSUPPORTED
        rt.bind(ctx)  # ZK_RT_WITH_DEPS coexists
        cols = cols_from_rows(star_trace(3, 4, nsvc=S))
        ctx.accumulate(cols, clustered=True)
        check(ctx, lh, joined_links(cols, S), oracle.aggregate(cols, S), S)
        rt.unbind()
        lh.unbind()


@pytest.mark.parametrize("clustered", [True, False])
def test_with_a_realtime_link_store(gpu, clustered):
    """A zk_rl store on the same ctx: its rows and the histogram are both right."""
    S = 61
    cols, links, ref = generated(70 + S, 20_000, S)
    batch = cols if clustered else cols.take(np.random.default_rng(3).permutation(len(cols)))
    with DepsContext(S) as ctx, RealtimeLinks(S) as rl, LinkHistogram(S) as lh:
        rl.bind(ctx)
        lh.bind(ctx)
        ctx.accumulate(batch, clustered=clustered, verify=clustered)
        check(ctx, lh, links, ref, S)
        assert rl.count() == (len(links[0]), 0)
        for s in range(S):
            got, want = rl.server_links(s), server_links(links, s)
            for g, w, name in zip(got, want, ("parent", "duration", "traceId")):
                t = np.uint64 if name == "traceId" else np.int64
                assert np.array_equal(g.astype(t), w.astype(t)), f"server {s}: {name}"


def expected_durations(links, S, m, qs):
    """{(parent name, child name): (count, {q: bin bounds})} of the oracle's per-link bins."""
    H = expected_hist(links, S, m)
    out = {}
    for x in np.flatnonzero(H.any(axis=1)).tolist():
        cum = np.cumsum(H[x].astype(np.int64))
        n = int(cum[-1])
        out[(service_name(x // S), service_name(x % S))] = (
            n, {float(q): bin_bounds(int(np.searchsorted(cum, nearest_rank(q, n), side="left")), m) for q in qs})
    return out


def test_job_surface(gpu):
    import torch

    from zipkin_amd.aggregates import Dictionary, LinkDuration, StoredSpanJob, ZipkinAggregateJob

    S, qs = 61, (0.5, 0.99)
    cols, links, ref = generated(70 + S, 20_000, S)
    want = expected_durations(links, S, 4, qs)
    names = Dictionary([service_name(i) for i in range(S)])
    half = (np.asarray(cols.trace_id) % np.uint64(2)).astype(np.int64)
    parts = [cols.take(np.flatnonzero(half == k)) for k in range(2)]
    job = ZipkinAggregateJob(names, clock=lambda: 10**15, link_quantiles=qs)
    plain = ZipkinAggregateJob(names, clock=lambda: 10**15)
    for _ in range(2):  # (the second run reuses the job's context and handle, reset)
        deps = job.run(parts, S)
        got = job.link_durations()
        assert all(isinstance(x, LinkDuration) for x in got)
        assert [(x.parent, x.child) for x in got] == [(l.parent.name, l.child.name) for l in deps.links]
        assert {(x.parent, x.child): (x.count, x.quantiles) for x in got} == want
    assert deps == plain.run(parts, S) and plain.link_durations() == []
    job.close()
    plain.close()
    # stored fragments already in HBM, through the device decoder
    small = tracegen_host(88, 3_000, max_depth=6, num_services=S)
    buf, off, exp = encode(small)
    cuts = [len(small) // 3]
    dev = [(torch.from_numpy(b).cuda(), torch.from_numpy(o.view(np.int64)).cuda(), len(o) - 1)
           for b, o in batches(buf, off, cuts)]
    want = expected_durations(joined_links(exp, S), S, 4, qs)
    sjob = StoredSpanJob(clock=lambda: 10**15, max_services=S, link_quantiles=qs)
    splain = StoredSpanJob(clock=lambda: 10**15, max_services=S)
    for _ in range(2):
        deps = sjob.run_device(dev, indexer=False)
        got = sjob.link_durations()
        assert [(x.parent, x.child) for x in got] == [(l.parent.name, l.child.name) for l in deps.links]
        assert {(x.parent, x.child): (x.count, x.quantiles) for x in got} == want
    pdeps = splain.run_device(dev, indexer=False)
    assert {(l.parent.name, l.child.name): tuple(l.duration_moments) for l in deps.links} == \
        {(l.parent.name, l.child.name): tuple(l.duration_moments) for l in pdeps.links}
    # the host-decode driver gives the same side output
    hjob = StoredSpanJob(clock=lambda: 10**15, max_services=S, link_quantiles=qs)
    hjob.run(batches(buf, off, cuts))
    assert {(x.parent, x.child): (x.count, x.quantiles) for x in hjob.link_durations()} == want
    sjob.close()
    splain.close()


def test_allreduce_at_world_one_is_identity(gpu):
    from zipkin_amd.comm import Comm, unique_id

    S = 61
    cols, links, ref = generated(70 + S, 20_000, S)
    with Comm(unique_id(), 0, 1, device=0) as comm, DepsContext(S) as ctx, LinkHistogram(S) as lh:
        lh.bind(ctx)
        ctx.accumulate(cols, clustered=True)
        before = lh.read()
        ptr, nbytes = lh.partial()
        assert ptr and nbytes == S * S * lh.bins * 4
        comm.allreduce_lh(lh)
        assert np.array_equal(lh.read(), before) and lh.dropped() == 0
        check(ctx, lh, links, ref, S)
