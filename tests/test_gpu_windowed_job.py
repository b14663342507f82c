"""WindowedAggregateJob (zipkin_amd/windows.py): one stored Dependencies record per time window, each
equal to the dependency path run on the records tests/winref.py selects for that window."""
import numpy as np
import pytest

from oracle.moments import Moments as OMoments
from oracle.moments import moments_close
from tests import winref
from tests.bulkfrag import service_name
from zipkin_amd import DepsContext, DeviceColumns, SpanColumns, WindowedAggregateJob, ZkError, _abi, tracegen_host
from zipkin_amd.aggregates import Dictionary, GpuAggregates, ZipkinAggregateJob, _link_durations, links_from_table
from zipkin_amd.realtime import LinkHistogram

pytestmark = pytest.mark.gpu

S = 61
HOUR = 3_600_000_000
BASE_TS = 1_421_053_208_373_000
QS = (0.5, 0.99)
LONE_AT = BASE_TS + 20 * HOUR  # a trace of one span, hours after every other: a window without a link


def lone_trace() -> SpanColumns:
    c = SpanColumns.empty(1)
    c.trace_id[0], c.span_id[0] = 0xABCDEF0123, 1
    c.first_ts[0], c.last_ts[0] = LONE_AT, LONE_AT + 10
    c.service_id[0] = 3
    c.flags[0] = (_abi.ZK_F_HAS_ANNOTATIONS | _abi.ZK_F_SVC_SERVER | (1 << _abi.ZK_F_SR_SHIFT) | (1 << _abi.ZK_F_SS_SHIFT))
    return c


def link_dict(links):
    return {(l.parent.name, l.child.name): tuple(l.duration_moments) for l in links}


@pytest.fixture(scope="module")
def ran(gpu):
    names = Dictionary([service_name(i) for i in range(S)])
    a = tracegen_host(401, 3000, max_depth=6, num_services=S, base_ts=BASE_TS)
    b = SpanColumns.concat([tracegen_host(402, 3000, max_depth=6, num_services=S, base_ts=BASE_TS), lone_trace()])
    agg = GpuAggregates("anorm", services=names, clock=lambda: 10**18)
    job = WindowedAggregateJob(names, window_us=HOUR, aggregates=agg, link_quantiles=QS, device=gpu)
    recs = job.run([DeviceColumns.from_host(a), DeviceColumns.from_host(b)], num_services=S)
    # the reference's selection: each batch's records of window w, batches in order
    origin, W = job.origin, job.num_windows
    sel = {}
    for w in range(W):
        parts = [c.take(winref.window_records(c, origin, HOUR, W, w)) for c in (a, b)]
        sel[w] = SpanColumns.concat(parts)
    yield names, a, b, agg, job, recs, sel
    job.close()


def test_windows_follow_the_data(ran):
    names, a, b, agg, job, recs, sel = ran
    both = SpanColumns.concat([a, b])
    timed = (both.flags & np.uint32(_abi.ZK_F_HAS_ANNOTATIONS)) != 0
    lo, hi = int(both.first_ts[timed].min()), int(both.first_ts[timed].max())
    assert job.origin == lo // HOUR * HOUR and job.num_windows == (hi - job.origin) // HOUR + 1
    assert sum(len(c) for c in sel.values()) + job.rest["untimed_records"] == len(both)
    assert job.rest["before_records"] == job.rest["after_records"] == 0
    assert {w: s["records"] for w, s in job.stats.items()} == {w: len(c) for w, c in sel.items() if len(c)}


def test_one_record_per_window_with_links(ran, gpu):
    names, a, b, agg, job, recs, sel = ran
    want = {}
    with DepsContext(S, device=gpu) as ctx:
        for w, cols in sel.items():
            if not len(cols):
                continue
            ctx.reset()
            ctx.accumulate(cols, clustered=True, verify=True)
            links = links_from_table(ctx.finalize(), names)
            if len(links):
                want[job.origin + w * HOUR] = link_dict(links)
    assert len(want) >= 7
    assert [r.start_time for r in recs] == sorted(want)
    assert agg.count() == len(recs)
    for r in recs:
        assert r.end_time == r.start_time + HOUR
        assert link_dict(r.links) == want[r.start_time]  # bit for bit: the same exact sums
        assert link_dict(agg.getDependencies(r.start_time, r.end_time).links) == want[r.start_time]


def test_a_window_without_links_stores_nothing(ran):
    names, a, b, agg, job, recs, sel = ran
    w = (LONE_AT - job.origin) // HOUR
    assert len(sel[w]) == 1 and job.stats[w]["records"] == 1 and job.stats[w]["joined_links"] == 0
    assert job.origin + w * HOUR not in [r.start_time for r in recs]
    assert agg.getDependencies(job.origin + w * HOUR, job.origin + (w + 1) * HOUR).links == ()


def test_all_windows_sum_to_the_plain_job(ran, gpu):
    names, a, b, agg, job, recs, sel = ran
    plain = ZipkinAggregateJob(names, device=gpu, order="rows", clock=lambda: 10**18)
    whole = link_dict(plain.run([a, b], num_services=S).links)
    plain.close()
    end = job.origin + job.num_windows * HOUR
    total = {}
    for l in agg.getDependencies(job.origin, end).links:
        k = (l.parent.name, l.child.name)
        total[k] = l.duration_moments if k not in total else total[k].plus(l.duration_moments)
    assert set(total) == set(whole)
    for k, m in total.items():
        assert m.m0 == whole[k][0]
        assert moments_close(OMoments(*whole[k]), OMoments(*m)), k


def test_link_durations_per_window(ran, gpu):
    names, a, b, agg, job, recs, sel = ran
    name_list = [names.name(i) for i in range(S)]
    with DepsContext(S, device=gpu) as ctx, LinkHistogram(S, device=gpu) as lh:
        lh.bind(ctx)
        for r in recs:
            w = (r.start_time - job.origin) // HOUR
            ctx.reset()
            lh.reset()
            ctx.accumulate(sel[w], clustered=True, verify=False)
            want = _link_durations(ctx.finalize(), name_list, lh, QS)
            got = agg.getLinkDurations(r.start_time, r.end_time, QS)
            assert got and got == want
            assert agg.getLinkHistogram(r.start_time, r.end_time)[1:] == (1, 1)


def test_a_trace_recurring_in_the_second_batch_fails_the_job(gpu):
    names = Dictionary([service_name(i) for i in range(S)])
    a = tracegen_host(403, 500, max_depth=6, num_services=S, base_ts=BASE_TS)
    b = tracegen_host(404, 500, max_depth=6, num_services=S, base_ts=BASE_TS)
    first = a.take(slice(0, int(winref.run_starts(a.trace_id)[1])))  # a's first trace again, in batch 2
    job = WindowedAggregateJob(names, window_us=HOUR, device=gpu, verify=True)
    try:
        with pytest.raises(ZkError) as e:
            job.run([a, SpanColumns.concat([b, first])], num_services=S)
        assert e.value.status == _abi.ZK_ERR_NOT_CLUSTERED
        assert len(job.run([a, b], num_services=S)) >= 7  # the handle and the context survive a failed run
    finally:
        job.close()


def test_too_many_windows_raises(gpu):
    names = Dictionary([service_name(i) for i in range(S)])
    a = tracegen_host(405, 200, max_depth=5, num_services=S, base_ts=BASE_TS)
    job = WindowedAggregateJob(names, window_us=HOUR, max_windows=3, device=gpu)
    with pytest.raises(ValueError):
        job.run([a], num_services=S)
    job.close()
