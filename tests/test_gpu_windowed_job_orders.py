"""WindowedAggregateJob(order="rows" / "any") (zipkin_amd/windows.py): trace-clustered input cut into
batches anywhere, and records in any order, give the records order="whole" gives on the uncut set, and
every window equals the C oracle on the records tests/winref.py selects for it."""
import numpy as np
import pytest

from oracle import oracle
from oracle.moments import Moments as OMoments
from oracle.moments import moments_close
from tests import winref, winref_table
from tests.bulkfrag import service_name
from tests.test_gpu_parity import cols_from_rows, star_trace
from zipkin_amd import SpanColumns, WindowedAggregateJob, ZkError, _abi, tracegen_host
from zipkin_amd.aggregates import Dictionary, GpuAggregates, ZipkinAggregateJob, links_from_table
from zipkin_amd.context import LinkTable

pytestmark = pytest.mark.gpu

S = 61
HOUR = 3_600_000_000
BASE_TS = 1_421_053_208_373_000
QS = (0.5, 0.99)
LONE_AT = BASE_TS + 20 * HOUR  # a trace of one span, hours after every other: a window without a link
BIG = 0xB16B16
# the big trace starts 500 us before an hour ends and its children go on into the next hour: the
# batches that hold only its later fragments would, by their own records, put them in the next window
BIG_T0 = (BASE_TS - 3 * HOUR) // HOUR * HOUR + HOUR - 500


def lone_trace() -> SpanColumns:
    c = SpanColumns.empty(1)
    c.trace_id[0], c.span_id[0] = 0xABCDEF0123, 1
    c.first_ts[0], c.last_ts[0] = LONE_AT, LONE_AT + 10
    c.service_id[0] = 3
    c.flags[0] = (_abi.ZK_F_HAS_ANNOTATIONS | _abi.ZK_F_SVC_SERVER | (1 << _abi.ZK_F_SR_SHIFT) | (1 << _abi.ZK_F_SS_SHIFT))
    return c


def link_dict(links):
    return {(l.parent.name, l.child.name): tuple(l.duration_moments) for l in links}


def run_job(names, batches, gpu, **kw):
    agg = GpuAggregates("anorm", services=names, clock=lambda: 10**18)
    job = WindowedAggregateJob(names, window_us=HOUR, aggregates=agg, link_quantiles=QS, device=gpu, verify=True, **kw)
    try:
        recs = job.run(batches, num_services=S)
        return dict(recs=recs, agg=agg, origin=job.origin, W=job.num_windows, stats=dict(job.stats), rest=dict(job.rest),
                    hists=set(job.link_histograms))
    finally:
        job.close()


@pytest.fixture(scope="module")
def world(gpu):
    names = Dictionary([service_name(i) for i in range(S)])
    a = tracegen_host(411, 1500, max_depth=6, num_services=S, base_ts=BASE_TS)
    b = tracegen_host(412, 1500, max_depth=6, num_services=S, base_ts=BASE_TS)
    big = cols_from_rows(star_trace(BIG, 1100, svc_root=2, nsvc=S, t0=BIG_T0))
    assert len(big) > 2000
    cols = SpanColumns.concat([a, big, b, lone_trace()])
    big0 = len(a)
    whole = run_job(names, [cols], gpu)
    return dict(names=names, cols=cols, big0=big0, big1=big0 + len(big), whole=whole)


def cuts_for(world, batches, seed):
    """batches - 1 cut positions: two at random inside the big trace (it spans three batches), the others
    at random anywhere else."""
    rng = np.random.default_rng(seed)
    inside = rng.choice(np.arange(world["big0"] + 1, world["big1"]), 2, replace=False).tolist()
    n = len(world["cols"])
    other = []
    while len(other) < batches - 3:
        p = int(rng.integers(1, n))
        if not world["big0"] <= p <= world["big1"] and p not in other:
            other.append(p)
    return sorted(inside + other)


def same_records(got, whole):
    assert (got["origin"], got["W"]) == (whole["origin"], whole["W"])
    assert [(r.start_time, r.end_time) for r in got["recs"]] == [(r.start_time, r.end_time) for r in whole["recs"]]
    for r, q in zip(got["recs"], whole["recs"]):
        assert link_dict(r.links) == link_dict(q.links), r.start_time  # m0..m4 bit for bit
    for k in ("before_records", "after_records", "untimed_records"):  # (runs differ: a cut run counts twice)
        assert got["rest"][k] == whole["rest"][k], k
    assert got["hists"] == whole["hists"]
    assert got["agg"].count() == whole["agg"].count() == len(whole["recs"])
    for r in whole["recs"]:
        want = whole["agg"].getLinkDurations(r.start_time, r.end_time, QS)
        assert want and got["agg"].getLinkDurations(r.start_time, r.end_time, QS) == want
        assert got["agg"].getLinkHistogram(r.start_time, r.end_time)[1:] == (1, 1)


@pytest.fixture(scope="module", params=["rows-3", "rows-5", "any-4"])
def ran(request, world, gpu):
    """order="rows" on the set cut into 3 and into 5 batches (the big trace over three of them), and
    order="any" on the set globally permuted, then cut into 4."""
    order, k = request.param.split("-")
    k = int(k)
    if order == "rows":
        parts = winref_table.cut(world["cols"], cuts_for(world, k, k))
        assert sum(bool((p.trace_id == np.uint64(BIG)).any()) for p in parts) == 3
    else:
        cols = winref_table.shuffled(world["cols"], 17)
        n = len(cols)
        parts = winref_table.cut(cols, [n // 4 + 1, n // 2 + 3, 3 * n // 4])
    assert len(parts) == k
    got = run_job(world["names"], parts, gpu, order=order)
    got["order"] = order
    return got


def test_the_set(world):
    w = world["whole"]
    assert 6 <= len(w["recs"]) and w["W"] >= 20 and 50_000 <= len(world["cols"]) <= 200_000


def test_equals_whole(ran, world):
    same_records(ran, world["whole"])
    job_stats = ("records", "merged_spans", "valid_spans", "invalid_spans", "child_spans", "joined_links",
                 "missing_parent", "no_service", "ambiguous", "not_clustered")  # (not: the tile spills)
    whole = world["whole"]["stats"]
    assert set(ran["stats"]) == set(whole)
    for w, s in ran["stats"].items():
        assert {k: s[k] for k in job_stats} == {k: whole[w][k] for k in job_stats}, w
        assert s["ambiguous"] == 0 and s["not_clustered"] == 0


def test_windows_equal_the_oracle(ran, world):
    cols, names = world["cols"], world["names"]
    origin, W = ran["origin"], ran["W"]
    by_start = {r.start_time: r for r in ran["recs"]}
    seen = 0
    for w in range(W):
        sel = winref.window_records(cols, origin, HOUR, W, w)
        if not len(sel):
            assert w not in ran["stats"]
            continue
        assert ran["stats"][w]["records"] == len(sel)
        m0, ms = oracle.aggregate(cols.take(sel), S).dense()
        want = link_dict(links_from_table(LinkTable(S, m0, *ms, (m0 > 0).astype(np.uint8)), names))
        r = by_start.get(origin + w * HOUR)
        assert (r is None) == (not want)
        if r is not None:
            assert link_dict(r.links) == want, w
            seen += 1
    assert seen == len(ran["recs"]) >= 6


def test_the_big_trace_lies_in_one_window(ran, world):
    w = (BIG_T0 - world["whole"]["origin"]) // HOUR
    in_w = len(winref.window_records(world["cols"], world["whole"]["origin"], HOUR, world["whole"]["W"], w))
    assert in_w > 2000 and ran["stats"][w]["records"] == in_w


def test_windows_sum_to_the_plain_job(ran, world, gpu):
    plain = ZipkinAggregateJob(world["names"], device=gpu, order="rows", clock=lambda: 10**18)
    whole = link_dict(plain.run([world["cols"]], num_services=S).links)
    plain.close()
    total = {}
    for l in ran["agg"].getDependencies(ran["origin"], ran["origin"] + ran["W"] * HOUR).links:
        k = (l.parent.name, l.child.name)
        total[k] = l.duration_moments if k not in total else total[k].plus(l.duration_moments)
    assert set(total) == set(whole)
    for k, m in total.items():
        assert m.m0 == whole[k][0]
        assert moments_close(OMoments(*whole[k]), OMoments(*m)), k


def test_a_window_without_links_stores_nothing(ran):
    w = (LONE_AT - ran["origin"]) // HOUR
    assert ran["stats"][w]["records"] == 1 and ran["stats"][w]["joined_links"] == 0
    start = ran["origin"] + w * HOUR
    assert start not in [r.start_time for r in ran["recs"]] and w not in ran["hists"]
    assert ran["agg"].getDependencies(start, start + HOUR).links == ()


def test_an_unobserved_batch_is_refused(world, gpu, monkeypatch):
    """run() observes every batch itself; a partition that meets records the table does not hold (here:
    observe switched off) raises instead of filing them under the rest."""
    from zipkin_amd.windows import WindowPartition

    monkeypatch.setattr(WindowPartition, "observe", lambda self, cols, **kw: None)
    job = WindowedAggregateJob(world["names"], window_us=HOUR, device=gpu, order="rows")
    try:
        with pytest.raises(ValueError):
            job.run([world["cols"]], num_services=S)
    finally:
        job.close()


def test_default_order_still_refuses_a_recurring_trace(gpu):
    names = Dictionary([service_name(i) for i in range(S)])
    a = tracegen_host(403, 500, max_depth=6, num_services=S, base_ts=BASE_TS)
    b = tracegen_host(404, 500, max_depth=6, num_services=S, base_ts=BASE_TS)
    first = a.take(slice(0, int(winref.run_starts(a.trace_id)[1])))  # a's first trace again, in batch 2
    batches = [a, SpanColumns.concat([b, first])]
    job = WindowedAggregateJob(names, window_us=HOUR, device=gpu, verify=True)
    assert job.order == "whole"
    try:
        with pytest.raises(ZkError) as e:
            job.run(batches, num_services=S)
        assert e.value.status == _abi.ZK_ERR_NOT_CLUSTERED
    finally:
        job.close()
    # the same batches are what order="any" is for
    job = WindowedAggregateJob(names, window_us=HOUR, device=gpu, order="any")
    try:
        assert len(job.run(batches, num_services=S)) >= 7
    finally:
        job.close()
