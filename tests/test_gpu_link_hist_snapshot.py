"""Link-histogram snapshots on the GPU (include/zksketch.h zk_lh_snapshot / zk_lh_merge): the device
compaction and the device merge, held against the independent format reference tests/lhsnap.py.

Every synthetic state is written through merge(encode(dense)), so both kernels face the reference:
read() must equal `dense`, snapshot() must equal encode(dense) byte for byte, and the host quantiles of
that blob must equal quantiles_all on the handle for the present cells. Shapes: the chunk geometry of
every sub_bits (156 = 2 x 64 + 28, 592 = 9 x 64 + 16, 4352 = 68 x 64 bins), rows of 1 / 63 / 64 / 65 /
every / alternating bins, the tail of the four-waves-per-block grid (S = 3, 9, 61: cells % 4 = 1), a
table whose scan spans many blocks (S = 363), counts up to 2^32 - 1, the capacity rule, the refusals;
then states from real links (K1, the group join, the spill kernel's atomics) and the job / store
surface."""
import functools

import numpy as np
import pytest

from oracle.realtime import joined_links
from tests import lhsnap
from tests.bulkfrag import batches, encode, service_name
from tests.test_gpu_link_hist import expected_durations, expected_hist
from tests.test_gpu_parity import SERVER, cols_from_rows, star_trace
from zipkin_amd import DepsContext, SpanColumns, ZkError, _abi, tracegen_host
from zipkin_amd.realtime import LinkHistogram, LinkHistogramSnapshot

pytestmark = pytest.mark.gpu

U32 = 2**32 - 1
QS = (0.0, 0.5, 0.99, 1.0)


def check_state(lh, dense, dropped=0):
    """The handle holds exactly `dense`: read(), the snapshot's bytes, its size bound, its quantiles."""
    S, m = lh.num_services, lh.m
    want = lhsnap.encode(dense, S, m, dropped)
    assert np.array_equal(lh.read(), dense)
    blob = lh.snapshot()
    assert blob == want, f"{len(blob)} bytes, want {len(want)}"
    snap = LinkHistogramSnapshot(blob)
    links = int(dense.sum(dtype=np.uint64))
    assert (snap.links, snap.dropped, len(snap)) == (links, dropped, int(dense.any(axis=1).sum()))
    assert len(blob) <= 64 + 16 * len(snap) + 8 * min(links, dense.size)
    lo, hi, cnt = snap.quantiles(QS)
    LO, HI, CNT = lh.quantiles_all(QS)
    cells = snap.rows["parent"].astype(np.int64) * S + snap.rows["child"]
    assert np.array_equal(lo, LO[cells]) and np.array_equal(hi, HI[cells]) and np.array_equal(cnt, CNT[cells])
    assert np.count_nonzero(CNT) == len(cells)
    return snap


def put(lh, dense, dropped=0):
    lh.reset()
    lh.merge(lhsnap.encode(dense, lh.num_services, lh.m, dropped))


def random_rows(rng, dense, cells, max_entries=9, high=100_000):
    bins = dense.shape[1]
    for c in cells:
        b = rng.choice(bins, int(rng.integers(1, max_entries + 1)), replace=False)
        dense[c, b] = rng.integers(1, high, len(b))


@pytest.mark.parametrize("m", [2, 4, 7])
def test_chunk_geometry(gpu, m):
    S, bins = 3, lhsnap.nbins(m)
    assert bins == {2: 2 * 64 + 28, 4: 9 * 64 + 16, 7: 68 * 64}[m]
    d = np.zeros((S * S, bins), np.uint32)
    d[0, [0, 63, 64, 65, bins - 2, bins - 1]] = [1, 2, 3, 4, 5, 6]
    d[1] = 1 + np.arange(bins) % 7            # every bin
    d[2, 0::2] = 5                            # alternating bins
    d[4, 17] = 9                              # rows of 1, 63, 64 and 65 entries
    d[5, np.arange(63) * 2 + 1] = 1 + np.arange(63)
    d[6, 40:104] = 7
    d[7, bins - 65:] = 11
    d[8, bins - 1] = 3                        # the grid's tail wave (cell 8 = 4 * 2 + 0); cell 3 stays absent
    with LinkHistogram(S, sub_bits=m) as lh:
        put(lh, d, dropped=3)
        snap = check_state(lh, d, dropped=3)
        assert np.diff(np.r_[snap.rows["first"], len(snap.entries)]).tolist() == [6, bins, (bins + 1) // 2, 1, 63, 64, 65, 1]


@pytest.mark.parametrize("S", [9, 61])
def test_cell_geometry(gpu, S):
    cells = S * S
    assert cells % 4 == 1
    rng = np.random.default_rng(S)
    d = np.zeros((cells, lhsnap.nbins(4)), np.uint32)
    random_rows(rng, d, np.r_[0, cells - 1, rng.choice(np.arange(1, cells - 1), cells // 2, replace=False)])
    with LinkHistogram(S) as lh:
        put(lh, d)
        check_state(lh, d)


@pytest.fixture(scope="module")
def wide():
    """S = 363 at m = 2: 131,769 cells (% 4 = 1), an 82 MB table, so the scans span many blocks."""
    with LinkHistogram(363, sub_bits=2) as lh:
        yield lh


@pytest.mark.parametrize("pattern", ["first", "last", "every fourth", "run of 300", "none"])
def test_many_blocks(gpu, wide, pattern):
    S, cells = 363, 363 * 363
    present = {"first": [0], "last": [cells - 1], "every fourth": np.arange(1, cells, 4),
               "run of 300": np.arange(70_001, 70_301), "none": []}[pattern]
    d = np.zeros((cells, lhsnap.nbins(2)), np.uint32)
    random_rows(np.random.default_rng(len(present)), d, present, max_entries=5, high=1000)  # (links < 2^32)
    put(wide, d)
    snap = check_state(wide, d)
    if pattern == "none":
        assert len(snap.blob) == 64 and len(snap) == 0


def test_counts_and_capacity(gpu):
    S, m = 3, 4
    bins = lhsnap.nbins(m)
    one_record = cols_from_rows([(1, 10, 0, 1, 50, 0, SERVER)])
    with DepsContext(S) as ctx, LinkHistogram(S) as lh:
        a = np.zeros((S * S, bins), np.uint32)
        a[0, 5], a[4, 500], a[4, 501] = 1, 2**31, 7
        put(lh, a)
        check_state(lh, a)
        # a merge into rows that already hold counts: shared and new bins, shared and new rows
        b = np.zeros_like(a)
        b[4, [499, 500]], b[8, bins - 1], b[0, 5] = [3, 2**31 - 100], 2, 9
        assert int(a.sum(dtype=np.uint64) + b.sum(dtype=np.uint64)) == U32 - 77
        lh.merge(lhsnap.encode(b, S, m, dropped=2))
        check_state(lh, a + b, dropped=2)
        # a single entry of 2^32 - 1 on a fresh handle: links = reserved = 2^32 - 1
        full = np.zeros_like(a)
        full[7, 300] = U32
        put(lh, full)
        check_state(lh, full)
        # from here every merge with links >= 1 is refused, and so is a bound accumulate of one record
        unit = np.zeros_like(a)
        unit[2, 0] = 1
        with pytest.raises(ZkError) as e:
            lh.merge(lhsnap.encode(unit, S, m))
        assert e.value.status == _abi.ZK_ERR_CAPACITY
        lh.bind(ctx)
        with pytest.raises(ZkError) as e:
            ctx.accumulate(one_record, clustered=True)
        assert e.value.status == _abi.ZK_ERR_CAPACITY
        lh.merge(lhsnap.encode(np.zeros_like(a), S, m, dropped=4))  # no link: nothing to refuse
        check_state(lh, full, dropped=4)
        lh.unbind()


def test_capacity_counts_what_was_merged_before(gpu):
    S, m = 3, 4
    d = np.zeros((S * S, lhsnap.nbins(m)), np.uint32)
    d[1, 1] = U32 - 5
    five, six = np.zeros_like(d), np.zeros_like(d)
    five[2, 2], six[2, 2] = 5, 6
    with LinkHistogram(S) as lh:
        put(lh, d)
        with pytest.raises(ZkError) as e:
            lh.merge(lhsnap.encode(six, S, m))  # reserved + links = 2^32
        assert e.value.status == _abi.ZK_ERR_CAPACITY
        check_state(lh, d)
        lh.merge(lhsnap.encode(five, S, m))     # reserved = 2^32 - 1 exactly
        check_state(lh, d + five)


def test_refusals_leave_the_table_unchanged(gpu):
    S, m = 5, 4
    rng = np.random.default_rng(5)
    d = np.zeros((S * S, lhsnap.nbins(m)), np.uint32)
    random_rows(rng, d, [0, 7, 24])
    good = lhsnap.encode(d, S, m)
    other_m = np.zeros((S * S, lhsnap.nbins(2)), np.uint32)
    other_m[3, 3] = 1
    wide_ids = LinkHistogramSnapshot(good).remap([0, 1, 2, 3, S]).blob  # a row with child (and parent) = S
    corrupt = bytearray(good)
    corrupt[-8] ^= 1  # the last count changed: links no longer the sum (or the count is 0)
    with LinkHistogram(S) as lh:
        put(lh, d)
        for blob, status in ((lhsnap.encode(other_m, S, 2), _abi.ZK_ERR_INVALID_ARG),
                             (wide_ids, _abi.ZK_ERR_SERVICE_RANGE),
                             (bytes(corrupt), _abi.ZK_ERR_INVALID_ARG),
                             (good[:-8], _abi.ZK_ERR_INVALID_ARG),
                             (b"", _abi.ZK_ERR_INVALID_ARG)):
            with pytest.raises(ZkError) as e:
                lh.merge(blob)
            assert e.value.status == status
            check_state(lh, d)
        lh.merge(good)  # (and a good one still goes in)
        check_state(lh, d + d)


@functools.lru_cache(maxsize=None)
def real_batches():
    """(A, B, the dropped child) at S = 61: A clustered with a trace of 1025 records (the spill
    kernel), B the fragments of other traces in any order; computed once, never changed."""
    S = 61
    a = SpanColumns.concat([tracegen_host(201, 3000, max_depth=6, num_services=S),
                            cols_from_rows(star_trace(7777, 512, nsvc=S)),
                            tracegen_host(202, 500, max_depth=5, num_services=S)])
    b = tracegen_host(203, 3000, max_depth=6, num_services=S)
    b = b.take(np.random.default_rng(203).permutation(len(b)))
    tid = 2**62 + 5
    long_child = cols_from_rows([(tid, 10, 0, 1, 2**41, 3, SERVER), (tid, 11, 10, 5, 5 + 2**40, 4, SERVER | 1)])
    return a, b, long_child


def test_snapshots_of_real_links_merge_to_the_state_of_both(gpu):
    S = 61
    a, b, long_child = real_batches()
    with DepsContext(S) as c1, DepsContext(S) as c2, DepsContext(S) as c3, LinkHistogram(S) as h1, \
            LinkHistogram(S) as h2, LinkHistogram(S) as h3, LinkHistogram(S) as fresh:
        h1.bind(c1)
        c1.accumulate(a, clustered=True, verify=True)
        m0_a = c1.finalize().m0.copy()
        assert c1.stats()["spilled_traces"] >= 1
        want_a = expected_hist(joined_links(a, S), S, 4)
        sa = check_state(h1, want_a)
        h2.bind(c2)
        c2.accumulate(b, clustered=False, verify=False)
        c2.accumulate(long_child, clustered=True)
        want_b = expected_hist(joined_links(b, S), S, 4)
        sb = check_state(h2, want_b, dropped=1)  # the child of 2^40 us: in no bin, carried as `dropped`
        h3.bind(c3)
        for part in (a, b, long_child):
            c3.accumulate(part, clustered=part is not b, verify=part is not b)
        c3.sync()
        both = h3.read()
        assert np.array_equal(both, want_a + want_b) and h3.dropped() == 1
        fresh.merge(sa)
        fresh.merge(sb.blob)
        check_state(fresh, both, dropped=1)
        total = sa.plus(sb)
        assert total.blob == fresh.snapshot() == sb.plus(sa).blob
        # every row's count is the finalized table's m0 of its cell
        with DepsContext(S) as plain:
            plain.accumulate(b, clustered=False, verify=False)
            m0_b = plain.finalize().m0.copy()
        for snap, m0 in ((sa, m0_a), (total, m0_a + m0_b)):
            cells = snap.rows["parent"].astype(np.int64) * S + snap.rows["child"]
            assert np.array_equal(snap.quantiles(())[2], m0[cells]) and len(cells) == np.count_nonzero(m0)


def test_incremental_runs_store_snapshots_a_window_sums(gpu):
    from zipkin_amd.aggregates import Dictionary, GpuAggregates, ZipkinAggregateJob
    from zipkin_amd.incremental import IncrementalAggregator

    S, qs = 61, (0.5, 0.99)
    names = Dictionary([service_name(i) for i in range(S)])
    agg = GpuAggregates("anorm", services=names, clock=lambda: 10**15)
    job = ZipkinAggregateJob(names, clock=lambda: 10**15, link_quantiles=qs)
    inc = IncrementalAggregator(agg, job=job)
    runs = [tracegen_host(301, 2500, max_depth=6, num_services=S), tracegen_host(302, 2500, max_depth=6, num_services=S)]
    # every trace of a run created at one instant: the run's record is (t, t) and holds all of them
    for t, cols in zip((1000, 2000), runs):
        rec = inc.apply(cols, np.full(len(cols), t, np.int64), num_services=S)
        assert (rec.start_time, rec.end_time) == (t, t) and inc.last_selected == len(cols)
    job.close()
    assert agg.count() == 2

    def as_dict(durations):
        return {(x.parent, x.child): (x.count, x.quantiles) for x in durations}

    both = SpanColumns.concat(runs)
    got = agg.getLinkDurations(1000, 2000, qs)
    assert as_dict(got) == expected_durations(joined_links(both, S), S, 4, qs)
    m0 = {}
    for l in agg.getDependencies(1000, 2000).links:
        m0[(l.parent.name, l.child.name)] = m0.get((l.parent.name, l.child.name), 0) + l.duration_moments.m0
    assert {(x.parent, x.child): x.count for x in got} == m0
    assert agg.getLinkHistogram(1000, 2000)[1:] == (2, 2)
    # a window that holds only the first record
    assert as_dict(agg.getLinkDurations(1000, 1999, qs)) == expected_durations(joined_links(runs[0], S), S, 4, qs)
    assert agg.getLinkHistogram(1000, 1999)[1:] == (1, 1)
    assert agg.getLinkDurations(2001, 3000, qs) == []


def test_stored_span_drivers_store_equal_snapshots(gpu):
    import torch

    from zipkin_amd.aggregates import Dictionary, GpuAggregates, StoredSpanJob

    S, qs = 61, (0.5, 0.99)
    small = tracegen_host(88, 3_000, max_depth=6, num_services=S)
    buf, off, exp = encode(small)
    cuts = [len(small) // 3]
    dev = [(torch.from_numpy(b).cuda(), torch.from_numpy(o.view(np.int64)).cuda(), len(o) - 1)
           for b, o in batches(buf, off, cuts)]
    stores = [GpuAggregates("anorm", services=Dictionary([service_name(i) for i in range(S)]), clock=lambda: 10**15)
              for _ in range(3)]
    djob = StoredSpanJob(clock=lambda: 10**15, max_services=S, link_quantiles=qs, aggregates=stores[0])
    hjob = StoredSpanJob(clock=lambda: 10**15, max_services=S, link_quantiles=qs, aggregates=stores[1])
    plain = StoredSpanJob(clock=lambda: 10**15, max_services=S, aggregates=stores[2])
    ddeps = djob.run_device(dev, indexer=False)
    hdeps = hjob.run(batches(buf, off, cuts))
    plain.run_device(dev, indexer=False)
    snaps = [s.getLinkHistogram(0, 10**15) for s in stores]
    assert snaps[0][1:] == snaps[1][1:] == (1, 1) and snaps[2][1:] == (1, 0)
    assert snaps[0][0].blob == snaps[1][0].blob and len(snaps[0][0]) == len(ddeps.links) == len(hdeps.links)
    assert len(snaps[2][0]) == 0
    want = expected_durations(joined_links(exp, S), S, 4, qs)
    for s in stores[:2]:
        assert {(x.parent, x.child): (x.count, x.quantiles) for x in s.getLinkDurations(0, 10**15, qs)} == want
    for j in (djob, hjob, plain):
        j.close()
