"""The exact-sum kernels at the bounds of their domain, against tests/exactref.py (Python integers and
Fractions; independent of the library and of the C oracle).

Every other device test takes its durations from TraceGen (< 2^19 us). Here every cell's content is a
chosen multiset of durations up to the largest accepted (2^40 - 1 us), placed by star traces (a root
server span per trace, child spans below it), so the expected power sums and moments cost nothing
and are exact. Reached that way (zipkin_amd/csrc):
  * every link reducer -- k_bucket_lds_reduce_wide<9> with atomic and with owner flushes (its
    d >= 2^21 rows, the 128-bit rebuild at the flush, its second sub-part), k_bucket_reduce<10>
    (RunSums::add above 2^32) and k_link_reduce_atomic (limb_value above bit 32) -- at the smallest S
    that selects each (bucket_geometry, launch_partitioned_reduce in zk_reduce.hip);
  * every place that computes d = last - first and packs (cell << 40) | d -- the streaming K1, the
    spill kernel, the group join, the trace pass, a trace held back over a batch edge -- with the
    same durations, and beside each a child of exactly 2^40 us, which must be counted and dropped.
Asserted everywhere: the caller-owned table decodes to the exact sums, finalize equals the Fractions
bit for bit, the counters are right; for S <= 725 the C oracle is checked against the same data."""
import numpy as np
import pytest

from oracle import oracle
from tests import exactref
from tests.exactref import DMAX, EDGE_DURATIONS
from tests.test_gpu_parity import CLIENT, SERVER, assert_parity
from tests.test_gpu_sharded import Shard
from zipkin_amd import SpanColumns, ZkError, _abi, table

pytestmark = pytest.mark.gpu

T0 = 1_000_000
ROOT_SID = 1
GOLD = 0x9E3779B97F4A7C15


def star_batch(root_svc, counts, child_svc, d, fragments=1, tid0=0):
    """Clustered star traces: trace t is a root server span of service root_svc[t] followed by
    counts[t] child spans (the next counts[t] entries of child_svc and d). A child is one server
    fragment [first, first + d], or (fragments = 2) a client fragment that supplies `first` and a
    server fragment that supplies `last`, so that d exists only after the merge."""
    root_svc = np.asarray(root_svc, np.uint32)
    counts = np.asarray(counts, np.int64)
    child_svc = np.asarray(child_svc, np.uint32)
    d = np.asarray(d, np.int64)
    T, n = len(root_svc), int(counts.sum())
    assert len(child_svc) == n and len(d) == n
    tids = (np.arange(T, dtype=np.uint64) + np.uint64(tid0 + 1)) * np.uint64(GOLD)  # odd multiplier: distinct
    tr = np.repeat(np.arange(T), counts)
    j = np.arange(n) - np.repeat(np.cumsum(counts) - counts, counts)
    first = T0 + 5 + j
    width = int(counts.max(initial=0)) * fragments + 1

    def rows(trace, rank, sid, pid, fst, lst, svc, flags):
        return (trace * width + rank, tids[trace], sid, pid, fst, lst, svc, np.full(len(trace), flags, np.uint32))

    parts = [rows(np.arange(T), np.zeros(T, np.int64), np.full(T, ROOT_SID), np.zeros(T, np.int64),
                  np.full(T, T0), np.full(T, T0 + 10), root_svc, SERVER)]
    pid = np.full(n, ROOT_SID)
    if fragments == 1:
        parts.append(rows(tr, 1 + j, 2 + j, pid, first, first + d, child_svc, SERVER | 1))
    else:
        parts.append(rows(tr, 1 + 2 * j, 2 + j, pid, first, first, child_svc, CLIENT | 1))
        parts.append(rows(tr, 2 + 2 * j, 2 + j, pid, first + d, first + d, child_svc, SERVER | 1))
    order = np.argsort(np.concatenate([p[0] for p in parts]), kind="stable")
    cols = SpanColumns.empty(len(order))
    for i, k in enumerate(("trace_id", "span_id", "parent_id", "first_ts", "last_ts", "service_id", "flags")):
        col = getattr(cols, k)
        col[:] = np.concatenate([np.asarray(p[i + 1]).astype(col.dtype) for p in parts])[order]
    return cols


def traces_of(cells, rng, per_trace=255):
    """Star traces realising {(parent, child): [durations]}: the children of one parent service are
    shuffled together and cut into traces of <= per_trace children (<= 256 records)."""
    root_svc, counts, child_svc, ds = [], [], [], []
    for p in sorted({p for p, _ in cells}):
        svc = np.concatenate([np.full(len(v), c, np.uint32) for (pp, c), v in cells.items() if pp == p])
        d = np.concatenate([np.asarray(v, np.int64) for (pp, c), v in cells.items() if pp == p])
        perm = rng.permutation(len(d))
        svc, d = svc[perm], d[perm]
        for a in range(0, len(d), per_trace):
            root_svc.append(p)
            counts.append(min(per_trace, len(d) - a))
        child_svc.append(svc)
        ds.append(d)
    return root_svc, counts, np.concatenate(child_svc), np.concatenate(ds)


def random_durations(rng, n, classes=(21, 32, 40)):
    """n seeded durations, drawn in turn from the magnitude classes < 2^21, < 2^32, < 2^40."""
    return [int(rng.integers(0, 1 << classes[i % len(classes)])) for i in range(n)]


def mixed(rng, n):
    """Narrow and wide durations in one cell: every edge duration, then random ones of every class."""
    reps = list(EDGE_DURATIONS) * 3
    return reps + random_durations(rng, n - len(reps))


def wide(rng, n):
    return [(1 << 21) + int(rng.integers(0, (1 << 40) - (1 << 21))) for _ in range(n)]


def run_and_check(batches, S, cells, *, over_range=0, ctx_kw=None, acc_kw=None, check_oracle=True):
    """Accumulate `batches` (SpanColumns, or (SpanColumns, accumulate keywords)) into a caller-owned
    table and compare with the exact reference of `cells` = {(parent, child): [durations]}.
    over_range: children of >= 2^40 us among the batches (counted, dropped, finalize refuses)."""
    want = {k: exactref.multiset(v) for k, v in cells.items()}
    links = sum(len(v) for v in cells.values())
    sh = Shard(S, **(ctx_kw or {}))
    try:
        for b in batches:
            b, kw = b if isinstance(b, tuple) else (b, acc_kw or {"clustered": True})
            sh.ctx.accumulate(b, **kw)
        if over_range:
            with pytest.raises(ZkError) as e:
                sh.ctx.finalize()
            assert e.value.status == _abi.ZK_ERR_DURATION_RANGE
            got = None
        else:
            got = sh.ctx.finalize()
        st = sh.ctx.stats()
        sh.ctx.sync()
        acc = sh.table.cpu().numpy()
    finally:
        sh.close()
    assert table.decode(acc, S) == {k: exactref.power_sums(m) for k, m in want.items()}
    assert st["joined_links"] == links + over_range and st["duration_range"] == over_range
    assert st["records"] == sum(len(b[0] if isinstance(b, tuple) else b) for b in batches)
    assert st["missing_parent"] == 0 and st["no_service"] == 0 and st["ambiguous"] == 0 and st["not_clustered"] == 0
    if got is not None:
        exactref.assert_moments(got, want, S)
        if check_oracle and S <= 725:
            whole = SpanColumns.concat([b[0] if isinstance(b, tuple) else b for b in batches])
            assert_parity(got, st, oracle.aggregate(whole, S))
    return st


# ---- reducers ---------------------------------------------------------------------------------
def reducer_cells(S, rng):
    """Busy cells (thousands of links each, so every limb carries) in the first and in the last cell
    bucket: narrow only, mixed, only 2^40 - 1, wide only; the last cell S * S - 1 among them."""
    P = S - 1
    return {
        (0, 0): [0, 1, (1 << 21) - 1] * 5 + random_durations(rng, 2500, classes=(21,)),
        (0, 1): mixed(rng, 4000),
        (0, 2): [DMAX] * 3000,
        (P, 0): wide(rng, 2500),
        (P, P - 1): [DMAX] * 2100,
        (P, P): mixed(rng, 3000),
    }


@pytest.mark.parametrize("S", [23, 363, 725, 1025])
def test_reducers_at_duration_bounds(gpu, S):
    """S = 23: k_bucket_lds_reduce_wide<9>, 2 buckets, splits = 256 (atomic flush adds); 363: the same
    kernel, 258 buckets, splits = 1 (owner stores); 725: k_bucket_reduce<10>, 514 buckets;
    1025: k_link_reduce_atomic (no buckets)."""
    rng = np.random.default_rng(S)
    cells = reducer_cells(S, rng)
    cols = star_batch(*traces_of(cells, rng))
    assert np.unique(cols.trace_id, return_counts=True)[1].max() <= 256  # records of a trace
    run_and_check([cols], S, cells)


def test_wide_reducer_second_subpart(gpu):
    """2^20 + 3 links in ONE bucket at S = 363 (splits = 1): the smallest input at which the wide
    kernel's sub-part loop (kSub = 2^20 links) runs a second time, adding a second flush to cells
    that already hold the first. Cells below 512: one holds only 2^40 - 1, one wide durations, one
    narrow and wide mixed (drawn from small pools, so the expected sums come from the multisets)."""
    S, total = 363, (1 << 20) + 3
    rng = np.random.default_rng(363_363)
    pools = {(0, 5): [DMAX],
             (0, 200): wide(rng, 61),
             (1, 148): list(EDGE_DURATIONS) + random_durations(rng, 54)}  # cell 511
    sizes = {(0, 5): 350_000, (0, 200): 350_000}
    sizes[(1, 148)] = total - sum(sizes.values())
    cells = {k: np.asarray(pools[k], np.int64)[rng.integers(0, len(pools[k]), sizes[k])] for k in pools}
    assert all(p * S + c < 512 for p, c in cells)
    cols = star_batch(*traces_of(cells, rng))
    assert sum(len(v) for v in cells.values()) == total
    run_and_check([cols], S, cells)


# ---- link emitters ------------------------------------------------------------------------------
ES = 23  # every emitter case: the wide reducer with atomic flushes behind it


def emitter_cells(rng, n_mixed=90):
    return {(0, 1): mixed(rng, n_mixed), (0, 2): [DMAX] * 40, (22, 22): mixed(rng, n_mixed), (22, 0): wide(rng, 30)}


def with_over_range(root_svc, counts, child_svc, d, at_trace):
    """One more child, of exactly 2^40 us, at the end of trace `at_trace`."""
    pos = int(np.sum(counts[: at_trace + 1]))
    counts = list(counts)
    counts[at_trace] += 1
    return root_svc, counts, np.insert(child_svc, pos, 3), np.insert(d, pos, DMAX + 1)


@pytest.mark.parametrize("over_range", [0, 1])
def test_streaming_join_merges_the_duration_from_two_fragments(gpu, over_range):
    rng = np.random.default_rng(1)
    cells = emitter_cells(rng)
    tr = traces_of(cells, rng, per_trace=40)
    if over_range:
        tr = with_over_range(*tr, at_trace=1)
    run_and_check([star_batch(*tr, fragments=2)], ES, cells, over_range=over_range)


@pytest.mark.parametrize("over_range", [0, 1])
def test_spill_kernel_at_duration_bounds(gpu, over_range):
    """One trace of 1025 records and one of 2049 (longer than a K1 tile: the spill kernel), between
    ordinary traces."""
    rng = np.random.default_rng(2)
    small = emitter_cells(rng)
    a, b = traces_of(small, rng, per_trace=60), None
    big = {(5, 6): mixed(rng, 1024), (7, 8): mixed(rng, 1000) + [DMAX] * 1048}
    b = traces_of(big, rng, per_trace=4096)
    assert list(b[1]) == [1024, 2048]
    half = len(a[0]) // 2  # the giant traces between the small ones
    root_svc = a[0][:half] + b[0] + a[0][half:]
    counts = a[1][:half] + b[1] + a[1][half:]
    na = int(np.sum(a[1][:half]))
    child_svc = np.concatenate([a[2][:na], b[2], a[2][na:]])
    d = np.concatenate([a[3][:na], b[3], a[3][na:]])
    tr = (root_svc, counts, child_svc, d)
    if over_range:
        tr = with_over_range(*tr, at_trace=half + 1)  # inside the 2049-record trace
    st = run_and_check([star_batch(*tr)], ES, {**small, **big}, over_range=over_range)
    assert st["spilled_traces"] >= 1


_UNCLUSTERED = {}


def unclustered_batch(over_range):
    """Just over 2^18 records of 16-record traces, shuffled: durations and cells drawn from small
    pools (every edge duration among them), so the multisets are counted, not summed."""
    if over_range not in _UNCLUSTERED:
        rng = np.random.default_rng(3)
        T, K = (1 << 14) + 3, 15
        pool = np.asarray(list(EDGE_DURATIONS) + random_durations(rng, 30), np.int64)
        root_svc = rng.choice(np.array([0, 7, 22]), T)
        child_svc = rng.choice(np.array([0, 1, 22]), T * K)
        child_svc[np.repeat(root_svc, K) == 7] = 9  # cell (7, 9) holds only 2^40 - 1
        d = pool[rng.integers(0, len(pool), T * K)]
        d[child_svc == 9] = DMAX
        parents = np.repeat(root_svc, K)
        cells = {(p, c): d[(parents == p) & (child_svc == c)] for p in (0, 7, 22) for c in (0, 1, 9, 22)}
        cells = {k: v for k, v in cells.items() if len(v)}
        assert set(cells[(7, 9)].tolist()) == {DMAX} and len(cells) == 7
        tr = (list(root_svc), [K] * T, child_svc, d)
        if over_range:
            tr = with_over_range(*tr, at_trace=T // 2)
        cols = star_batch(*tr)
        assert len(cols) > 1 << 18
        _UNCLUSTERED[over_range] = (cols.take(rng.permutation(len(cols))), cells)
    return _UNCLUSTERED[over_range]


@pytest.mark.parametrize("over_range", [0, 1])
@pytest.mark.parametrize("trace_pass", [False, True])
def test_unclustered_batch_at_duration_bounds(gpu, trace_pass, over_range):
    """trace_pass False: the group join (k_group_join: an unverified batch of > 2^18 records);
    True: the clustering pass, then the streaming K1."""
    cols, cells = unclustered_batch(over_range)
    run_and_check([cols], ES, cells, over_range=over_range, ctx_kw={"trace_pass": trace_pass},
                  acc_kw={"clustered": False, "verify": False}, check_oracle=not trace_pass)


@pytest.mark.parametrize("over_range", [0, 1])
def test_held_back_trace_at_duration_bounds(gpu, over_range):
    """ZK_BATCH_CONTINUES: the batch edge falls inside the last trace, between the client and the
    server fragment of one child; the children of 2^40 - 1 us (and of 2^40) lie behind the edge."""
    rng = np.random.default_rng(4)
    cells = emitter_cells(rng)
    h = ([4], [6], np.array([1, 1, 2, 1, 2, 1], np.uint32), np.array([5, 1 << 21, DMAX, DMAX, DMAX - 1, 1 << 32], np.int64))
    held = {(4, 1): [5, 1 << 21, DMAX, 1 << 32], (4, 2): [DMAX, DMAX - 1]}
    a = traces_of(cells, rng, per_trace=50)
    k = len(a[0]) // 2
    na = int(np.sum(a[1][:k]))
    first = (a[0][:k] + h[0], a[1][:k] + h[1], np.concatenate([a[2][:na], h[2]]), np.concatenate([a[3][:na], h[3]]))
    if over_range:
        first = with_over_range(*first, at_trace=k)
    b1 = star_batch(*first, fragments=2)
    b2 = star_batch(a[0][k:], a[1][k:], a[2][na:], a[3][na:], fragments=2, tid0=10_000)
    held_len = 1 + 2 * (len(h[2]) + over_range)
    edge = len(b1) - held_len + 4  # the root, one whole child, the next child's client fragment
    far = b1.take(slice(edge, len(b1)))
    # the cut child's server fragment leads the far side
    assert far.trace_id[0] == b1.trace_id[edge - 1] and far.span_id[0] == b1.span_id[edge - 1]
    assert far.last_ts[0] - b1.first_ts[edge - 1] == 1 << 21
    batches = [(b1.take(slice(0, edge)), {"clustered": True, "continues": True}),
               (SpanColumns.concat([far, b2]), {"clustered": True})]
    run_and_check(batches, ES, {**cells, **held}, over_range=over_range)
