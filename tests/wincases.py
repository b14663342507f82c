"""Inputs of the window-partition tests (tests/test_windows_host.py, tests/test_gpu_windows.py): small
trace-clustered batches aimed at the edges of the kernels' geometry (zk_win_plan) and of the window
rule. A case is (name, cols, origin, window, W, hold_last).

Every record's span_id is its index in the batch and its other columns are functions of that index,
so a moved record is recognised in all seven columns."""
import functools

import numpy as np

from zipkin_amd import SpanColumns
from zipkin_amd.windows import plan

HOUR = 3_600_000_000
T0 = 1_400_000_000_000_000 // HOUR * HOUR
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
TIMED = 1 << 1  # ZK_F_HAS_ANNOTATIONS
I64_EDGES = (INT64_MIN, -1, 0, 1, INT64_MAX)
WINDOWS = (1, HOUR, INT64_MAX)
WS = (1, 1024)


def build(runs) -> SpanColumns:
    """runs: [(trace_id, [(first_ts, timed), ...])] -> a batch with the runs back to back."""
    return fill(np.repeat(np.array([r[0] for r in runs], np.uint64), [len(r[1]) for r in runs]),
                np.array([t for r in runs for t, _ in r[1]], np.int64),
                np.array([bool(f) for r in runs for _, f in r[1]], bool))


def fill(trace_id, ts, timed) -> SpanColumns:
    """A batch from per-record trace ids, times and timed bits; the other columns from the index."""
    n = len(trace_id)
    c = SpanColumns.empty(n)
    idx = np.arange(n, dtype=np.uint64)
    c.trace_id[:] = trace_id
    c.span_id[:] = idx
    c.parent_id[:] = idx * np.uint64(0x9E3779B97F4A7C15)
    c.first_ts[:] = ts
    c.last_ts[:] = (idx * np.uint64(7919)).view(np.int64)
    c.service_id[:] = (idx % np.uint64(61)).astype(np.uint32)
    # the fragment's other flag bits vary too (has-parent, counts, a name id)
    c.flags[:] = ((idx.astype(np.uint32) * np.uint32(2654435761)) & np.uint32(0xFFFF_FF0D)) | (
        timed.astype(np.uint32) * np.uint32(TIMED))
    return c


class Ids:
    """Distinct pseudo-random trace ids."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.seen = set()

    def __call__(self) -> int:
        while True:
            v = int(self.rng.integers(0, 2 ** 64, dtype=np.uint64))
            if v not in self.seen and v not in (0, 2 ** 64 - 1):
                self.seen.add(v)
                return v


def random_run(rng, length, origin=T0, window=HOUR, W=8):
    """A run of `length` fragments: mostly timed inside the W windows; some before, after, untimed.
    Untimed fragments carry INT64_MIN, which must never win the minimum."""
    kind = rng.integers(0, 20)
    base = origin + int(rng.integers(0, W * window))
    if kind == 0:
        base = origin - 1 - int(rng.integers(0, window))
    elif kind == 1:
        base = origin + W * window + int(rng.integers(0, window))
    recs = []
    for _ in range(length):
        timed = kind != 2 and rng.integers(0, 4) != 0
        recs.append((base + int(rng.integers(0, 1000)), True) if timed else (INT64_MIN, False))
    return recs


def random_runs(seed, n, ids=None, **kw):
    """Runs of 1-40 records with seeded random times, n records in all."""
    rng = np.random.default_rng(seed)
    ids = ids or Ids(seed)
    runs, left = [], n
    while left:
        k = min(left, int(rng.integers(1, 41)))
        runs.append((ids(), random_run(rng, k, **kw)))
        left -= k
    return runs


def special_run(length, where, t):
    """A run whose only timed fragment (time t) is its first / last / a middle record, or none; the
    untimed fragments carry INT64_MIN."""
    recs = [(INT64_MIN, False)] * length
    pos = {"first": 0, "last": length - 1, "middle": length // 2, "none": None}[where]
    if pos is not None:
        recs[pos] = (t, True)
    return recs


def with_specials(seed, n, specials):
    """n records: random runs around the given (start, length, where) special runs, which get times in
    distinct windows."""
    ids = Ids(seed)
    runs, at = [], 0
    for k, (start, length, where) in enumerate(sorted(specials)):
        assert start >= at and start + length <= n
        if start > at:
            runs += random_runs(seed + 1 + k, start - at, ids)
        runs.append((ids(), special_run(length, where, T0 + (2 + 3 * k) % 8 * HOUR + 5)))
        at = start + length
    if at < n:
        runs += random_runs(seed + 99, n - at, ids)
    return runs


@functools.lru_cache(maxsize=None)
def smallest_n_with_ranges(k: int) -> int:
    n = 1
    while plan(n)[2] < k:
        n += 1
    return n


SHAPE_LABELS = ("1", "2", "c-1", "c", "c+1", "n3", "n3+5")  # c: records per chunk, n3: the first n with 3 ranges
WHERES = ("first", "last", "middle", "none")
EDGE_GEOS = ("meets_edge", "crosses_edge", "covers_two", "covers_two_longer", "whole_batch")


def shape_cases():
    c = plan(1)[0]
    n3 = smallest_n_with_ranges(3)
    out = []
    for label, n in zip(SHAPE_LABELS, (1, 2, c - 1, c, c + 1, n3, n3 + 5)):
        out.append((f"shape_{label}", build(random_runs(n, n)), T0, HOUR, 8, False))
    return out


def edge_cases():
    """At the smallest n with >= 4 ranges: runs that meet, cross and cover range edges, each crossed with
    where its timed fragment lies."""
    n = smallest_n_with_ranges(4)
    rr = plan(n)[1]
    out = []
    for where in WHERES:
        geo = {
            "meets_edge": [(rr - 20, 20, where), (rr, 30, where)],
            "crosses_edge": [(rr - 10, 25, where)],
            "covers_two": [(rr - 7, 2 * rr + 7 + (n - 3 * rr + 1) // 2, where)],
            "covers_two_longer": [(rr - 7, 2 * rr + 16, where)],
            "whole_batch": [(0, n, where)],
        }
        for name, sp in geo.items():
            m = n + 40 if name == "covers_two_longer" else n
            out.append((f"{name}_{where}", build(with_specials(17, m, sp)), T0, HOUR, 8, False))
    return out


def id_cases():
    ids = Ids(5)
    a, b = ids(), ids()
    t = lambda w: T0 + w * HOUR + 9  # noqa: E731
    extremes = [(0, [(t(1), True)] * 3), (2 ** 64 - 1, [(t(2), True)] * 2), (0, [(t(3), True)]),
                (2 ** 64 - 1, [(INT64_MIN, False)]), (1, [(t(0), True)])]
    repeated = [(a, [(t(1), True), (t(1) + 1, True)]), (b, [(t(5), True)]), (a, [(t(6), True)] * 3),
                (b, [(INT64_MIN, False)] * 2)]
    garbage = [(ids(), [(INT64_MIN, False), (t(4), True), (INT64_MIN, False)]),
               (ids(), [(t(2), True), (INT64_MIN, False), (t(2) - HOUR, True)]),
               (ids(), [(INT64_MIN, False)] * 70 + [(t(7), True)] + [(INT64_MIN, False)] * 70)]
    return [("ids_0_and_max", build(extremes), T0, HOUR, 8, False),
            ("ids_repeated_not_adjacent", build(repeated), T0, HOUR, 8, False),
            ("untimed_int64_min_inside_timed_runs", build(garbage), T0, HOUR, 8, False)]


def rule_times(origin, window, W):
    """The boundary trace times of the window rule, within int64."""
    end = origin + W * window
    ts = set(I64_EDGES) | {origin - 1, origin, end - 1, end}
    return sorted(x for x in ts if INT64_MIN <= x <= INT64_MAX)


def rule_cases():
    """Every boundary time as a run of its own (two fragments: the time and a later one), for every
    origin x window x W of the lists above."""
    out = []
    for origin in I64_EDGES:
        for window in WINDOWS:
            for W in WS:
                ids = Ids(3)
                runs = [(ids(), [(min(t + 1, INT64_MAX), True), (t, True)]) for t in rule_times(origin, window, W)]
                out.append((f"rule_o{origin}_w{window}_W{W}", build(runs), origin, window, W, False))
    return out


def window_cases():
    ids = Ids(11)
    rng = np.random.default_rng(11)
    rr_runs = [(ids(), [(T0 + (k % 1024) * HOUR + 3, True)] * int(rng.integers(1, 4))) for k in range(3 * 1024)]
    one = [(ids(), [(T0 + int(rng.integers(0, 8 * HOUR)), True)] * int(rng.integers(1, 41))) for _ in range(150)]
    return [("W1", build(random_runs(21, 2500)), T0 + 3 * HOUR, HOUR, 1, False),
            ("W1024_round_robin", build(rr_runs), T0, HOUR, 1024, False),
            ("all_in_one_window", build(one), T0 - 2 * HOUR, 16 * HOUR, 3, False),
            ("all_in_the_rest", build(random_runs(25, 2500)), T0 + 100 * HOUR, HOUR, 8, False)]


def hold_cases():
    c = plan(1)[0]
    n = smallest_n_with_ranges(4)
    rr = plan(n)[1]
    return [("hold_last_run_of_1", build(with_specials(31, n, [(n - 1, 1, "first")])), T0, HOUR, 8, True),
            ("hold_last_run_crosses_range", build(with_specials(32, 2 * c + 10, [(2 * c - 5, 15, "last")])), T0, HOUR, 8, True),
            ("hold_last_run_crosses_two_ranges", build(with_specials(33, n, [(rr - 9, n - rr + 9, "middle")])), T0, HOUR, 8, True),
            ("hold_whole_batch_one_run", build(with_specials(34, n, [(0, n, "first")])), T0, HOUR, 8, True)]


def big_batch(seed, n, specials) -> SpanColumns:
    """n records built with numpy alone (for batches of millions): random runs of 1-40 records as
    random_run makes them, then the (start, length, where) special runs laid over them, each with its
    only timed fragment where `where` says and a time in a window of its own turn."""
    rng = np.random.default_rng(seed)
    start = np.zeros(n, bool)
    at = np.cumsum(rng.integers(1, 41, size=n // 8 + 8))
    start[0] = True
    start[at[at < n]] = True
    for a, k, _ in specials:
        assert 0 <= a and a + k <= n
        start[a] = True
        start[a + 1:a + k] = False
        if a + k < n:
            start[a + k] = True
    run = np.cumsum(start) - 1
    nruns = int(run[-1]) + 1
    # distinct ids: an odd multiplier is a bijection of u64 (and no run gets 0 or 2^64 - 1 by chance)
    tids = (np.arange(1, nruns + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    kind = rng.integers(0, 20, nruns)
    base = T0 + rng.integers(0, 8 * HOUR, nruns)
    base = np.where(kind == 0, T0 - 1 - rng.integers(0, HOUR, nruns), base)
    base = np.where(kind == 1, T0 + 8 * HOUR + rng.integers(0, HOUR, nruns), base)
    timed = (kind[run] != 2) & (rng.integers(0, 4, n) != 0)
    ts = np.where(timed, base[run] + rng.integers(0, 1000, n), INT64_MIN).astype(np.int64)
    for j, (a, k, where) in enumerate(specials):
        timed[a:a + k] = False
        ts[a:a + k] = INT64_MIN
        pos = {"first": a, "last": a + k - 1, "middle": a + k // 2, "none": None}[where]
        if pos is not None:
            timed[pos], ts[pos] = True, T0 + (1 + 3 * j) % 8 * HOUR + 5
    return fill(tids[run], ts, timed)


def smallest_n_with_chunks_per_range(k: int) -> int:
    """The smallest n whose plan gives every range k chunks (doubling, then bisection)."""
    c = plan(1)[0]
    lo, hi = 1, 2
    while plan(hi)[1] < k * c:
        lo, hi = hi, hi * 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if plan(mid)[1] >= k * c else (mid, hi)
    return hi


def multi_chunk_cases():
    """Ranges of more than one chunk, which only batches of millions of records have: the run carried
    from chunk to chunk inside a range, the cursors the scatter carries, hold-last cutting inside a
    range. One batch holds all the geometries, each in a range of its own."""
    c = plan(1)[0]
    n = smallest_n_with_chunks_per_range(3)
    R = plan(n)[1]
    assert R == 3 * c
    sp = []
    for k, where in zip((3, 5, 7, 9), WHERES):       # across one chunk edge inside a range
        sp.append((k * R + c - 10, 25, where))
    for k, where in zip((11, 13, 15, 17), WHERES):   # over three chunks, starting and ending inside the range
        sp.append((k * R + c - 24, c + 100, where))
    for k, where in zip((21, 23, 25, 27), WHERES):   # entering a range and ending in its third chunk
        sp.append((k * R - 5, 2 * c + 105, where))
    for k, where in zip((31, 33, 35, 37), WHERES):   # starting in a range's first chunk and leaving it
        sp.append((k * R + 500, R - 500 + 7, where))
    for k, where in zip((41, 47, 53, 59), WHERES):   # leaving over three chunks, two whole ranges, entering over two
        sp.append((k * R + 900, 3 * R + 600, where))
    sp.append((n - 2 * c - 30, 2 * c + 30, "first"))  # the batch's last run, over the last chunks
    # hold-last at two chunks per range: the last run crosses the chunk edge inside the last range
    n2 = smallest_n_with_chunks_per_range(2)
    R2 = plan(n2)[1]
    last0 = (n2 - 1) // R2 * R2
    m = last0 + c + 76
    assert plan(m)[1] == R2 == 2 * c and m >= n2
    return [("multi_chunk_ranges", big_batch(51, n, sp), T0, HOUR, 8, False),
            ("multi_chunk_ranges_hold_last", big_batch(52, n, sp), T0, HOUR, 8, True),
            ("hold_last_run_crosses_chunk_inside_range",
             big_batch(53, m, [(last0 + c - 24, 100, "last"), (5 * R2 + c - 3, 9, "middle")]), T0, HOUR, 8, True)]


def all_cases():
    return (shape_cases() + edge_cases() + id_cases() + rule_cases() + window_cases() + hold_cases()
            + multi_chunk_cases())


def names():
    """The names of all_cases(), without building a batch or asking the library for its geometry: test
    collection stays free of library calls."""
    return ([f"shape_{x}" for x in SHAPE_LABELS] + [f"{g}_{w}" for w in WHERES for g in EDGE_GEOS]
            + ["ids_0_and_max", "ids_repeated_not_adjacent", "untimed_int64_min_inside_timed_runs"]
            + [f"rule_o{o}_w{w}_W{W}" for o in I64_EDGES for w in WINDOWS for W in WS]
            + ["W1", "W1024_round_robin", "all_in_one_window", "all_in_the_rest"]
            + ["hold_last_run_of_1", "hold_last_run_crosses_range", "hold_last_run_crosses_two_ranges",
               "hold_whole_batch_one_run"]
            + ["multi_chunk_ranges", "multi_chunk_ranges_hold_last", "hold_last_run_crosses_chunk_inside_range"])


@functools.lru_cache(maxsize=None)
def _table():
    cases = {c[0]: c for c in all_cases()}
    assert list(cases) == names()
    return cases


def case(name):
    return _table()[name]
