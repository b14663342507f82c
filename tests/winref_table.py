"""Reference of the table-mode trace-time partition (include/zkwindow.h, ZK_WIN_TRACE_TABLE), in plain
numpy and Python integers.

The trace-time table is a dict traceId -> the minimum first_ts over the timed fragments of every
observed batch; a record's class follows from its trace's time in that dict by the window rule of
tests/winref.py, and the partition is a stable argsort of the per-record classes. Nothing of the
library is imported."""
import numpy as np

from tests.winref import COLS, HAS_ANNOTATIONS, index, run_starts


def table_of(batches) -> dict:
    """{traceId: min timed first_ts} over the batches (one batch or a sequence of them)."""
    if hasattr(batches, "trace_id"):
        batches = [batches]
    table = {}
    for cols in batches:
        timed = (cols.flags & np.uint32(HAS_ANNOTATIONS)) != 0
        for tid, t in zip(cols.trace_id[timed].tolist(), cols.first_ts[timed].tolist()):
            if tid not in table or t < table[tid]:
                table[tid] = t
    return table


def classify(cols, table, origin: int, window: int, W: int) -> np.ndarray:
    """cls[i] of record i: its window 0..W-1, W before, W + 1 after, W + 2 untimed (its traceId is not
    in the table)."""
    by_id = {}
    for tid in set(cols.trace_id.tolist()):
        if tid not in table:
            by_id[tid] = W + 2
            continue
        t = table[tid]
        w = index(t, origin, window, W)
        by_id[tid] = w if w < W else (W if t < origin else W + 1)
    return np.array([by_id[t] for t in cols.trace_id.tolist()], np.int64).reshape(len(cols.trace_id))


def partition(cols, table, origin: int, window: int, W: int):
    """(out, offsets, counts): out = {column: array} in window order then the rest, offsets of W + 2
    entries, counts = the zk_win_counts fields in table mode."""
    n = len(cols.trace_id)
    cls = classify(cols, table, origin, window, W)
    part = np.minimum(cls, W)
    order = np.argsort(part, kind="stable")
    out = {k: np.ascontiguousarray(getattr(cols, k)[order]) for k in COLS}
    per = np.bincount(part, minlength=W + 1)
    offsets = np.concatenate(([0], np.cumsum(per))).astype(np.uint64)
    rcls = cls[run_starts(cols.trace_id)]
    timed = (cols.flags & np.uint32(HAS_ANNOTATIONS)) != 0
    known = np.array([t in table for t in cols.trace_id.tolist()], bool).reshape(n)
    counts = {
        "partitioned_runs": int((rcls < W).sum()), "partitioned_records": int((cls < W).sum()),
        "before_runs": int((rcls == W).sum()), "before_records": int((cls == W).sum()),
        "after_runs": int((rcls == W + 1).sum()), "after_records": int((cls == W + 1).sum()),
        "untimed_runs": int((rcls == W + 2).sum()), "untimed_records": int((cls == W + 2).sum()),
        "held_runs": 0, "held_records": 0, "held_from": n,
        "unobserved_records": int((timed & ~known).sum()),
    }
    return out, offsets, counts


def shuffled(cols, seed: int):
    """The batch's records in a seeded random order (a SpanColumns-like object with take())."""
    return cols.take(np.random.default_rng(seed).permutation(len(cols.trace_id)))


def cut(cols, positions):
    """The batch cut at the given record positions into len(positions) + 1 batches."""
    edges = [0] + sorted(int(p) for p in positions) + [len(cols.trace_id)]
    return [cols.take(slice(a, b)) for a, b in zip(edges, edges[1:])]
