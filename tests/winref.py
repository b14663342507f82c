"""Reference of the trace-time partition (include/zkwindow.h), in plain numpy and Python integers.

Independent of the library and of oracle/: run boundaries by neighbour compare, the per-run minimum
over the timed fragments, the window rule with Python's unbounded integers, and a stable argsort on
the window ids. Columns are anything with the seven attributes of zipkin_amd.SpanColumns; outputs
are plain dicts of numpy arrays."""
import numpy as np

COLS = ("trace_id", "span_id", "parent_id", "first_ts", "last_ts", "service_id", "flags")
HAS_ANNOTATIONS = 1 << 1
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
MAX_WINDOWS = 1024


def index(t: int, origin: int, window: int, W: int) -> int:
    """The window of trace time t; W for before and after."""
    assert window > 0 and 1 <= W <= MAX_WINDOWS
    if t < origin:
        return W
    w = (t - origin) // window
    return w if w < W else W


def run_starts(trace_id: np.ndarray) -> np.ndarray:
    """Index of the first record of every trace run (maximal stretch of equal adjacent ids)."""
    n = len(trace_id)
    if n == 0:
        return np.zeros(0, np.int64)
    return np.flatnonzero(np.concatenate(([True], trace_id[1:] != trace_id[:-1]))).astype(np.int64)


def classify(cols, origin: int, window: int, W: int):
    """(starts, cls): cls[r] of run r is its window 0..W-1, W before, W + 1 after, W + 2 untimed."""
    starts = run_starts(cols.trace_id)
    ends = np.concatenate((starts[1:], [len(cols.trace_id)])).astype(np.int64)
    timed = (cols.flags & np.uint32(HAS_ANNOTATIONS)) != 0
    cls = np.zeros(len(starts), np.int64)
    for r, (a, b) in enumerate(zip(starts.tolist(), ends.tolist())):
        ts = cols.first_ts[a:b][timed[a:b]]
        if len(ts) == 0:
            cls[r] = W + 2
            continue
        t = int(ts.min())
        if t < origin:
            cls[r] = W
        else:
            w = (t - origin) // window
            cls[r] = w if w < W else W + 1
    return starts, cls


def partition(cols, origin: int, window: int, W: int, hold_last: bool = False):
    """(out, offsets, counts): out = {column: array} in window order then the rest, offsets of W + 2
    entries, counts = the zk_win_counts fields."""
    n = len(cols.trace_id)
    starts, cls = classify(cols, origin, window, W)
    ends = np.concatenate((starts[1:], [n])).astype(np.int64)
    held_from = n
    held_runs = 0
    if hold_last and n:
        held_from = int(starts[-1])
        held_runs = 1
        starts, ends, cls = starts[:-1], ends[:-1], cls[:-1]
    lens = ends - starts
    rec_cls = np.repeat(cls, lens)  # class of every record before held_from
    part = np.minimum(rec_cls, W)
    order = np.argsort(part, kind="stable")
    out = {k: np.ascontiguousarray(getattr(cols, k)[:held_from][order]) for k in COLS}
    per = np.bincount(part, minlength=W + 1)
    offsets = np.concatenate(([0], np.cumsum(per))).astype(np.uint64)
    counts = {
        "partitioned_runs": int((cls < W).sum()), "partitioned_records": int(lens[cls < W].sum()),
        "before_runs": int((cls == W).sum()), "before_records": int(lens[cls == W].sum()),
        "after_runs": int((cls == W + 1).sum()), "after_records": int(lens[cls == W + 1].sum()),
        "untimed_runs": int((cls == W + 2).sum()), "untimed_records": int(lens[cls == W + 2].sum()),
        "held_runs": held_runs, "held_records": n - held_from, "held_from": held_from,
    }
    return out, offsets, counts


def window_records(cols, origin: int, window: int, W: int, w: int) -> np.ndarray:
    """Indices (ascending) of the input records of window w (w == W: the rest)."""
    starts, cls = classify(cols, origin, window, W)
    ends = np.concatenate((starts[1:], [len(cols.trace_id)])).astype(np.int64)
    rec = np.minimum(np.repeat(cls, ends - starts), W)
    return np.flatnonzero(rec == w)
