"""Reference of the trace duration index (include/zkduration.h), in plain numpy and Python integers.

The index is a dict traceId -> (start, end): the minimum first_ts and the maximum last_ts over the timed
fragments of every observed batch. Nothing of the library's duration code is imported."""
import json
from pathlib import Path

import numpy as np

from tests.wincases import INT64_MAX, INT64_MIN, TIMED
from zipkin_amd import SpanColumns

GOLDEN = Path(__file__).resolve().parent / "golden" / "trace_durations.json"
ORDERS = ("duration-desc", "duration-asc", "timestamp-desc", "timestamp-asc")


def build(traces) -> SpanColumns:
    """traces: [(trace_id, [(first_ts, last_ts, timed), ...])] -> a batch with the runs back to back."""
    return fill(np.repeat(np.array([t[0] for t in traces], np.uint64), [len(t[1]) for t in traces]),
                np.array([r[0] for t in traces for r in t[1]], np.int64),
                np.array([r[1] for t in traces for r in t[1]], np.int64),
                np.array([bool(r[2]) for t in traces for r in t[1]], bool))


def fill(trace_id, first_ts, last_ts, timed) -> SpanColumns:
    """A batch from per-record trace ids, the two times and timed bits; the other columns from the
    index (tests/wincases.fill with a last_ts of its own)."""
    n = len(trace_id)
    c = SpanColumns.empty(n)
    idx = np.arange(n, dtype=np.uint64)
    c.trace_id[:] = trace_id
    c.span_id[:] = idx
    c.parent_id[:] = idx * np.uint64(0x9E3779B97F4A7C15)
    c.first_ts[:] = first_ts
    c.last_ts[:] = last_ts
    c.service_id[:] = (idx % np.uint64(61)).astype(np.uint32)
    c.flags[:] = ((idx.astype(np.uint32) * np.uint32(2654435761)) & np.uint32(0xFFFF_FF0D)) | (
        np.asarray(timed, bool).astype(np.uint32) * np.uint32(TIMED))
    return c


def table_of(batches) -> dict:
    """{traceId: (start, end)} over the batches (one batch or a sequence of them)."""
    if hasattr(batches, "trace_id"):
        batches = [batches]
    table = {}
    for cols in batches:
        timed = (cols.flags & np.uint32(TIMED)) != 0
        for tid, a, b in zip(cols.trace_id[timed].tolist(), cols.first_ts[timed].tolist(), cols.last_ts[timed].tolist()):
            s, e = table.get(tid, (a, b))
            table[tid] = (min(s, a), max(e, b))
    return table


def duration(start: int, end: int) -> int:
    """end - start as the reference's Long subtraction: it wraps."""
    d = (end - start) & (2 ** 64 - 1)
    return d - 2 ** 64 if d >= 2 ** 63 else d


def entries(table, ids):
    """getTracesDuration: [(traceId, duration, start)] of the asked ids the table holds, in asked order."""
    return [(i, duration(*table[i]), table[i][0]) for i in ids if i in table]


def top(table, order: str, k: int, lo: int = INT64_MIN, hi: int = INT64_MAX):
    """The first k (traceId, duration, start) in `order` of the traces with lo <= start <= hi; equal keys by
    traceId ascending."""
    assert order in ORDERS
    rows = [(i, duration(s, e), s) for i, (s, e) in table.items() if lo <= s <= hi]
    col = 1 if order.startswith("duration") else 2
    sign = -1 if order.endswith("desc") else 1
    rows.sort(key=lambda r: (sign * r[col], r[0]))
    return rows[:k]


def golden():
    return json.loads(GOLDEN.read_text())


def golden_batch(g, names) -> SpanColumns:
    """The named spans of the golden file as one batch: a span is one timed fragment from its first to
    its last annotation."""
    return build([(g["spans"][n]["trace_id"], [(min(g["spans"][n]["timestamps"]), max(g["spans"][n]["timestamps"]), True)])
                  for n in names])
