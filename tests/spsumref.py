"""Model of zk_sp_summaries' output (include/zkspans.h): the 40-byte heads and the entry columns, in plain
Python integers, built from tests/spref.py's trace and start_end alone. Nothing of the library's span-store
code is imported."""
from tests import spref as R

FOUND, TIMED, OVERFLOW = 1, 2, 4  # ZK_SP_SUM_FOUND, ZK_SP_SUM_TIMED, ZK_SP_SUM_OVERFLOW
HEAD = ("trace_id", "start", "end", "fragments", "spans", "span_ts", "state")
ZERO = (0, 0, 0, 0, 0, 0, 0)


def one(trace_id, rows, max_rows):
    """(head, entries) of one asked id whose rows in the store are `rows`."""
    if not rows:
        return ZERO, []
    se = R.start_end(rows)
    state = FOUND | (TIMED if se is not None else 0)
    start, end = se if se is not None else (0, 0)
    if len(rows) > max_rows:
        return (trace_id, start, end, len(rows), 0, 0, state | OVERFLOW), []
    spans = R.trace(rows)
    entries = [(v, s["first"], s["last"]) for s in spans if s["first"] is not None for v in s["services"]]
    return (trace_id, start, end, len(rows), len(spans), len(entries), state), entries


def summaries(store, ids, max_rows):
    """(heads, entries): one head tuple (in HEAD's order) per asked id, and the (service_id, first, last)
    entries of the asked ids one after another."""
    by = {}
    for r in store:
        by.setdefault(r[0], []).append(r)
    heads, entries = [], []
    for i in ids:
        h, e = one(i, by.get(i, []), max_rows)
        heads.append(h)
        entries += e
    return heads, entries


def assemble(heads, entries, services=None):
    """The TraceSummary tuples (spref.summary's form) that the heads and entries stand for: ids that are
    not found and untimed traces are left out. A head with OVERFLOW has no entries to assemble from."""
    out, at = [], 0
    for tid, start, end, _, _, c, state in heads:
        assert not state & OVERFLOW
        if state & TIMED:
            ts = [(services[v].lower() if services is not None else v, f, l) for v, f, l in entries[at:at + c]]
            out.append((tid, start, end, R.to_int(R.wrap64(end - start)), ts, []))
        at += c
    assert at == len(entries)
    return out
