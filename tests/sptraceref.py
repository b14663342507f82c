"""Model of zk_sp_traces' output (include/zkspans.h): the 48-byte heads, the merged spans and the services
column, in plain Python integers, built on tests/spref.py's model store and the host class
zipkin_amd.spanstore.Trace, whose _merge, getRootMostSpan and toSpanDepths the header names as the call's
semantics. tests/test_span_trace_host.py holds that class against tests/spref.py's own restatement."""
import json
from pathlib import Path

from tests import spref as R
from zipkin_amd.spanstore import Trace

GOLDEN = Path(__file__).resolve().parent / "golden" / "trace_combos.json"
FOUND, TIMED, OVERFLOW = 1, 2, 4                              # ZK_SP_TR_*
HAS_PARENT, SPAN_TIMED, PARENT_FOUND, ROOT_MOST = 1, 2, 4, 8  # ZK_SP_SPAN_*
HEAD = ("trace_id", "start", "end", "root_most", "fragments", "spans", "services", "state")
SPAN = ("span_id", "parent_id", "first", "last", "name", "depth", "services", "bits")
ZERO = (0,) * 8


def one(trace_id, rows, max_rows):
    """(head, spans, services) of one asked id whose rows in the store are `rows`."""
    if not rows:
        return ZERO, [], []
    se = R.start_end(rows)
    state = FOUND | (TIMED if se is not None else 0)
    start, end = se if se is not None else (0, 0)
    if len(rows) > max_rows:
        return (trace_id, start, end, 0, len(rows), 0, 0, state | OVERFLOW), [], []
    t = Trace(rows)
    root, depths, held = t.getRootMostSpan(), t.toSpanDepths(), t.getIdToSpanMap()
    spans, services = [], []
    for s in t.spans:
        bits = (HAS_PARENT if s.parent is not None else 0) | (SPAN_TIMED if s.first is not None else 0)
        bits |= (PARENT_FOUND if s.parent is not None and s.parent in held else 0) | (ROOT_MOST if s.id == root.id else 0)
        spans.append((s.id, s.parent or 0, s.first or 0, s.last or 0, s.name, depths.get(s.id, 0), len(s.services), bits))
        services += list(s.services)
    return (trace_id, start, end, root.id, len(rows), len(spans), len(services), state), spans, services


def traces(store, ids, max_rows):
    """(heads, spans, services): one head tuple (in HEAD's order) per asked id, the span tuples (in SPAN's
    order) of the asked ids one after another, and their service ids."""
    by = {}
    for r in store:
        by.setdefault(r[0], []).append(r)
    heads, spans, services = [], [], []
    for i in ids:
        h, s, v = one(i, by.get(i, []), max_rows)
        heads.append(h)
        spans += s
        services += v
    return heads, spans, services


def combo_view(c):
    """What two TraceCombos are compared in: spans, summary, depths, root-most span, serviceCounts."""
    root = c.trace.getRootMostSpan()
    return (list(c.trace.spans), c.summary, c.timeline, c.span_depths, c.trace.toSpanDepths(),
            None if root is None else root.id, root, c.trace.serviceCounts())


def golden():
    return json.loads(GOLDEN.read_text())
