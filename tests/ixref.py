"""Reference of the trace-id index by service and span name (include/zkindex.h), in plain numpy and
Python integers.

The index is a list (a multiset) of entries (service, name id, ts, traceId): one per indexed fragment of
every observed batch. Nothing of the library's index code is imported."""
import json
from pathlib import Path

import numpy as np

from zipkin_amd import SpanColumns

GOLDEN = Path(__file__).resolve().parent / "golden" / "trace_ids_by_name.json"
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
TIMED = 1 << 1        # ZK_F_HAS_ANNOTATIONS
SVC_CLIENT = 1 << 2   # ZK_F_SVC_CLIENT
SVC_SERVER = 1 << 3   # ZK_F_SVC_SERVER
CS, CR, SR, SS = 8, 10, 12, 14  # the shifts of the 2-bit core annotation counts
NAME_SHIFT = 16
ANY = None            # trace_ids' name: every entry of the service


def batch(service, name, ts, trace_id, *, timed=True, svc=SVC_SERVER, cs=0, cr=0, sr=0, ss=0, seed=0) -> SpanColumns:
    """A batch from per-record service ids, name ids, last timestamps and trace ids; timed, the SVC bits
    and the four counts per record or one for all. The other columns, and the flag bits the index does
    not read (bit 0, bits 4..7), are noise."""
    trace_id = np.asarray(trace_id, np.uint64)
    n = len(trace_id)
    rng = np.random.default_rng(seed + n)
    full = lambda v, dt: np.broadcast_to(np.asarray(v, dt), (n,))
    c = SpanColumns.empty(n)
    c.trace_id[:] = trace_id
    c.span_id[:] = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    c.parent_id[:] = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    c.last_ts[:] = full(ts, np.int64)
    c.first_ts[:] = rng.integers(-2 ** 62, 2 ** 62, n)
    c.service_id[:] = full(service, np.uint32)
    flags = rng.integers(0, 256, n).astype(np.uint32) & np.uint32(0xF1)
    flags |= full(timed, bool).astype(np.uint32) * np.uint32(TIMED)
    flags |= full(svc, np.uint32)
    for count, shift in ((cs, CS), (cr, CR), (sr, SR), (ss, SS)):
        flags |= (full(count, np.uint32) & np.uint32(3)) << np.uint32(shift)
    flags |= full(name, np.uint32) << np.uint32(NAME_SHIFT)
    c.flags[:] = flags
    return c


def indexed_mask(cols, client_service=None) -> np.ndarray:
    """The INDEXED predicate per record."""
    f = cols.flags
    ok = ((f & np.uint32(TIMED)) != 0) & ((f & np.uint32(SVC_CLIENT | SVC_SERVER)) != 0)
    if client_service is not None:
        client_side = ((f >> np.uint32(CS)) & np.uint32(0xF)) != 0
        ok &= ~((cols.service_id == np.uint32(client_service)) & client_side)
    return ok


def entries_of(batches, num_services, client_service=None):
    """[(service, name, ts, trace_id)] over the batches (one batch or a sequence); a batch with an indexed
    record whose service id is out of range raises ValueError (the device refuses the whole batch)."""
    if hasattr(batches, "trace_id"):
        batches = [batches]
    out = []
    for cols in batches:
        m = indexed_mask(cols, client_service)
        if (cols.service_id[m] >= num_services).any():
            raise ValueError("service range")
        out += list(zip(cols.service_id[m].tolist(), (cols.flags[m] >> np.uint32(NAME_SHIFT)).tolist(),
                        cols.last_ts[m].tolist(), cols.trace_id[m].tolist()))
    return out


def trace_ids(entries, service, name, end_ts, limit):
    """([(trace_id, ts)] the first `limit` by ts descending then traceId ascending, matched)."""
    rows = [(t, ts) for s, nm, ts, t in entries if s == service and (name is ANY or nm == name) and ts <= end_ts]
    rows.sort(key=lambda r: (-r[1], r[0]))
    return rows[:limit], len(rows)


def span_names(entries, service):
    """The distinct non-zero name ids of the service's entries, ascending."""
    return sorted({nm for s, nm, _, _ in entries if s == service and nm != 0})


def service_counts(entries, num_services=None):
    """Entries per service: a dict, or with num_services an array."""
    if num_services is None:
        d = {}
        for s, *_ in entries:
            d[s] = d.get(s, 0) + 1
        return d
    return np.bincount(np.array([e[0] for e in entries], np.int64), minlength=num_services).astype(np.uint64)


def golden():
    return json.loads(GOLDEN.read_text())


def golden_batch(g):
    """(batch, services, span_names) of the golden file's spans: a span is one timed fragment whose
    last_ts is its last annotation's timestamp, its service from the side the file names."""
    services = sorted({s["service"] for s in g["spans"].values()})
    names = sorted({s["name"] for s in g["spans"].values()})
    spans = list(g["spans"].values())
    client = np.array([s["side"] == "client" for s in spans])
    b = batch([services.index(s["service"]) for s in spans], [names.index(s["name"]) + 1 for s in spans],
              [max(s["timestamps"]) for s in spans], [s["trace_id"] for s in spans],
              svc=np.where(client, SVC_CLIENT, SVC_SERVER), cs=[s["core"].count("cs") for s in spans],
              cr=[s["core"].count("cr") for s in spans], sr=[s["core"].count("sr") for s in spans],
              ss=[s["core"].count("ss") for s in spans])
    return b, services, names
