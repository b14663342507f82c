"""Reference of the span store by trace id (include/zkspans.h) and of Trace / TraceSummary at record
granularity, in plain Python integers.

The store is a list (a multiset) of row tuples (trace_id, span_id, parent_id, first_ts, last_ts,
service_id, flags): every record of every observed batch. Nothing of the library's span-store code is
imported."""
import json
from pathlib import Path

import numpy as np

from zipkin_amd import SpanColumns

GOLDEN = Path(__file__).resolve().parent / "golden" / "trace_summaries.json"
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
M64 = 2 ** 64 - 1
HAS_PARENT = 1 << 0   # ZK_F_HAS_PARENT
TIMED = 1 << 1        # ZK_F_HAS_ANNOTATIONS
SVC_CLIENT = 1 << 2   # ZK_F_SVC_CLIENT
SVC_SERVER = 1 << 3   # ZK_F_SVC_SERVER
NAME_SHIFT = 16
SALT = 0x8CB92BA72F3D8DD7  # ZK_SP_SALT
COLS = ("trace_id", "span_id", "parent_id", "first_ts", "last_ts", "service_id", "flags")


def mix64(z: int) -> int:
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def unmix64(z: int) -> int:
    z &= M64
    z = z ^ (z >> 31) ^ (z >> 62)
    z = (z * 0x319642B2D24D8EC3) & M64
    z = z ^ (z >> 27) ^ (z >> 54)
    z = (z * 0x96DE1B173F119089) & M64
    return z ^ (z >> 30) ^ (z >> 60)


def bucket(trace_id: int) -> int:
    """The header's bucket function: the 12 highest bits of the salted hash."""
    return mix64(trace_id ^ SALT) >> 52


def id_in_bucket(b: int, k: int) -> int:
    """The k-th (any k < 2^52) trace id whose bucket is b."""
    return unmix64((b << 52) | k) ^ SALT


def rows_of(batches):
    """The store after observing the batches (one batch or a sequence): a list of row tuples."""
    if hasattr(batches, "trace_id"):
        batches = [batches]
    out = []
    for c in batches:
        out += list(zip(*[getattr(c, k).tolist() for k in COLS]))
    return out


def cols_of(rows) -> SpanColumns:
    """A batch of the rows, in their order."""
    c = SpanColumns.empty(len(rows))
    for j, k in enumerate(COLS):
        col = getattr(c, k)
        for i, r in enumerate(rows):
            col[i] = r[j]
    return c


def exist(store, ids):
    have = {r[0] for r in store}
    return [i in have for i in ids]


def gather(store, ids):
    """(counts, rows): per asked id its rows in canonical order, the asked ids' rows one after another."""
    by = {}
    for r in store:
        by.setdefault(r[0], []).append(r)
    counts, rows = [], []
    for i in ids:
        mine = sorted(by.get(i, []), key=lambda r: r[1:])
        counts.append(len(mine))
        rows += mine
    return counts, rows


def spans_by_trace_ids(store, ids):
    """getSpansByTraceIds: one row list per asked id that exists, in the order asked."""
    by = {}
    for r in store:
        by.setdefault(r[0], []).append(r)
    return [sorted(by[i], key=lambda r: r[1:]) for i in ids if i in by]


def trace(rows, services=None):
    """The merged spans of one trace's rows, in span order: dicts id, parent, name, first, last, services."""
    spans = {}
    for r in sorted(rows, key=lambda r: r[1:]):
        _, sid, pid, first, last, svc, fl = r
        s = spans.setdefault(sid, {"id": sid, "parent": None, "name": 0, "first": None, "last": None, "services": set()})
        if fl & HAS_PARENT and s["parent"] is None:
            s["parent"] = pid
        if s["name"] == 0:
            s["name"] = fl >> NAME_SHIFT
        if fl & TIMED:
            s["first"] = first if s["first"] is None else min(s["first"], first)
            s["last"] = last if s["last"] is None else max(s["last"], last)
        if fl & (SVC_CLIENT | SVC_SERVER):
            s["services"].add(svc)
    out = sorted(spans.values(), key=lambda s: (INT64_MAX if s["first"] is None else s["first"], s["id"]))
    for s in out:
        s["services"] = [services[v].lower() if services is not None else v for v in sorted(s["services"])]
    return out


def start_end(rows):
    timed = [r for r in rows if r[6] & TIMED]
    if not timed:
        return None
    return min(r[3] for r in timed), max(r[4] for r in timed)


def wrap64(x: int) -> int:
    x &= M64
    return x - 2 ** 64 if x >> 63 else x


def to_int(x: int) -> int:
    x &= 0xFFFFFFFF
    return x - 2 ** 32 if x >> 31 else x


def span_timestamps(rows, services=None):
    return [(v, s["first"], s["last"]) for s in trace(rows, services) if s["first"] is not None for v in s["services"]]


def service_counts(rows, services=None):
    out = {}
    for s in trace(rows, services):
        for v in s["services"]:
            out[v] = out.get(v, 0) + 1
    return out


def summary(rows, services=None):
    """(trace_id, start, end, duration_micro, span_timestamps, endpoints) or None."""
    se = start_end(rows)
    if not rows or se is None:
        return None
    return (rows[0][0], se[0], se[1], to_int(wrap64(se[1] - se[0])), span_timestamps(rows, services), [])


def root_most(rows):
    spans = trace(rows)
    if not spans:
        return None
    for s in spans:
        if s["parent"] is None:
            return s
    by = {s["id"]: s for s in spans}
    s, seen = spans[0], set()
    while s["parent"] in by and s["id"] not in seen:
        seen.add(s["id"])
        s = by[s["parent"]]
    return s


def span_depths(rows):
    """span id -> depth under the root-most span (depth 1); None for no rows."""
    root = root_most(rows)
    if root is None:
        return None
    spans = trace(rows)
    depths, level, d = {}, [root], 1
    while level:
        nxt = []
        for s in level:
            if s["id"] in depths:
                continue
            depths[s["id"]] = d
            nxt += [c for c in spans if c["parent"] == s["id"]]
        level, d = nxt, d + 1
    return depths


def golden():
    return json.loads(GOLDEN.read_text())


def golden_rows(case, services):
    """The rows of a golden case: one record per (span, service side) as the file lists them."""
    rows = []
    for r in case["records"]:
        fl = (HAS_PARENT if r["parent_id"] is not None else 0) | (TIMED if r["timed"] else 0)
        if r["service"] is not None:
            fl |= SVC_CLIENT if r.get("side", "client") == "client" else SVC_SERVER
        fl |= r.get("name_id", 0) << NAME_SHIFT
        rows.append((case["trace_id"], r["span_id"], r["parent_id"] or 0, r["first_ts"], r["last_ts"],
                     services.index(r["service"]) if r["service"] is not None else 0, fl))
    return rows


def shuffled_batches(cols, k, seed):
    """The batch's records in shuffled order, cut into k batches."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(cols))
    cuts = np.linspace(0, len(cols), k + 1).astype(int)
    return [cols.take(perm[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
