"""The dependency job's join rows WITH the child span's name id (TEST INFRASTRUCTURE ONLY): a plain
dict-based restatement of oracle/realtime.py joined_links, independent of its numpy formulation, plus
the merged span's name id -- the maximum of bits 16..31 of its fragments' flags (include/zkagg.h
ZK_F_NAME_SHIFT), 0 when none carries a name. With the rpc column dropped the rows must equal
joined_links on the same columns (`assert_tied_to_oracle`): that ties this helper to the oracle, and
the tests call it on every input they use.

Also the name assignment the generated batches share (`assign_names`)."""
from __future__ import annotations

import numpy as np

from oracle.realtime import joined_links

MAX_DURATION = 1 << 40
R = 7  # distinct span names of the generated batches (ids 1..R)
_I64_MAX, _I64_MIN = (1 << 63) - 1, -(1 << 63)


def rpc_rows(cols, num_services: int):
    """[(parent service, child service, duration, traceId, rpc id)] of every joined child span,
    sorted. Rules as joined_links: fragments grouped by (traceId, spanId); first/last = min/max over
    the fragments with annotations; service = the smallest (kind, id) with server before client, over
    fragments with a service id < num_services; valid = every core annotation at most once; parentId =
    the smallest over the fragments carrying one; joined against a valid merged parent of the same
    trace; both sides need a service; duration = last - first in [0, 2^40)."""
    spans = {}
    for tid, sid, pid, first, last, svc, f in zip(cols.trace_id.tolist(), cols.span_id.tolist(),
                                                  cols.parent_id.tolist(), cols.first_ts.tolist(),
                                                  cols.last_ts.tolist(), cols.service_id.tolist(),
                                                  cols.flags.tolist()):
        s = spans.get((tid, sid))
        if s is None:
            s = spans[(tid, sid)] = {"first": _I64_MAX, "last": _I64_MIN, "svc": None, "counts": [0, 0, 0, 0],
                                     "parent": None, "name": 0}
        if f & 2:
            s["first"] = min(s["first"], first)
            s["last"] = max(s["last"], last)
        kind = 0 if f & 8 else 1 if f & 4 else 2
        if kind < 2 and svc < num_services:
            key = (kind, svc)
            s["svc"] = key if s["svc"] is None else min(s["svc"], key)
        for c, sh in enumerate((8, 10, 12, 14)):
            s["counts"][c] += (f >> sh) & 3
        if f & 1:
            s["parent"] = pid if s["parent"] is None else min(s["parent"], pid)
        s["name"] = max(s["name"], f >> 16)
    rows = []
    for (tid, _), s in spans.items():
        if max(s["counts"]) > 1 or s["parent"] is None:
            continue
        p = spans.get((tid, s["parent"]))
        if p is None or max(p["counts"]) > 1 or p["svc"] is None or s["svc"] is None:
            continue
        if s["first"] == _I64_MAX:
            continue
        d = s["last"] - s["first"]
        if 0 <= d < MAX_DURATION:
            rows.append((p["svc"][1], s["svc"][1], d, tid, s["name"]))
    return sorted(rows)


def assert_tied_to_oracle(rows, cols, num_services: int) -> None:
    """rows minus the rpc column == joined_links of the same columns with the name bits masked off"""
    masked = cols.without_names()
    p, c, d, t = joined_links(masked, num_services)
    want = sorted(zip(p.tolist(), c.tolist(), d.tolist(), t.tolist()))
    assert sorted(r[:4] for r in rows) == want


def server_rows(rows, server: int, rpc=None):
    """(parent, duration, traceId, rpc) lists of `server` and rpc id `rpc` (None: any), in the
    (parent, duration, traceId, rpc) order zk_rl_server_rpc_links returns."""
    sel = sorted((p, d, t, n) for p, c, d, t, n in rows if c == server and (rpc is None or n == rpc))
    return [list(x) for x in zip(*sel)] if sel else [[], [], [], []]


def _mix(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    return (x ^ (x >> np.uint64(29))) >> np.uint64(17)


def assign_names(cols, seed: int, r: int = R):
    """Name ids into bits 16..31 of cols.flags, in place: every fragment of a span gets
    1 + mix(spanId) % r; about 10 % of the fragments are then set to 0 (no name) and about 5 % to a
    different id (fragments of one span that disagree: the maximum wins)."""
    rng = np.random.default_rng(seed)
    ids = 1 + (_mix(cols.span_id) % np.uint64(r)).astype(np.int64)
    u = rng.random(len(cols))
    ids[u < 0.10] = 0
    other = (u >= 0.10) & (u < 0.15)
    ids[other] = ids[other] % r + 1
    cols.set_name_ids(ids)
    return cols
