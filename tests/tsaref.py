"""The time-skew adjuster and the trace timeline restated from their stated rules, over plain
dicts and tuples. Nothing of zipkin_amd's Trace, TimeSkewAdjuster or TraceTimeline is imported: the span
merge is tests/spref.py's, the annotation order tests/anref.py's.

A span is a dict: id, parent, name, first, last, services (spref.trace's), and ann, a list of annotations
[ts, value, kind, host], host = (ipv4, port, service_id) or None."""
import json
from collections import deque
from pathlib import Path

from tests import anref as A
from tests import spref as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "time_skew.json"
LOOPBACK = 0x7F000001
TWO63, TWO64 = 1 << 63, 1 << 64


def fnv_mix(text: bytes) -> int:
    """zk_hash_string: 64-bit FNV-1a, then the splitmix64 finalizer."""
    h = 0xCBF29CE484222325
    for c in text:
        h = ((h ^ c) * 0x100000001B3) % TWO64
    return R.mix64(h)


H_SR, H_SS = fnv_mix(b"sr"), fnv_mix(b"ss")


def jlong(x: int) -> int:
    """An integer as the JVM's Long holds it."""
    return (x + TWO63) % TWO64 - TWO63


def jhalf(x: int) -> int:
    """Long / 2: toward zero."""
    return x // 2 if x >= 0 else -((-x) // 2)


def order(spans):
    return sorted(spans, key=lambda s: (R.INT64_MAX if s["first"] is None else s["first"], s["id"]))


def retime(s):
    if s["ann"]:
        s["first"], s["last"] = min(a[0] for a in s["ann"]), max(a[0] for a in s["ann"])
    return s


def annotated(span_rows, ann_rows):
    """The trace's merged spans in span order, each with its annotations in canonical order."""
    spans = R.trace(span_rows)
    for s in spans:
        s["ann"] = [[r[2], r[3], r[6] & A.KIND_MASK, (r[4], r[6] >> A.PORT_SHIFT, r[5]) if r[6] & A.HAS_HOST else None]
                    for r in sorted(ann_rows, key=A.key) if r[1] == s["id"]]
        retime(s)
    return order(spans)


def skew_of(cs, cr, sr, ss, endpoint):
    cd, sd = jlong(cr - cs), jlong(ss - sr)
    if sd > cd:
        return None
    if cs < sr and cr > ss:
        return None
    latency = jhalf(jlong(cd - sd))
    skew = jlong(jlong(sr - latency) - cs)
    return None if skew == 0 or endpoint is None else (endpoint, skew)


def shift(ann, by):
    if by is None or by[1] == 0:
        return
    endpoint, skew = by
    for a in ann:
        if a[3] is None:
            continue
        if a[3][0] == endpoint[0] or (a[2] in (A.CS, A.CR) and a[3][0] == LOOPBACK):
            a[0] = jlong(a[0] - skew)


def first_of(ann, *kinds):
    for a in ann:
        if a[2] in kinds:
            return a
    return None


def adjust(spans):
    """TIME_SKEW over annotated() spans: a new list, the input untouched."""
    spans = [dict(s, ann=[list(a) for a in s["ann"]]) for s in spans]
    root = next((s for s in spans if s["parent"] is None), None)
    if root is None:
        return spans
    kids_of = {}
    for s in spans:
        if s["parent"] is not None:
            kids_of.setdefault(s["parent"], []).append(s)
    kept, todo = [], deque([(root, None)])
    while todo:  # level by level: a span touches itself and its children only
        s, prev = todo.popleft()
        kept.append(s)
        ann, kids = s["ann"], kids_of.get(s["id"], [])
        shift(ann, prev)
        kinds = [a[2] for a in ann]
        once = all(kinds.count(k) <= 1 for k in (A.CS, A.CR, A.SR, A.SS))
        if once and A.CS in kinds and A.CR in kinds and not (A.SR in kinds and A.SS in kinds) and kids:
            lead = first_of(kids[0]["ann"], A.CS, A.CR)
            endpoint = lead[3] if lead else None
            cs, cr = first_of(ann, A.CS)[0], first_of(ann, A.CR)[0]
            ann.append([cs, H_SR, A.SR, endpoint])
            ann.append([cr, H_SS, A.SS, endpoint])
            for k in kids:
                kcs, kcr = first_of(k["ann"], A.CS), first_of(k["ann"], A.CR)
                if kcs and kcr:
                    shift(k["ann"], skew_of(cs, cr, kcs[0], kcr[0], endpoint))
        own = None
        by_kind = {a[2]: a for a in ann}  # the last of each
        if all(k in by_kind for k in (A.CS, A.CR, A.SR, A.SS)):
            own = skew_of(by_kind[A.CS][0], by_kind[A.CR][0], by_kind[A.SR][0], by_kind[A.SS][0], by_kind[A.SR][3])
            shift(ann, own)
        todo.extend((k, own) for k in kids)
    return order([retime(s) for s in kept])


def fold(spans, adjusters):
    for name in adjusters:
        spans = {"NOTHING": lambda x: x, "TIME_SKEW": adjust}[name](spans)
    return spans


def summary(spans, trace_id, services=None):
    """(trace_id, start, end, duration_micro, span_timestamps, endpoints) or None."""
    timed = [s for s in spans if s["first"] is not None]
    if not timed:
        return None
    start, end = min(s["first"] for s in timed), max(s["last"] for s in timed)
    return (trace_id, start, end, R.to_int(jlong(end - start)),
            [(v, s["first"], s["last"]) for s in timed for v in s["services"]], [])


def root_most(spans):
    for s in spans:
        if s["parent"] is None:
            return s
    by = {s["id"]: s for s in spans}
    s, seen = spans[0], set()
    while s["parent"] in by and s["id"] not in seen:
        seen.add(s["id"])
        s = by[s["parent"]]
    return s


def timeline(spans, trace_id, services=None):
    """(trace_id, root span id, [(ts, value, ipv4, port, service, span_id, parent_id, span name)]) or None."""
    if not spans:
        return None
    out = []
    for s in spans:
        for ts, value, _, host in s["ann"]:
            if host is None:
                ep = (0, 0, 0 if services is None else "Unknown")
            else:
                ep = (host[0], host[1], host[2] if services is None else services[host[2]])
            out.append((ts, value) + ep + (s["id"], s["parent"], s["name"]))
    return (trace_id, root_most(spans)["id"], sorted(out, key=lambda a: a[0]))


def view(spans):
    """{span id: [(ts, value, kind, host)]}, the form the tests compare in."""
    return {s["id"]: [(a[0], a[1], a[2], a[3]) for a in s["ann"]] for s in spans}


def random_case(rng, trace_id, max_spans=64):
    """A seeded random trace in the golden file's form: a tree of up to max_spans spans, hosts drawn from
    three ipv4s whose clocks are off by up to +-500 (both signs), a client and a server side per span; now
    and then a missing or doubled core annotation, an annotation without a host, a loopback client, a free
    annotation, a second root or a parent that is not in the trace."""
    ips = [167772161, 167772162, 167772163]
    off = {ip: int(rng.integers(-500, 501)) for ip in ips}
    off[LOOPBACK] = 0
    n = int(rng.integers(1, max_spans + 1))
    ids = rng.choice(10 * max_spans, n, replace=False).tolist()
    spans = []
    for i, sid in enumerate(ids):
        parent = None if i == 0 else ids[int(rng.integers(0, i))]
        if i and rng.random() < 0.05:
            parent = None if rng.random() < 0.5 else 10 * max_spans + 7
        t0 = 1000 + 40 * i + int(rng.integers(0, 30))
        lat, work = int(rng.integers(0, 20)), int(rng.integers(0, 200))
        client = ips[int(rng.integers(0, 3))] if rng.random() < 0.9 else LOOPBACK
        server = ips[int(rng.integers(0, 3))]
        anns = [[t0 + off[client], "cs", client], [t0 + lat + off[server], "sr", server],
                [t0 + lat + work + off[server], "ss", server], [t0 + 2 * lat + work + off[client], "cr", client]]
        if rng.random() < 0.3:
            anns = [a for a in anns if a[1] in ("cs", "cr")] if rng.random() < 0.6 else [a for a in anns if rng.random() < 0.7]
        if rng.random() < 0.1 and anns:
            anns.append(list(anns[int(rng.integers(0, len(anns)))]))
            anns[-1][0] += int(rng.integers(0, 3))
        if rng.random() < 0.1 and anns:
            anns[int(rng.integers(0, len(anns)))][2] = None
        if rng.random() < 0.3:
            anns.append([t0 + int(rng.integers(0, 50)), "foo" if rng.random() < 0.5 else "bar", ips[int(rng.integers(0, 3))]])
        spans.append({"id": sid, "parent": parent, "annotations": anns})
    return {"trace_id": trace_id, "spans": spans}


# ---- the golden file ---------------------------------------------------------------------------------------
def golden():
    return json.loads(GOLDEN.read_text())


KIND_OF = {"cs": A.CS, "cr": A.CR, "sr": A.SR, "ss": A.SS}


def golden_rows(case):
    """(span rows, annotation rows) of a golden case. A span lists its annotations [ts, text, ipv4 or null];
    its record is derived as the decoder derives it: times from the annotations, the service from the first
    sr/ss host, else the first cs/cr host; a host's service id is ipv4 & 0xFF, its port 80."""
    tid = case["trace_id"]
    spans, anns = [], []
    for s in case["spans"]:
        fl = R.HAS_PARENT if s["parent"] is not None else 0
        svc = 0
        if s["annotations"]:
            fl |= R.TIMED
        server = [a for a in s["annotations"] if a[1] in ("sr", "ss") and a[2] is not None]
        client = [a for a in s["annotations"] if a[1] in ("cs", "cr") and a[2] is not None]
        if server:
            fl, svc = fl | R.SVC_SERVER, server[0][2] & 0xFF
        elif client:
            fl, svc = fl | R.SVC_CLIENT, client[0][2] & 0xFF
        ts = [a[0] for a in s["annotations"]]
        spans.append((tid, s["id"], s["parent"] or 0, min(ts) if ts else 0, max(ts) if ts else 0, svc, fl))
        for t, text, ip in s["annotations"]:
            bits = KIND_OF.get(text, 0) | ((A.HAS_HOST | (80 << A.PORT_SHIFT)) if ip is not None else 0)
            anns.append((tid, s["id"], t, fnv_mix(text.encode()), ip or 0, (ip & 0xFF) if ip is not None else 0, bits))
    return spans, anns
