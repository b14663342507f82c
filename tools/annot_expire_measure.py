#!/usr/bin/env python3
"""Measurement of the annotation store's expiry beside the span store's, recorded, not gated:
the yardstick is zk_sp_expire in the same process, not a number fixed in advance, and bench.py does not run it.

Workload: the C2 batch on the device (bench.py's: --records 1e8, S = 500, seed 2) with EVERY fragment marked
timed, in a TraceSpanStore; and in a TraceAnnotationStore one row per fragment (trace_id, span_id, ts =
last_ts; the other four columns are views of the batch's columns, their values do not matter here). Both
stores so hold the same entry count, the same traces with the same ends, and one cutoff removes the same
traces from both. In one process the two expiries alternate: fill both, zk_an_expire, zk_sp_expire, --runs
times after a first call that is reported apart. Per phase (zk_an_expire_ms / zk_sp_expire_ms: ends, sizing
sync, rewrite) the median and [min, max] of the device ms, and the bytes/s of the phase's own bytes:
  ends     the range tables cleared (16 B per slot), the fold's read (annotations 16 B per entry: trace_id,
           ts; spans 20 B: trace_id, last_ts, flags), the mark's read (8 B) and 1 bit per entry written;
  rewrite  1 bit per entry of the mixed segments read twice, per survivor trace_id twice and the other six
           columns read and seven written (annotations 52 + 44 B, spans 56 + 48 B).
  --case half     one segment, the cutoff at the median trace end: half the traces expire;
  --case sorted   64 time-sorted segments (the batch sorted by its fragments' trace end), the same cutoff:
                  the old segments are freed whole, at most one is rewritten;
  --case none     one segment, the cutoff at the smallest ts: nothing expires.
Every case is a process of its own, so that each runs under its own time limit, chained with &&:
  for c in half sorted none; do timeout -k 10 300 python tools/annot_expire_measure.py --case $c || exit 1; done &&
  python tools/annot_expire_measure.py --report
A case writes <out>/part_<case>.json; --report (no device needed) joins the parts into <out>/measure.json
and <out>/measure.txt and removes them. Needs a gfx950 device."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CASES = ("half", "sorted", "none")
PHASES = ("ends", "size", "rewrite")
# bytes per entry: the fold's read, the mark's read, a survivor's read and write
BYTES = {"an": {"fold": 16, "mark": 8, "read": 52, "write": 44}, "sp": {"fold": 20, "mark": 8, "read": 56, "write": 48}}
SLOT_BYTES = 16
CHUNK = 1 << 24  # expire_chunk's default in both stores
BUCKETS = 4096
K = 64
TITLES = {"half": "(half) one segment, half the traces expiring",
          "sorted": "(sorted) 64 time-sorted segments, old ones freed whole, at most one rewritten",
          "none": "(none) one segment, nothing expiring"}
NAMES = {"an": "zk_an_expire", "sp": "zk_sp_expire"}


def summary(xs):
    xs = list(xs)
    return {"first": xs[0], "median": statistics.median(xs[1:]), "min": min(xs[1:]), "max": max(xs[1:]), "runs": len(xs) - 1}


def table_bytes(entries: int) -> int:
    """The bytes the ranges' tables are cleared over, for entries spread evenly over the buckets: ranges of
    whole buckets inside the chunk, slots the power of two at or above twice a range's entries."""
    per_bucket = max(1, entries // BUCKETS)
    per_range = max(1, min(BUCKETS, CHUNK // per_bucket))
    total, b = 0, 0
    while b < BUCKETS:
        nb = min(per_range, BUCKETS - b)
        slots = 1024
        while slots < 2 * nb * per_bucket:
            slots *= 2
        total += (slots + 1) * SLOT_BYTES
        b += nb
    return total


def run_case(a):
    import torch

    from zipkin_amd import DepsContext, DeviceAnnotationRows, DeviceColumns, TraceAnnotationStore, TraceSpanStore, tracegen_params

    if not torch.cuda.is_available():
        raise SystemExit("annot_expire_measure needs a HIP device")
    S = a.services
    ctx = DepsContext(S, device=0)
    p = tracegen_params(a.seed, int(a.records / 15) + 1000, target_records=a.records, max_depth=a.max_depth, num_services=S)
    cols = DeviceColumns(a.records, device="cuda:0")
    n, ntr = ctx.tracegen_device(p, cols)
    ctx.sync()
    ctx.close()
    cols = cols.slice(0, n)
    cols.flags |= 2  # ZK_F_HAS_ANNOTATIONS on every fragment: a trace's end is the maximum last_ts in both stores
    torch.cuda.synchronize()
    res = {"case": a.case, "records": n, "traces": ntr, "services": S, "seed": a.seed, "device": torch.cuda.get_device_name(0),
           "runs": a.runs}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    _, inv = torch.unique(cols.trace_id, return_inverse=True)
    ends = torch.full((int(inv.max()) + 1,), -2 ** 63, dtype=torch.int64, device=inv.device)
    ends.scatter_reduce_(0, inv, cols.last_ts, "amax")
    cut = int(cols.last_ts.min()) if a.case == "none" else int(ends.median()) + 1
    if a.case == "sorted":  # in the order of the fragments' trace ends: a segment is then all old, all new, or the one in between
        perm = torch.argsort(ends[inv])
        for k in ("trace_id", "span_id", "parent_id", "first_ts", "last_ts", "service_id", "flags"):
            getattr(cols, k).copy_(getattr(cols, k)[perm])
        del perm
    del inv, ends
    torch.cuda.synchronize()
    rows = DeviceAnnotationRows(cols.trace_id, cols.span_id, cols.last_ts, cols.parent_id, cols.service_id, cols.service_id, cols.flags)
    parts = 1 if a.case != "sorted" else K

    def fill(h, data, cut_of):
        h.reset()
        for j in range(parts):
            h.observe(cut_of(data, j * n // parts, (j + 1) * n // parts), sync=False)
        return h.info()

    def rows_slice(r, lo, hi):
        return DeviceAnnotationRows(*[getattr(r, k)[lo:hi] for k in ("trace_id", "span_id", "ts", "value", "ipv4", "service_id", "bits")])

    got = {"an": {"walls": [], "phases": []}, "sp": {"walls": [], "phases": []}}
    with TraceAnnotationStore(device=0, timing=True) as an, TraceSpanStore(device=0, timing=True) as sp:
        for _ in range(a.runs + 1):
            got["an"]["before"] = fill(an, rows, rows_slice)
            got["sp"]["before"] = fill(sp, cols, lambda c, lo, hi: c.slice(lo, hi))
            for key, h in (("an", an), ("sp", sp)):  # the two expiries in turn, in one process
                w, removed = wall(lambda: h.expire(cut))
                got[key]["walls"].append(w)
                got[key]["phases"].append(h.expire_ms())
                got[key]["removed"] = removed
                got[key]["after"] = h.info()
    for key, g in got.items():
        o = {"cutoff": cut, "removed": g["removed"], "before": g["before"], "after": g["after"], "wall_ms": summary(g["walls"])}
        for k in PHASES:
            o[k + "_ms"] = summary(x[k] for x in g["phases"])
        o["device_ms"] = summary(sum(x.values()) for x in g["phases"])
        res[key] = o
    return res


def rate(nbytes, d):
    """bytes/s of a phase as {median, min, max} in TB/s (the slowest run gives the minimum); None when the phase ran nothing."""
    if d["median"] <= 0 or d["max"] <= 0 or d["min"] <= 0:
        return None
    return {"median": nbytes / (d["median"] * 1e-3) / 1e12, "min": nbytes / (d["max"] * 1e-3) / 1e12, "max": nbytes / (d["min"] * 1e-3) / 1e12}


def report(outdir: Path):
    parts = {c: json.loads((outdir / f"part_{c}.json").read_text()) for c in CASES if (outdir / f"part_{c}.json").exists()}
    if not parts:
        raise SystemExit("no part_<case>.json to report")
    head = next(iter(parts.values()))
    fmt = lambda d: f"{d['median']:9.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    tbs = lambda r: "        -" if r is None else f"{r['median']:6.2f} [{r['min']:.2f}, {r['max']:.2f}] TB/s"  # noqa: E731
    lines = [f"annot_expire_measure: {head['records']} entries in each store, {head['traces']} traces, S = {head['services']}, seed {head['seed']}, "
             f"{head['device']}; device ms, median [min, max] of {head['runs']} runs, first call apart",
             " zk_an_expire and zk_sp_expire in turn in one process, the same cutoff; TB/s from each phase's own bytes"]
    for c, part in parts.items():
        lines.append(f" {TITLES[c]}")
        for key in ("an", "sp"):
            o, B = part[key], BYTES[key]
            e = o["before"]["entries"]
            # half: the one segment is mixed; sorted: at most one of 64, counted as one whole segment; none: nothing is rewritten
            mixed = e if c == "half" else e // K if c == "sorted" else 0
            surv = o["after"]["entries"] if c == "half" else mixed
            o["ends_bytes"] = e * (B["fold"] + B["mark"]) + e // 8 + table_bytes(e)
            o["rewrite_bytes"] = 2 * (mixed // 8) + surv * (B["read"] + B["write"])
            o["ends_tbs"], o["rewrite_tbs"] = rate(o["ends_bytes"], o["ends_ms"]), rate(o["rewrite_bytes"], o["rewrite_ms"]) if mixed else None
            lines += [f"  {NAMES[key]}: {e} entries in {o['before']['segments']} segment(s), {o['before']['bytes'] / 2**20:.0f} MiB"
                      f" -> {o['after']['entries']} in {o['after']['segments']}, {o['after']['bytes'] / 2**20:.0f} MiB; removed {o['removed']}",
                      f"   ends    ({B['fold']} + {B['mark']} B/entry read, tables cleared)   {fmt(o['ends_ms'])}   {tbs(o['ends_tbs'])}",
                      f"   sizing sync                                  {fmt(o['size_ms'])}",
                      f"   rewrite ({B['read']} B/survivor read, {B['write']} B written)     {fmt(o['rewrite_ms'])}   {tbs(o['rewrite_tbs'])}"
                      + (" (at most: the bytes of one whole segment)" if c == "sorted" else ""),
                      f"   device sum                                   {fmt(o['device_ms'])}",
                      f"   wall, sync (scratch and old segments freed)  {fmt(o['wall_ms'])}"]
        an, sp = part["an"], part["sp"]
        ratios = [f"ends {an['ends_ms']['median'] / sp['ends_ms']['median']:.3f} (by bytes {an['ends_bytes'] / sp['ends_bytes']:.3f})"]
        if sp["rewrite_ms"]["median"] > 0 and an["rewrite_bytes"]:
            ratios.append(f"rewrite {an['rewrite_ms']['median'] / sp['rewrite_ms']['median']:.3f} (by bytes {an['rewrite_bytes'] / sp['rewrite_bytes']:.3f})")
        lines.append("  annotations / spans, median device ms: " + ", ".join(ratios))
    missing = [c for c in CASES if c not in parts]
    if missing:
        lines.append(" not measured: " + ", ".join(TITLES[c] for c in missing))
    res = {"records": head["records"], "traces": head["traces"], "services": head["services"], "seed": head["seed"],
           "device": head["device"], "runs": head["runs"], "not_measured": missing}
    for c, part in parts.items():
        res[c] = {"an": part["an"], "sp": part["sp"]}
    (outdir / "measure.json").write_text(json.dumps(res, indent=1) + "\n")
    (outdir / "measure.txt").write_text("\n".join(lines) + "\n")
    for c in parts:
        (outdir / f"part_{c}.json").unlink()
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--report", action="store_true", help="join the cases' parts into measure.json and measure.txt")
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--services", type=int, default=500)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "annot_expire"))
    a = ap.parse_args()
    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    if a.report:
        return report(outdir)
    if not a.case:
        raise SystemExit("--case half|sorted|none, or --report")
    res = run_case(a)
    (outdir / f"part_{a.case}.json").write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
