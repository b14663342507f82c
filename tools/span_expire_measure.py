#!/usr/bin/env python3
"""Measurement of the span store's expiry, recorded, not gated: no number here has an
earlier one to compare with, and bench.py does not run it.

Workload: the C2 batch on the device (bench.py's: --records 1e8, S = 500, seed 2) in a TraceSpanStore; the
cutoff is the median trace end, so about half of the traces expire, whole. Reported as the median and range
of --runs runs, the first call apart, by pass (zk_sp_expire_ms: ends, sizing sync, rewrite), with each
pass's share of --peak-tbs TB/s from its own bytes: the end-table passes clear 16 B per slot of every
range's table, read 20 B per entry (fold) and 8 B per entry again (mark) and write 1 bit per entry; the
rewrite reads 1 bit per entry of the mixed segments, 56 B per survivor of them (trace_id twice), and
writes 48 B per survivor.
  --case a    one merged segment;
  --case b    64 time-sorted segments (the batch sorted by its records' trace end): at most one is mixed;
  --case c    64 segments in the batch's own order, each about half expiring; beside it zk_sp_compact on the
              same 64-segment store in the same process (wall time: both calls synchronise).
Every case is a process of its own, so that each runs under its own time limit, chained with &&:
  for c in a b c; do timeout -k 10 300 python tools/span_expire_measure.py --case $c || exit 1; done &&
  python tools/span_expire_measure.py --report
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

CASES = ("a", "b", "c")
FOLD_READ, MARK_READ, SLOT_BYTES = 20, 8, 16
SURVIVOR_READ, SURVIVOR_WRITE, ENTRY_BYTES = 56, 48, 48
CHUNK = 1 << 24  # zk_sp_config.expire_chunk's default
BUCKETS = 4096
K = 64
TITLES = {"a": "(a) one merged segment",
          "b": "(b) 64 time-sorted segments, at most one mixed",
          "c": "(c) 64 segments in the batch's order, each about half expiring"}


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

    from zipkin_amd import DepsContext, DeviceColumns, TraceSpanStore, tracegen_params

    if not torch.cuda.is_available():
        raise SystemExit("span_expire_measure needs a HIP device")
    S = a.services
    ctx = DepsContext(S, device=0)
    p = tracegen_params(a.seed, int(a.records / 15) + 1000, target_records=a.records, max_depth=a.max_depth, num_services=S)
    cols = DeviceColumns(a.records, device="cuda:0")
    n, ntr = ctx.tracegen_device(p, cols)
    ctx.sync()
    ctx.close()
    cols = cols.slice(0, n)
    torch.cuda.synchronize()
    peak = a.peak_tbs * 1e12
    res = {"case": a.case, "records": n, "traces": ntr, "services": S, "seed": a.seed, "device": torch.cuda.get_device_name(0),
           "peak_tbs": a.peak_tbs, "runs": a.runs, "chunk": a.chunk}
    runs = a.runs + 1

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    # every trace's end, and the cutoff: the median end over the traces with a timed fragment
    timed = (cols.flags & 2) != 0
    _, inv = torch.unique(cols.trace_id, return_inverse=True)
    ends = torch.full((int(inv.max()) + 1,), -2 ** 63, dtype=torch.int64, device=inv.device)
    ends.scatter_reduce_(0, inv[timed], cols.last_ts[timed], "amax")
    cut = int(ends[ends > -2 ** 63].median()) + 1
    if a.case == "b":  # in the order of the records' trace ends: a segment is then all old, all new, or the one in between
        perm = torch.argsort(ends[inv])
        for k in ("trace_id", "span_id", "parent_id", "first_ts", "last_ts", "service_id", "flags"):
            getattr(cols, k).copy_(getattr(cols, k)[perm])
        del perm
    del inv, ends, timed
    torch.cuda.synchronize()

    def fill(h):
        h.reset()
        if a.case == "a":
            h.observe(cols, sync=False)
        else:
            for j in range(K):
                h.observe(cols.slice(j * n // K, (j + 1) * n // K), sync=False)
        return h.info()

    walls, phases, compacts = [], [], []
    with TraceSpanStore(device=0, timing=True, expire_chunk=a.chunk) as sp:
        for _ in range(runs):
            before = fill(sp)
            w, removed = wall(lambda: sp.expire(cut))
            walls.append(w)
            phases.append(sp.expire_ms())
            after = sp.info()
            if a.case == "c":
                fill(sp)
                compacts.append(wall(sp.compact)[0])
    o = {"cutoff": cut, "removed": removed, "before": before, "after": after, "wall_ms": summary(walls)}
    for k in TraceSpanStore.EXPIRE_PHASES:
        o[k + "_ms"] = summary(x[k] for x in phases)
    o["device_ms"] = summary(sum(x.values()) for x in phases)
    o["ends_bytes"] = before["entries"] * (FOLD_READ + MARK_READ) + before["entries"] // 8 + table_bytes(before["entries"])
    o["ends_share_of_peak"] = o["ends_bytes"] / (o["ends_ms"]["median"] * 1e-3) / peak
    res["sp_expire"] = o
    if a.case == "c":
        c = {"wall_ms": summary(compacts), "bytes_moved": 2 * before["entries"] * ENTRY_BYTES}
        c["share_of_peak"] = c["bytes_moved"] / (c["wall_ms"]["median"] * 1e-3) / peak
        res["compact64"] = c
    return res


def report(outdir: Path):
    parts = {c: json.loads((outdir / f"part_{c}.json").read_text()) for c in CASES}
    head = parts["a"]
    peak = head["peak_tbs"] * 1e12
    fmt = lambda d: f"{d['median']:9.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    lines = [f"span_expire_measure: {head['records']} records, {head['traces']} traces, S = {head['services']}, seed {head['seed']}, "
             f"{head['device']}; ms, median [min, max] of {head['runs']} runs, first call apart",
             f" zk_sp_expire at the median trace end; share of {head['peak_tbs']:g} TB/s from each pass's own bytes"]
    for c in CASES:
        o = parts[c]["sp_expire"]
        # (a), (c): every segment is mixed; (b): at most one of 64, counted as one whole segment
        mixed = o["before"]["entries"] if c != "b" else o["before"]["entries"] // K
        surv = o["after"]["entries"] if c != "b" else mixed
        o["rewrite_bytes"] = 2 * (mixed // 8) + surv * (SURVIVOR_READ + SURVIVOR_WRITE)
        o["rewrite_share_of_peak"] = o["rewrite_bytes"] / (o["rewrite_ms"]["median"] * 1e-3) / peak if o["rewrite_ms"]["median"] > 0 else 0.0
        lines += [f" {TITLES[c]}: {o['before']['entries']} entries in {o['before']['segments']} segment(s), {o['before']['bytes'] / 2**20:.0f} MiB"
                  f" -> {o['after']['entries']} in {o['after']['segments']}, {o['after']['bytes'] / 2**20:.0f} MiB; removed {o['removed']}",
                  f"  ends    (tables cleared, 20 + 8 B/entry read)       {fmt(o['ends_ms'])}   {100 * o['ends_share_of_peak']:.1f} %",
                  f"  sizing sync                                         {fmt(o['size_ms'])}",
                  f"  rewrite (56 B/survivor read, 48 B written)          {fmt(o['rewrite_ms'])}   {100 * o['rewrite_share_of_peak']:.1f} %"
                  + (" (at most: the bytes of one whole segment)" if c == "b" else ""),
                  f"  device sum                                          {fmt(o['device_ms'])}",
                  f"  wall, sync (scratch allocated and freed, old segments freed) {fmt(o['wall_ms'])}"]
    k = parts["c"]["compact64"]
    ratio = parts["c"]["sp_expire"]["wall_ms"]["median"] / k["wall_ms"]["median"]
    lines.append(f"  zk_sp_compact of the same 64 segments, same process: wall {fmt(k['wall_ms'])}   {100 * k['share_of_peak']:.1f} % "
                 f"(48 B read + 48 B written per entry); expire (c) / compact = {ratio:.2f}")
    res = {"records": head["records"], "traces": head["traces"], "services": head["services"], "seed": head["seed"],
           "device": head["device"], "peak_tbs": head["peak_tbs"], "runs": head["runs"],
           "a": parts["a"]["sp_expire"], "b": parts["b"]["sp_expire"], "c": parts["c"]["sp_expire"],
           "compact64": k, "expire_c_over_compact": ratio}
    (outdir / "measure.json").write_text(json.dumps(res, indent=1) + "\n")
    (outdir / "measure.txt").write_text("\n".join(lines) + "\n")
    for c in CASES:
        (outdir / f"part_{c}.json").unlink()
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--report", action="store_true", help="join the three cases' parts into measure.json and measure.txt")
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--services", type=int, default=500)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="the HBM bandwidth the shares are of, TB/s")
    ap.add_argument("--chunk", type=int, default=0, help="zk_sp_config.expire_chunk (0: the default)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "span_expire"))
    a = ap.parse_args()
    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    if a.report:
        return report(outdir)
    if not a.case:
        raise SystemExit("--case a|b|c, or --report")
    res = run_case(a)
    (outdir / f"part_{a.case}.json").write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
