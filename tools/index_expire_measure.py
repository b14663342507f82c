#!/usr/bin/env python3
"""Measurement of index retention, recorded, not gated: no number here has an earlier one
to compare with, and bench.py does not run it.

Workload: the C2 batch on the device (bench.py's: --records 1e8, S = 500, seed 2) as 64 segments of the
trace-id index by service and span name; the cutoff is the median last_ts, so half of the entries expire.
Reported as the median and range of --runs runs, the first call apart, by pass (zk_ix_expire_ms: count,
sizing sync, rewrite), with each pass's share of --peak-tbs TB/s from its own bytes: the count reads 8 B
per entry of every segment; the rewrite reads 8 B per entry of the mixed segments again, 10 B more per
survivor of them, and writes 18 B per survivor.
  --case a    one merged segment, half expiring;
  --case b    64 time-sorted segments (the batch sorted by last_ts): at most one is mixed;
  --case c    64 segments in the batch's own order, each half expiring; beside it zk_ix_compact on the
              same 64-segment index in the same process (wall time: both calls synchronise);
  --case td   zk_td_expire on the same batch's table with half the traces expiring (cutoff: the median
              trace end), beside the grow phase of a zk_td_observe that rehashes (the second half of the
              batch observed after the first).
Every case is a process of its own, so that each runs under its own time limit, chained with &&:
  for c in a b c td; do timeout -k 10 300 python tools/index_expire_measure.py --case $c || exit 1; done &&
  python tools/index_expire_measure.py --report
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

CASES = ("a", "b", "c", "td")
COUNT_READ, AGAIN_READ, SURVIVOR_READ, SURVIVOR_WRITE = 8, 8, 10, 18  # bytes per entry (see above)
ENTRY_BYTES = 18
SLOT_BYTES = 24
K = 64
TITLES = {"a": "(a) one merged segment, half expiring",
          "b": "(b) 64 time-sorted segments, at most one mixed",
          "c": "(c) 64 segments in the batch's order, each half expiring"}


def summary(xs):
    xs = list(xs)
    return {"first": xs[0], "median": statistics.median(xs[1:]), "min": min(xs[1:]), "max": max(xs[1:]), "runs": len(xs) - 1}


def run_case(a):
    import torch

    from zipkin_amd import DepsContext, DeviceColumns, TraceDurationIndex, TraceNameIndex, tracegen_params

    if not torch.cuda.is_available():
        raise SystemExit("index_expire_measure needs a HIP device")
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
           "peak_tbs": a.peak_tbs, "runs": a.runs}
    runs = a.runs + 1

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    if a.case == "td":
        timed = (cols.flags & 2) != 0
        _, inv = torch.unique(cols.trace_id, return_inverse=True)
        ends = torch.full((int(inv.max()) + 1,), -2 ** 63, dtype=torch.int64, device=inv.device)
        ends.scatter_reduce_(0, inv[timed], cols.last_ts[timed], "amax")
        cut = int(ends[ends > -2 ** 63].median()) + 1
        del inv, ends, timed
        walls, phases, grows = [], [], []
        with TraceDurationIndex(device=0, timing=True) as td:
            for _ in range(runs):
                td.reset()
                td.observe(cols)
                before = td.info()
                w, removed = wall(lambda: td.expire(cut))
                walls.append(w)
                phases.append(td.expire_ms())
                after = td.info()
        for _ in range(runs):  # a rehash to set it beside: the second half grows the table of the first
            with TraceDurationIndex(device=0, timing=True) as td:
                td.observe(cols.slice(0, n // 2))
                half = td.info()
                td.observe(cols.slice(n // 2, n))
                grows.append(td.observe_ms()["grow"])
                full = td.info()
        o = {"cutoff": cut, "removed": removed, "before": before, "after": after, "wall_ms": summary(walls)}
        for k in TraceDurationIndex.EXPIRE_PHASES:
            o[k + "_ms"] = summary(x[k] for x in phases)
        o["count_bytes"] = (before["slots"] + 1) * 16
        o["rebuild_bytes"] = (after["slots"] + 1) * SLOT_BYTES + (before["slots"] + 1) * SLOT_BYTES + after["traces"] * SLOT_BYTES
        o["count_share_of_peak"] = o["count_bytes"] / (o["count_ms"]["median"] * 1e-3) / peak
        o["rebuild_share_of_peak"] = o["rebuild_bytes"] / (o["rebuild_ms"]["median"] * 1e-3) / peak
        o["observe_rehash"] = {"grow_ms": summary(grows), "from": half, "to": full}
        res["td_expire"] = o
        return res

    cut = int(cols.last_ts.median())
    if a.case == "b":  # the batch in time order: a segment is then all old, all new, or the one in between
        perm = torch.argsort(cols.last_ts)
        for k in ("trace_id", "span_id", "parent_id", "first_ts", "last_ts", "service_id", "flags"):
            getattr(cols, k).copy_(getattr(cols, k)[perm])
        del perm
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
    with TraceNameIndex(S, device=0, timing=True) as ix:
        for _ in range(runs):
            before = fill(ix)
            w, removed = wall(lambda: ix.expire(cut))
            walls.append(w)
            phases.append(ix.expire_ms())
            after = ix.info()
            if a.case == "c":
                fill(ix)
                compacts.append(wall(ix.compact)[0])
    o = {"cutoff": cut, "removed": removed, "before": before, "after": after, "wall_ms": summary(walls)}
    for k in TraceNameIndex.EXPIRE_PHASES:
        o[k + "_ms"] = summary(x[k] for x in phases)
    o["device_ms"] = summary(sum(x.values()) for x in phases)
    o["count_bytes"] = before["entries"] * COUNT_READ
    o["count_share_of_peak"] = o["count_bytes"] / (o["count_ms"]["median"] * 1e-3) / peak
    res["ix_expire"] = o
    if a.case == "c":
        c = {"wall_ms": summary(compacts), "bytes_moved": 2 * before["entries"] * ENTRY_BYTES}
        c["share_of_peak"] = c["bytes_moved"] / (c["wall_ms"]["median"] * 1e-3) / peak
        res["compact64"] = c
    return res


def rewrite_bytes(o, mixed_entries):
    return mixed_entries * AGAIN_READ + o["after"]["entries"] * (SURVIVOR_READ + SURVIVOR_WRITE)


def report(outdir: Path):
    parts = {c: json.loads((outdir / f"part_{c}.json").read_text()) for c in CASES}
    head = parts["a"]
    peak = head["peak_tbs"] * 1e12
    fmt = lambda d: f"{d['median']:9.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    lines = [f"index_expire_measure: {head['records']} records, {head['traces']} traces, S = {head['services']}, seed {head['seed']}, "
             f"{head['device']}; ms, median [min, max] of {head['runs']} runs, first call apart",
             f" zk_ix_expire at the median last_ts; share of {head['peak_tbs']:g} TB/s from each pass's own bytes"]
    for c in ("a", "b", "c"):
        o = parts[c]["ix_expire"]
        # (a), (c): every segment is mixed; (b): at most one of 64
        mixed = o["before"]["entries"] if c != "b" else o["before"]["entries"] // K
        o["rewrite_bytes"] = rewrite_bytes(o, mixed) if c != "b" else mixed * (AGAIN_READ + SURVIVOR_READ + SURVIVOR_WRITE)
        o["rewrite_share_of_peak"] = o["rewrite_bytes"] / (o["rewrite_ms"]["median"] * 1e-3) / peak if o["rewrite_ms"]["median"] > 0 else 0.0
        lines += [f" {TITLES[c]}: {o['before']['entries']} entries in {o['before']['segments']} segment(s), {o['before']['bytes'] / 2**20:.0f} MiB"
                  f" -> {o['after']['entries']} in {o['after']['segments']}, {o['after']['bytes'] / 2**20:.0f} MiB; removed {o['removed']}",
                  f"  count   (8 B/entry read)                        {fmt(o['count_ms'])}   {100 * o['count_share_of_peak']:.1f} %",
                  f"  sizing sync                                     {fmt(o['size_ms'])}",
                  f"  rewrite (8 B/entry + 10 B/survivor, 18 B written) {fmt(o['rewrite_ms'])}   {100 * o['rewrite_share_of_peak']:.1f} %"
                  + (" (at most: the bytes of one whole segment)" if c == "b" else ""),
                  f"  device sum                                      {fmt(o['device_ms'])}",
                  f"  wall, sync                                      {fmt(o['wall_ms'])}"]
    k = parts["c"]["compact64"]
    ratio = parts["c"]["ix_expire"]["wall_ms"]["median"] / k["wall_ms"]["median"]
    lines.append(f"  zk_ix_compact of the same 64 segments, same process: wall {fmt(k['wall_ms'])}   {100 * k['share_of_peak']:.1f} % "
                 f"(18 B read + 18 B written per entry); expire (c) / compact = {ratio:.2f}")
    t = parts["td"]["td_expire"]
    g = t["observe_rehash"]
    lines += [f" zk_td_expire at the median trace end: {t['before']['traces']} traces in {t['before']['slots']} slots -> "
              f"{t['after']['traces']} in {t['after']['slots']}; removed {t['removed']}",
              f"  count   (16 B/slot read)                        {fmt(t['count_ms'])}   {100 * t['count_share_of_peak']:.1f} %",
              f"  sizing sync                                     {fmt(t['size_ms'])}",
              f"  rebuild (clear + 24 B/slot read + 24 B/survivor) {fmt(t['rebuild_ms'])}   {100 * t['rebuild_share_of_peak']:.1f} %",
              f"  wall, sync                                      {fmt(t['wall_ms'])}",
              f"  zk_td_observe's grow phase when it rehashes {g['from']['traces']} traces from {g['from']['slots']} into "
              f"{g['to']['slots']} slots: {fmt(g['grow_ms'])}"]
    res = {"records": head["records"], "traces": head["traces"], "services": head["services"], "seed": head["seed"],
           "device": head["device"], "peak_tbs": head["peak_tbs"], "runs": head["runs"],
           "a": parts["a"]["ix_expire"], "b": parts["b"]["ix_expire"], "c": parts["c"]["ix_expire"],
           "compact64": k, "expire_c_over_compact": ratio, "td_expire": t}
    (outdir / "measure.json").write_text(json.dumps(res, indent=1) + "\n")
    (outdir / "measure.txt").write_text("\n".join(lines) + "\n")
    for c in CASES:
        (outdir / f"part_{c}.json").unlink()
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--report", action="store_true", help="join the four cases' parts into measure.json and measure.txt")
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--services", type=int, default=500)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="the HBM bandwidth the shares are of, TB/s")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "index_expire"))
    a = ap.parse_args()
    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    if a.report:
        return report(outdir)
    if not a.case:
        raise SystemExit("--case a|b|c|td, or --report")
    res = run_case(a)
    (outdir / f"part_{a.case}.json").write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
