#!/usr/bin/env python3
"""Measurement of the trace-id index by service and span name, recorded, not gated: no
number here has an earlier one to compare with, and bench.py does not run it.

Workload: the C2 batch on the device (bench.py's: --records 1e8, S = 500, seed 2); TraceGen gives no span
names, so name ids 1..--names are written into bits 16..31 of flags from the span id. Reported as the
median and range of --runs runs, the first call apart:
  - zk_ix_observe by pass (zk_ix_observe_ms: count, sizing sync, scatter) into an emptied index,
    alternating with zk_td_observe on the same batch in the same process; each pass's share of
    --peak-tbs TB/s from its own bytes: the count reads 8 B per record; the scatter reads 24 B per record
    once and 8 B of them (service_id, flags) a second time, and writes 18 B per indexed record;
  - zk_ix_trace_ids (zk_ix_query_ms: the handle's stream from the first pass to the last copy) for the
    largest and a median service, limit 100 and 4096, with and without a name, over one segment and
    over 64 segments of the same entries, with the bytes of the service's slices (18 B per entry) and
    the share of peak that three reads of them (the bound of DESIGN.md §5e) in that time come to;
  - zk_ix_compact of 64 segments (wall time: the call synchronises).
Writes <out>/measure.json and <out>/measure.txt. Needs a gfx950 device."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SLICE_READS = 3     # zk_ix_trace_ids reads the service's slices at most three times (include/zkindex.h)
ENTRY_BYTES = 18
COUNT_READ, SCATTER_READ, SCATTER_WRITE = 8, 32, 18  # bytes per record (per indexed record for the write)
INT64_MAX = 2 ** 63 - 1


def summary(xs):
    xs = list(xs)
    return {"first": xs[0], "median": statistics.median(xs[1:]), "min": min(xs[1:]), "max": max(xs[1:]), "runs": len(xs) - 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--services", type=int, default=500)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--names", type=int, default=7)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="the HBM bandwidth the shares are of, TB/s")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "trace_index"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from zipkin_amd import DepsContext, DeviceColumns, TraceDurationIndex, TraceNameIndex, tracegen_params

    if not torch.cuda.is_available():
        raise SystemExit("trace_index_measure needs a HIP device")
    S = a.services
    ctx = DepsContext(S, device=0)
    p = tracegen_params(a.seed, int(a.records / 15) + 1000, target_records=a.records, max_depth=a.max_depth,
                        num_services=S)
    cols = DeviceColumns(a.records, device="cuda:0")
    n, ntr = ctx.tracegen_device(p, cols)
    ctx.sync()
    ctx.close()
    cols = cols.slice(0, n)
    name = (torch.remainder(cols.span_id, a.names) + 1).to(torch.int32) << 16
    cols.flags.copy_((cols.flags & 0xFFFF) | name)
    del name
    torch.cuda.synchronize()
    peak = a.peak_tbs * 1e12
    res = {"records": n, "traces": ntr, "services": S, "names": a.names, "seed": a.seed,
           "device": torch.cuda.get_device_name(0), "peak_tbs": a.peak_tbs, "slice_reads_counted": SLICE_READS}
    runs = a.runs + 1

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def many_segments(h, k=64):
        h.reset()
        for j in range(k):
            h.observe(cols.slice(j * n // k, (j + 1) * n // k), sync=False)
        return h.info()

    with TraceNameIndex(S, device=0, timing=True) as ix, TraceNameIndex(S, device=0, timing=True) as ix64, \
            TraceDurationIndex(device=0, timing=True) as td:
        ix.observe(cols)
        td.observe(cols)
        res["index"] = ix.info()
        entries = res["index"]["entries"]
        walls, phases, td_walls, td_phases = [], [], [], []
        for _ in range(runs):  # the two alternate, so that whatever else the machine does meets both
            ix.reset()
            walls.append(wall(lambda: ix.observe(cols, sync=False)))
            phases.append(ix.observe_ms())
            td.reset()
            td_walls.append(wall(lambda: td.observe(cols, sync=False)))
            td_phases.append(td.observe_ms())
        o = {"wall_ms": summary(walls)}
        for k in ix.OBSERVE_PHASES:
            o[k + "_ms"] = summary(x[k] for x in phases)
        o["device_ms"] = summary(sum(x.values()) for x in phases)
        o["count_share_of_peak"] = n * COUNT_READ / (o["count_ms"]["median"] * 1e-3) / peak
        o["scatter_bytes"] = n * SCATTER_READ + entries * SCATTER_WRITE
        o["scatter_share_of_peak"] = o["scatter_bytes"] / (o["scatter_ms"]["median"] * 1e-3) / peak
        res["ix_observe"] = o
        t = {"wall_ms": summary(td_walls), "device_ms": summary(sum(x.values()) for x in td_phases)}
        for k in td.OBSERVE_PHASES:
            t[k + "_ms"] = summary(x[k] for x in td_phases)
        res["td_observe"] = t

        counts = ix.service_counts()
        order = np.argsort(counts, kind="stable")
        picks = {"largest": int(order[-1]), "median": int(order[len(order) // 2])}
        res["index64"] = many_segments(ix64)
        res["queries"] = {}
        for label, svc in picks.items():
            slice_bytes = int(counts[svc]) * ENTRY_BYTES
            for segs, h in (("1seg", ix), ("64seg", ix64)):
                for nm in (None, 1):
                    for limit in (100, 4096):
                        ws, dev = [], []
                        for _ in range(runs):
                            ws.append(wall(lambda: h.getTraceIdsByName(svc, nm, INT64_MAX, limit)))
                            dev.append(h.query_ms())
                        d = {"service": svc, "entries": int(counts[svc]), "slice_bytes": slice_bytes, "matched": h.matched,
                             "stream_ms": summary(dev), "wall_ms": summary(ws)}
                        d["share_of_peak"] = SLICE_READS * slice_bytes / (d["stream_ms"]["median"] * 1e-3) / peak
                        res["queries"][f"{label}_{segs}_{'name' if nm else 'any'}_limit{limit}"] = d

        cw = []
        for _ in range(runs):
            many_segments(ix64)
            cw.append(wall(ix64.compact))
        res["compact64"] = {"wall_ms": summary(cw), "bytes_moved": 2 * entries * ENTRY_BYTES}
        res["compact64"]["share_of_peak"] = res["compact64"]["bytes_moved"] / (res["compact64"]["wall_ms"]["median"] * 1e-3) / peak

    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "measure.json").write_text(json.dumps(res, indent=1) + "\n")
    fmt = lambda d: f"{d['median']:9.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    o, t = res["ix_observe"], res["td_observe"]
    lines = [f"trace_index_measure: {n} records, {ntr} traces, S = {S}, {a.names} names, seed {a.seed}, {res['device']}; "
             f"ms, median [min, max] of {a.runs} runs, first call apart",
             f" index: {entries} entries, {res['index']['bytes'] / 2**20:.0f} MiB in one segment; "
             f"share of {a.peak_tbs:g} TB/s from each pass's own bytes",
             " zk_ix_observe into an emptied index (alternating with zk_td_observe, emptied table)",
             f"  count   ( 8 B/record read)              {fmt(o['count_ms'])}   {100 * o['count_share_of_peak']:.1f} %",
             f"  sizing sync                             {fmt(o['size_ms'])}",
             f"  scatter (32 B/record read, 18 B/entry)  {fmt(o['scatter_ms'])}   {100 * o['scatter_share_of_peak']:.1f} %",
             f"  device sum                              {fmt(o['device_ms'])}",
             f"  wall, sync                              {fmt(o['wall_ms'])}",
             f"  zk_td_observe: runs {fmt(t['runs_ms'])}",
             f"  zk_td_observe: grow {fmt(t['grow_ms'])}",
             f"  zk_td_observe: insert {fmt(t['insert_ms'])}",
             f"  zk_td_observe: device sum {fmt(t['device_ms'])}",
             f" zk_ix_trace_ids, end_ts = INT64_MAX (share = {SLICE_READS} reads of the service's slices in the stream time)"]
    for key, d in res["queries"].items():
        lines.append(f"  {key:<32} {d['entries']:>9} entries {d['slice_bytes'] / 2**20:7.1f} MiB  matched {d['matched']:>9}  "
                     f"stream {fmt(d['stream_ms'])}   {100 * d['share_of_peak']:.2f} %   wall {fmt(d['wall_ms'])}")
    c = res["compact64"]
    lines.append(f" zk_ix_compact of 64 segments ({res['index64']['entries']} entries): wall {fmt(c['wall_ms'])}   "
                 f"{100 * c['share_of_peak']:.1f} % (18 B read + 18 B written per entry)")
    (outdir / "measure.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
