#!/usr/bin/env python3
"""Measurement of the trace-id index by annotation, recorded, not gated: no number here
has an earlier one to compare with, and bench.py does not run it.

Workload: one entry per record of the C2 batch on the device (bench.py's: --records 1e8, S = 500, seed 2):
service and traceId are the record's, ts its last timestamp, the key one of --keys hashes drawn from the
span id, val 0 (a time entry) for every second entry and else one of --values odd hashes. No decoder
produces device entries yet, so the entries are synthetic; their number, their service
skew and their timestamps are the batch's. Reported as the median and range of --runs runs, the first
call apart:
  - zk_ax_observe by pass (zk_ax_observe_ms: count, sizing sync, scatter) into an emptied index,
    alternating with zk_ix_observe of the batch's records in the same process; each pass's share of
    --peak-tbs TB/s from its own bytes: the count reads 4 B per entry; the scatter reads 36 B per entry
    once and the service (4 B) a second time, and writes 32 B per entry;
  - zk_ax_trace_ids (zk_ax_query_ms: the handle's stream from the first pass to the last copy) for the
    largest and a median service, limit 100 and 4096, with val any and fixed, over one segment and over
    64 segments of the same entries, with the bytes one read of the service's slices touches (8 B of key
    per entry, 8 B of val per key match when a value is asked, 16 B per match) and the share of peak that
    three such reads (the bound of DESIGN.md §5f) in that time come to.
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

SLICE_READS = 3      # zk_ax_trace_ids reads the service's slices at most three times (include/zkannindex.h)
ENTRY_BYTES = 32
COUNT_READ, SCATTER_READ, SCATTER_WRITE = 4, 40, 32            # bytes per entry
IX_COUNT_READ, IX_SCATTER_READ, IX_SCATTER_WRITE = 8, 32, 18   # zk_ix_observe's (tools/trace_index_measure.py)
INT64_MAX = 2 ** 63 - 1
GOLDEN = 0x9E3779B97F4A7C15 - (1 << 64)  # an odd 64-bit multiplier, as int64


def summary(xs):
    xs = list(xs)
    return {"first": xs[0], "median": statistics.median(xs[1:]), "min": min(xs[1:]), "max": max(xs[1:]), "runs": len(xs) - 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--services", type=int, default=500)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--keys", type=int, default=16)
    ap.add_argument("--values", type=int, default=4)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="the HBM bandwidth the shares are of, TB/s")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ann_index"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from zipkin_amd import DepsContext, DeviceAnnotationItems, DeviceColumns, TraceAnnotationIndex, TraceNameIndex, tracegen_params

    if not torch.cuda.is_available():
        raise SystemExit("ann_index_measure needs a HIP device")
    S = a.services
    ctx = DepsContext(S, device=0)
    p = tracegen_params(a.seed, int(a.records / 15) + 1000, target_records=a.records, max_depth=a.max_depth,
                        num_services=S)
    cols = DeviceColumns(a.records, device="cuda:0")
    n, ntr = ctx.tracegen_device(p, cols)
    ctx.sync()
    ctx.close()
    cols = cols.slice(0, n)
    sid = cols.span_id
    key = (torch.remainder(sid, a.keys) + 1) * GOLDEN
    vsel = torch.remainder(sid >> 8, 2 * a.values)  # even: a time entry; odd v: the value hash v * GOLDEN | 1
    val = torch.where(vsel % 2 == 0, torch.zeros_like(sid), (vsel * GOLDEN) | 1)
    items = DeviceAnnotationItems(cols.service_id, key, val, cols.last_ts, cols.trace_id)
    del vsel
    torch.cuda.synchronize()
    q_key, q_val = GOLDEN, GOLDEN | 1  # the key of span ids = 0 mod keys, the first value hash
    peak = a.peak_tbs * 1e12
    res = {"entries": n, "records": n, "traces": ntr, "services": S, "keys": a.keys, "values": a.values, "seed": a.seed,
           "device": torch.cuda.get_device_name(0), "peak_tbs": a.peak_tbs, "slice_reads_counted": SLICE_READS,
           "entry_bytes": ENTRY_BYTES}
    runs = a.runs + 1

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def part(j, k):
        lo, hi = j * n // k, (j + 1) * n // k
        return DeviceAnnotationItems(items.service[lo:hi], items.key[lo:hi], items.val[lo:hi], items.ts[lo:hi], items.trace_id[lo:hi])

    with TraceAnnotationIndex(S, device=0, timing=True) as ax, TraceAnnotationIndex(S, device=0, timing=True) as ax64, \
            TraceNameIndex(S, device=0, timing=True) as ix:
        ax.observe(items)
        ix.observe(cols)
        res["index"] = ax.info()
        res["ix_index"] = ix.info()
        walls, phases, ix_walls, ix_phases = [], [], [], []
        for _ in range(runs):  # the two alternate, so that whatever else the machine does meets both
            ax.reset()
            walls.append(wall(lambda: ax.observe(items, sync=False)))
            phases.append(ax.observe_ms())
            ix.reset()
            ix_walls.append(wall(lambda: ix.observe(cols, sync=False)))
            ix_phases.append(ix.observe_ms())

        def observe_summary(ws, ph, names, entries, cr, sr, sw):
            o = {"wall_ms": summary(ws)}
            for k in names:
                o[k + "_ms"] = summary(x[k] for x in ph)
            o["device_ms"] = summary(sum(x.values()) for x in ph)
            o["count_share_of_peak"] = n * cr / (o["count_ms"]["median"] * 1e-3) / peak
            o["scatter_bytes"] = n * sr + entries * sw
            o["scatter_share_of_peak"] = o["scatter_bytes"] / (o["scatter_ms"]["median"] * 1e-3) / peak
            return o

        res["ax_observe"] = observe_summary(walls, phases, ax.OBSERVE_PHASES, n, COUNT_READ, SCATTER_READ, SCATTER_WRITE)
        res["ix_observe"] = observe_summary(ix_walls, ix_phases, ix.OBSERVE_PHASES, res["ix_index"]["entries"], IX_COUNT_READ,
                                            IX_SCATTER_READ, IX_SCATTER_WRITE)

        counts = ax.service_counts()
        order = np.argsort(counts, kind="stable")
        picks = {"largest": int(order[-1]), "median": int(order[len(order) // 2])}
        for j in range(64):
            ax64.observe(part(j, 64), sync=False)
        res["index64"] = ax64.info()
        res["queries"] = {}
        for label, svc in picks.items():
            key_matched = ax.trace_ids(svc, q_key, 0, INT64_MAX, 1)[1]
            for segs, h in (("1seg", ax), ("64seg", ax64)):
                for vlabel, v in (("any", 0), ("value", q_val)):
                    for limit in (100, 4096):
                        ws, dev, matched = [], [], 0
                        for _ in range(runs):
                            ws.append(wall(lambda: h.trace_ids(svc, q_key, v, INT64_MAX, limit)))
                            dev.append(h.query_ms())
                        matched = h.trace_ids(svc, q_key, v, INT64_MAX, limit)[1]
                        read = int(counts[svc]) * 8 + (key_matched * 8 if v else 0) + matched * 16
                        d = {"service": svc, "entries": int(counts[svc]), "slice_bytes": int(counts[svc]) * ENTRY_BYTES,
                             "key_matched": key_matched, "matched": matched, "bytes_per_read": read,
                             "stream_ms": summary(dev), "wall_ms": summary(ws)}
                        d["share_of_peak"] = SLICE_READS * read / (d["stream_ms"]["median"] * 1e-3) / peak
                        res["queries"][f"{label}_{segs}_{vlabel}_limit{limit}"] = d

    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "measure.json").write_text(json.dumps(res, indent=1) + "\n")
    fmt = lambda d: f"{d['median']:9.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    o, t = res["ax_observe"], res["ix_observe"]
    lines = [f"ann_index_measure: {n} entries (one per record), {ntr} traces, S = {S}, {a.keys} keys, {a.values} values, seed {a.seed}, "
             f"{res['device']}; ms, median [min, max] of {a.runs} runs, first call apart",
             f" index: {res['index']['entries']} entries, {res['index']['bytes'] / 2**20:.0f} MiB in one segment, {ENTRY_BYTES} B per entry; "
             f"share of {a.peak_tbs:g} TB/s from each pass's own bytes",
             " zk_ax_observe into an emptied index (alternating with zk_ix_observe of the batch's records, emptied index)",
             f"  count   ( 4 B/entry read)               {fmt(o['count_ms'])}   {100 * o['count_share_of_peak']:.1f} %",
             f"  sizing sync                             {fmt(o['size_ms'])}",
             f"  scatter (40 B/entry read, 32 B written) {fmt(o['scatter_ms'])}   {100 * o['scatter_share_of_peak']:.1f} %",
             f"  device sum                              {fmt(o['device_ms'])}",
             f"  wall, sync                              {fmt(o['wall_ms'])}",
             f"  zk_ix_observe: count   ( 8 B/record read)              {fmt(t['count_ms'])}   {100 * t['count_share_of_peak']:.1f} %",
             f"  zk_ix_observe: sizing sync                             {fmt(t['size_ms'])}",
             f"  zk_ix_observe: scatter (32 B/record read, 18 B/entry)  {fmt(t['scatter_ms'])}   {100 * t['scatter_share_of_peak']:.1f} %",
             f"  zk_ix_observe: device sum ({res['ix_index']['entries']} entries)          {fmt(t['device_ms'])}",
             f"  zk_ix_observe: wall, sync                              {fmt(t['wall_ms'])}",
             f" zk_ax_trace_ids, end_ts = INT64_MAX (share = {SLICE_READS} reads of what one read of the service's slices touches, "
             "in the stream time)"]
    for k, d in res["queries"].items():
        lines.append(f"  {k:<34} {d['entries']:>9} entries {d['bytes_per_read'] / 2**20:7.2f} MiB/read  matched {d['matched']:>8}  "
                     f"stream {fmt(d['stream_ms'])}   {100 * d['share_of_peak']:.2f} %   wall {fmt(d['wall_ms'])}")
    (outdir / "measure.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
