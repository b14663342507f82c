#!/usr/bin/env python3
"""Measurement of the span store by trace id, recorded, not gated: no number here has an
earlier one to compare with, and bench.py does not run it.

Workload: the C2 batch on the device (bench.py's: --records 1e8, S = 500, seed 2), the batch the index
measurements use (tools/trace_index_measure.py). Reported as the median and range of --runs runs, the first
call apart:
  - zk_sp_observe by pass (zk_sp_observe_ms: count, sizing sync, scatter) into an emptied store,
    alternating with zk_ix_observe on the same batch in the same process (that code is the parent's); the
    rate in records/s and each pass's share of --peak-tbs TB/s from its own bytes: the count reads 8 B per
    record; the scatter reads 48 B per record and trace_id (8 B) a second time, and writes 48 B;
    zk_ix_observe's bytes are those of tools/trace_index_measure.py;
  - zk_sp_gather of 100 and of 4096 ids drawn from the batch (zk_sp_query_ms: the handle's stream from the
    count pass to the rows' copy; and the wall time of the call with the host's sort), over one segment and
    over 64 segments of the same records, with the bytes the passes move: 8 B per entry of the asked
    buckets' slices, twice, and 48 B read and written per matching row;
  - zk_sp_compact of 64 segments (wall time: the call synchronises; 48 B read and 48 B written per entry).
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

ROW_BYTES = 48
COUNT_READ, SCATTER_READ, SCATTER_WRITE = 8, 56, 48  # bytes per record
IX_COUNT_READ, IX_SCATTER_READ, IX_SCATTER_WRITE = 8, 32, 18  # zk_ix_observe's (per indexed record for the write)
SLICE_READS = 2  # the gather reads the asked buckets' trace_id slices in both passes


def summary(xs):
    xs = list(xs)
    return {"first": xs[0], "median": statistics.median(xs[1:]), "min": min(xs[1:]), "max": max(xs[1:]), "runs": len(xs) - 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--services", type=int, default=500)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="the HBM bandwidth the shares are of, TB/s")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "span_store"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from zipkin_amd import DepsContext, DeviceColumns, TraceNameIndex, TraceSpanStore, tracegen_params

    if not torch.cuda.is_available():
        raise SystemExit("span_store_measure needs a HIP device")
    S = a.services
    ctx = DepsContext(S, device=0)
    p = tracegen_params(a.seed, int(a.records / 15) + 1000, target_records=a.records, max_depth=a.max_depth,
                        num_services=S)
    cols = DeviceColumns(a.records, device="cuda:0")
    n, ntr = ctx.tracegen_device(p, cols)
    ctx.sync()
    ctx.close()
    cols = cols.slice(0, n)
    torch.cuda.synchronize()
    peak = a.peak_tbs * 1e12
    res = {"records": n, "traces": ntr, "services": S, "seed": a.seed, "device": torch.cuda.get_device_name(0),
           "peak_tbs": a.peak_tbs}
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

    # the asked ids: distinct trace ids of the batch, spread over it
    step = max(1, n // 4096)
    pick = cols.trace_id[::step][:8192].contiguous().cpu().numpy().view(np.uint64)
    pick = pick[np.sort(np.unique(pick, return_index=True)[1])][:4096]
    asks = {100: pick[:: max(1, len(pick) // 100)][:100].copy(), len(pick): pick}

    with TraceSpanStore(device=0, timing=True) as sp, TraceNameIndex(S, device=0, timing=True) as ix:
        sp.observe(cols)
        ix.observe(cols)
        res["store"] = sp.info()
        ix_entries = ix.info()["entries"]
        walls, phases, ix_walls, ix_phases = [], [], [], []
        for _ in range(runs):  # the two alternate, so that whatever else the machine does meets both
            sp.reset()
            walls.append(wall(lambda: sp.observe(cols, sync=False)))
            phases.append(sp.observe_ms())
            ix.reset()
            ix_walls.append(wall(lambda: ix.observe(cols, sync=False)))
            ix_phases.append(ix.observe_ms())
        o = {"wall_ms": summary(walls)}
        for k in sp.OBSERVE_PHASES:
            o[k + "_ms"] = summary(x[k] for x in phases)
        o["device_ms"] = summary(sum(x.values()) for x in phases)
        o["records_per_s"] = n / (o["device_ms"]["median"] * 1e-3)
        o["bytes"] = n * (COUNT_READ + SCATTER_READ + SCATTER_WRITE)
        o["bytes_per_s"] = o["bytes"] / (o["device_ms"]["median"] * 1e-3)
        o["share_of_peak"] = o["bytes_per_s"] / peak
        o["count_share_of_peak"] = n * COUNT_READ / (o["count_ms"]["median"] * 1e-3) / peak
        o["scatter_share_of_peak"] = n * (SCATTER_READ + SCATTER_WRITE) / (o["scatter_ms"]["median"] * 1e-3) / peak
        res["sp_observe"] = o
        t = {"wall_ms": summary(ix_walls), "device_ms": summary(sum(x.values()) for x in ix_phases), "entries": ix_entries}
        for k in ix.OBSERVE_PHASES:
            t[k + "_ms"] = summary(x[k] for x in ix_phases)
        t["bytes"] = n * (IX_COUNT_READ + IX_SCATTER_READ) + ix_entries * IX_SCATTER_WRITE
        t["bytes_per_s"] = t["bytes"] / (t["device_ms"]["median"] * 1e-3)
        t["share_of_peak"] = t["bytes_per_s"] / peak
        t["scatter_share_of_peak"] = (n * IX_SCATTER_READ + ix_entries * IX_SCATTER_WRITE) / (t["scatter_ms"]["median"] * 1e-3) / peak
        res["ix_observe"] = t
        ix.reset()

        res["gathers"] = {}
        for segs in ("1seg", "64seg"):
            if segs == "64seg":
                res["store64"] = many_segments(sp)
            for label, ids in asks.items():
                ws, dev, rows = [], [], 0
                for _ in range(runs):
                    ws.append(wall(lambda: sp.gather(ids)))
                    dev.append(sp.query_ms())
                counts, _ = sp.gather(ids)
                rows = int(counts.sum())
                # the entries of the asked buckets' slices: the store's share of 4096 buckets per asked id
                slice_entries = len(ids) * n / 4096
                d = {"ids": len(ids), "rows": rows, "slice_entries_expected": slice_entries,
                     "stream_ms": summary(dev), "wall_ms": summary(ws)}
                d["bytes"] = SLICE_READS * 8 * slice_entries + 2 * ROW_BYTES * rows
                d["share_of_peak"] = d["bytes"] / (d["stream_ms"]["median"] * 1e-3) / peak
                res["gathers"][f"{segs}_ids{label}"] = d

        cw = []
        for _ in range(runs):
            many_segments(sp)
            cw.append(wall(sp.compact))
        res["compact64"] = {"wall_ms": summary(cw), "bytes_moved": 2 * n * ROW_BYTES}
        res["compact64"]["share_of_peak"] = res["compact64"]["bytes_moved"] / (res["compact64"]["wall_ms"]["median"] * 1e-3) / peak

    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "measure.json").write_text(json.dumps(res, indent=1) + "\n")
    fmt = lambda d: f"{d['median']:9.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    o, t = res["sp_observe"], res["ix_observe"]
    lines = [f"span_store_measure: {n} records, {ntr} traces, S = {S}, seed {a.seed}, {res['device']}; "
             f"ms, median [min, max] of {a.runs} runs, first call apart",
             f" store: {res['store']['entries']} entries, {res['store']['bytes'] / 2**20:.0f} MiB in one segment; "
             f"share of {a.peak_tbs:g} TB/s from each pass's own bytes",
             " zk_sp_observe into an emptied store (alternating with zk_ix_observe, emptied index)",
             f"  count   ( 8 B/record read)                 {fmt(o['count_ms'])}   {100 * o['count_share_of_peak']:.1f} %",
             f"  sizing sync                                {fmt(o['size_ms'])}",
             f"  scatter (56 B/record read, 48 B written)   {fmt(o['scatter_ms'])}   {100 * o['scatter_share_of_peak']:.1f} %",
             f"  device sum                                 {fmt(o['device_ms'])}   {o['records_per_s'] / 1e9:.2f} G records/s, "
             f"{o['bytes_per_s'] / 1e12:.3f} TB/s = {100 * o['share_of_peak']:.1f} %",
             f"  wall, sync                                 {fmt(o['wall_ms'])}",
             f"  zk_ix_observe: count   {fmt(t['count_ms'])}",
             f"  zk_ix_observe: scatter {fmt(t['scatter_ms'])}   {100 * t['scatter_share_of_peak']:.1f} % "
             f"(32 B/record read, 18 B per entry written, {t['entries']} entries)",
             f"  zk_ix_observe: device sum {fmt(t['device_ms'])}   {t['bytes_per_s'] / 1e12:.3f} TB/s = {100 * t['share_of_peak']:.1f} %",
             f" zk_sp_gather (share = {SLICE_READS} reads of the asked buckets' trace_id slices + 96 B per row, in the stream time)"]
    for key, d in res["gathers"].items():
        lines.append(f"  {key:<14} {d['ids']:>5} ids {d['rows']:>7} rows  stream {fmt(d['stream_ms'])}   "
                     f"{100 * d['share_of_peak']:.2f} %   wall {fmt(d['wall_ms'])}")
    c = res["compact64"]
    lines.append(f" zk_sp_compact of 64 segments ({res['store64']['entries']} entries): wall {fmt(c['wall_ms'])}   "
                 f"{100 * c['share_of_peak']:.1f} % (48 B read + 48 B written per entry)")
    (outdir / "measure.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
