#!/usr/bin/env python3
"""Measurement of the annotation store by trace id, recorded, not gated: no number here has an
earlier one to compare with, and bench.py does not run it.

Workload: the C2 batch on the device (bench.py's: --records 1e8, S = 500, seed 2), the batch the span store's
measurement uses (tools/span_store_measure.py), and annotation rows made from it on the device: per record one
OPENING row (cs at first_ts for a client-side record, sr for a server-side one, another value otherwise; the
host's ipv4 is 10.0.0.0 + the record's service id) and one CLOSING row (cr / ss at last_ts). Reported as the
median and range of --runs runs, the first call apart:
  - zk_an_observe of the opening rows (one per record: --records entries) by pass (zk_an_observe_ms: count,
    sizing sync, scatter) into an emptied store, alternating with zk_sp_observe of the span batch in the same
    process (that code is the parent's); each pass's share of --peak-tbs TB/s from its own bytes: the count
    reads 8 B per entry; the scatter reads 44 B per entry and trace_id (8 B) a second time, and writes 44 B
    (the span store's: 8; 56 and 48);
  - zk_an_gather of 100 and of 4096 ids drawn from the batch over that one segment (zk_an_query_ms, and the wall
    time of the call with the host's sort), with the bytes the passes move: 8 B per entry of the asked buckets'
    slices, twice, and 44 B read and written per matching row;
  - with the closing rows observed as a second segment: the wall time of getTraceSummariesByIds(adjust=TIME_SKEW)
    and of getTraceTimelinesByIds at 4096 ids, against the unadjusted host path getTraceSummariesByIds of the
    same run (all three gather, merge and build on the host).
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

ROW_BYTES = 44
COUNT_READ, SCATTER_READ, SCATTER_WRITE = 8, 52, 44  # bytes per entry
SP_COUNT_READ, SP_SCATTER_READ, SP_SCATTER_WRITE = 8, 56, 48  # zk_sp_observe's, per record
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
    ap.add_argument("--query-runs", type=int, default=3, help="runs of the host-path queries at 4096 ids")
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="the HBM bandwidth the shares are of, TB/s")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "annot_store"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from zipkin_amd import DepsContext, DeviceAnnotationRows, DeviceColumns, TraceAnnotationStore, TraceSpanStore, _abi, tracegen_params

    if not torch.cuda.is_available():
        raise SystemExit("annot_store_measure needs a HIP device")
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

    # the rows: an opening and a closing one per record
    fl = cols.flags.to(torch.int64) & 0xFFFFFFFF
    client, server = (fl & _abi.ZK_F_SVC_CLIENT) != 0, (fl & _abi.ZK_F_SVC_SERVER) != 0
    host = (_abi.ZK_AN_HAS_HOST | (80 << _abi.ZK_AN_PORT_SHIFT))
    zero = torch.zeros_like(fl)
    ipv4 = ((10 << 24) + (cols.service_id.to(torch.int64) & 0xFFFFFF)).to(torch.int32)

    def rows(ts, k_client, k_server, value):
        kind = torch.where(server, zero + k_server, torch.where(client, zero + k_client, zero))
        return DeviceAnnotationRows(cols.trace_id, cols.span_id, ts, (zero + value) * (kind + 1), ipv4, cols.service_id,
                                    (kind | host).to(torch.int32))

    opening = rows(cols.first_ts, _abi.ZK_AN_KIND_CS, _abi.ZK_AN_KIND_SR, 0x1234567)
    closing = rows(cols.last_ts, _abi.ZK_AN_KIND_CR, _abi.ZK_AN_KIND_SS, 0x7654321)
    torch.cuda.synchronize()
    peak = a.peak_tbs * 1e12
    res = {"records": n, "traces": ntr, "services": S, "seed": a.seed, "device": torch.cuda.get_device_name(0),
           "peak_tbs": a.peak_tbs, "entries": n}
    runs = a.runs + 1

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # the asked ids: distinct trace ids of the batch, spread over it
    step = max(1, n // 4096)
    pick = cols.trace_id[::step][:8192].contiguous().cpu().numpy().view(np.uint64)
    pick = pick[np.sort(np.unique(pick, return_index=True)[1])][:4096]
    asks = {100: pick[:: max(1, len(pick) // 100)][:100].copy(), len(pick): pick}

    with TraceAnnotationStore(device=0, timing=True) as an, TraceSpanStore(device=0, timing=True) as sp:
        an.observe(opening)
        sp.observe(cols)
        res["store"] = an.info()
        walls, phases, sp_walls, sp_phases = [], [], [], []
        for _ in range(runs):  # the two alternate, so that whatever else the machine does meets both
            an.reset()
            walls.append(wall(lambda: an.observe(opening, sync=False)))
            phases.append(an.observe_ms())
            sp.reset()
            sp_walls.append(wall(lambda: sp.observe(cols, sync=False)))
            sp_phases.append(sp.observe_ms())

        def observed(ws, ph, names, count_read, scatter_read, scatter_write):
            o = {"wall_ms": summary(ws)}
            for k in names:
                o[k + "_ms"] = summary(x[k] for x in ph)
            o["device_ms"] = summary(sum(x.values()) for x in ph)
            o["entries_per_s"] = n / (o["device_ms"]["median"] * 1e-3)
            o["bytes"] = n * (count_read + scatter_read + scatter_write)
            o["bytes_per_s"] = o["bytes"] / (o["device_ms"]["median"] * 1e-3)
            o["share_of_peak"] = o["bytes_per_s"] / peak
            o["count_bytes_per_s"] = n * count_read / (o["count_ms"]["median"] * 1e-3)
            o["scatter_bytes_per_s"] = n * (scatter_read + scatter_write) / (o["scatter_ms"]["median"] * 1e-3)
            o["count_share_of_peak"] = o["count_bytes_per_s"] / peak
            o["scatter_share_of_peak"] = o["scatter_bytes_per_s"] / peak
            return o

        res["an_observe"] = observed(walls, phases, an.OBSERVE_PHASES, COUNT_READ, SCATTER_READ, SCATTER_WRITE)
        res["sp_observe"] = observed(sp_walls, sp_phases, sp.OBSERVE_PHASES, SP_COUNT_READ, SP_SCATTER_READ, SP_SCATTER_WRITE)

        res["gathers"] = {}
        for label, ids in asks.items():
            ws, dev = [], []
            for _ in range(runs):
                ws.append(wall(lambda: an.gather(ids)))
                dev.append(an.query_ms())
            counts, _ = an.gather(ids)
            got = int(counts.sum())
            slice_entries = len(ids) * n / 4096  # the store's share of 4096 buckets per asked id
            d = {"ids": len(ids), "rows": got, "slice_entries_expected": slice_entries, "stream_ms": summary(dev), "wall_ms": summary(ws)}
            d["bytes"] = SLICE_READS * 8 * slice_entries + 2 * ROW_BYTES * got
            d["share_of_peak"] = d["bytes"] / (d["stream_ms"]["median"] * 1e-3) / peak
            res["gathers"][f"1seg_ids{label}"] = d

        # both rows of every record: the adjuster and the timeline on the host, against the unadjusted host path
        an.observe(closing)
        res["store2"] = an.info()
        ids = asks[len(pick)]
        q = {"ids": len(ids)}
        plain, skew, lines = [], [], []
        for _ in range(a.query_runs + 1):
            plain.append(wall(lambda: sp.getTraceSummariesByIds(ids)))
            skew.append(wall(lambda: sp.getTraceSummariesByIds(ids, adjust=("TIME_SKEW",), annotations=an)))
            lines.append(wall(lambda: sp.getTraceTimelinesByIds(ids, annotations=an)))
        q["summaries_unadjusted_host_wall_ms"] = summary(plain)
        q["summaries_time_skew_wall_ms"] = summary(skew)
        q["timelines_wall_ms"] = summary(lines)
        got = sp.getTraceTimelinesByIds(ids, adjust=("TIME_SKEW",), annotations=an)
        q["traces"] = len(got)
        q["annotation_rows"] = int(an.gather(ids)[0].sum())
        q["span_rows"] = int(sp.gather(ids)[0].sum())
        res["queries"] = q

    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "measure.json").write_text(json.dumps(res, indent=1) + "\n")
    fmt = lambda d: f"{d['median']:9.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    o, t = res["an_observe"], res["sp_observe"]
    lines = [f"annot_store_measure: {n} records, {ntr} traces, S = {S}, seed {a.seed}, {res['device']}; "
             f"ms, median [min, max] of {a.runs} runs, first call apart",
             f" store: {res['store']['entries']} entries, {res['store']['bytes'] / 2**20:.0f} MiB in one segment; "
             f"share of {a.peak_tbs:g} TB/s from each pass's own bytes",
             " zk_an_observe into an emptied store (alternating with zk_sp_observe of the span batch, emptied store)",
             f"  count   ( 8 B/entry read)                  {fmt(o['count_ms'])}   {o['count_bytes_per_s'] / 1e12:.3f} TB/s = {100 * o['count_share_of_peak']:.1f} %",
             f"  sizing sync                                {fmt(o['size_ms'])}",
             f"  scatter (52 B/entry read, 44 B written)    {fmt(o['scatter_ms'])}   {o['scatter_bytes_per_s'] / 1e12:.3f} TB/s = {100 * o['scatter_share_of_peak']:.1f} %",
             f"  device sum                                 {fmt(o['device_ms'])}   {o['entries_per_s'] / 1e9:.2f} G entries/s, "
             f"{o['bytes_per_s'] / 1e12:.3f} TB/s = {100 * o['share_of_peak']:.1f} %",
             f"  wall, sync                                 {fmt(o['wall_ms'])}",
             f"  zk_sp_observe: count   {fmt(t['count_ms'])}   {t['count_bytes_per_s'] / 1e12:.3f} TB/s = {100 * t['count_share_of_peak']:.1f} %",
             f"  zk_sp_observe: scatter {fmt(t['scatter_ms'])}   {t['scatter_bytes_per_s'] / 1e12:.3f} TB/s = {100 * t['scatter_share_of_peak']:.1f} % "
             f"(56 B/record read, 48 B written)",
             f"  zk_sp_observe: device sum {fmt(t['device_ms'])}   {t['bytes_per_s'] / 1e12:.3f} TB/s = {100 * t['share_of_peak']:.1f} %",
             f" zk_an_gather (share = {SLICE_READS} reads of the asked buckets' trace_id slices + 88 B per row, in the stream time)"]
    for key, d in res["gathers"].items():
        lines.append(f"  {key:<14} {d['ids']:>5} ids {d['rows']:>7} rows  stream {fmt(d['stream_ms'])}   "
                     f"{100 * d['share_of_peak']:.2f} %   wall {fmt(d['wall_ms'])}")
    q = res["queries"]
    lines += [f" host-path queries of {q['ids']} ids ({q['traces']} traces, {q['span_rows']} span rows, {q['annotation_rows']} annotation rows "
              f"in {res['store2']['segments']} segments), wall ms, median [min, max] of {a.query_runs} runs",
              f"  getTraceSummariesByIds, unadjusted host path   {fmt(q['summaries_unadjusted_host_wall_ms'])}",
              f"  getTraceSummariesByIds(adjust=TIME_SKEW)       {fmt(q['summaries_time_skew_wall_ms'])}",
              f"  getTraceTimelinesByIds                         {fmt(q['timelines_wall_ms'])}"]
    (outdir / "measure.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
