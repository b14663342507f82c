#!/usr/bin/env python3
"""Measurement of the trace-time table and the table-mode partition, recorded, not gated.

Workload: the C2 batch on the device (bench.py's: --records 1e8, S = 500, seed 2), once trace-clustered
as TraceGen makes it and once globally shuffled; windows of one hour. Reported, by HIP events or a
host clock around synchronous calls, as the median and range of --runs runs with the first call apart:
  - yardsticks of the same session and batch, none of them the code under test: the existing clustered
    zk_win_partition (k_win_time and the other passes), a device-to-device copy of the seven columns,
    zk_timing.cluster_ms of the batch accumulated without ZK_BATCH_TRACE_CLUSTERED;
  - zk_win_observe on an empty table of the size it needs (reset between runs, so every run inserts
    every trace) and on a table that already holds the batch (every update finds its key and skips):
    the run count, the sizing step, the inserts (zk_win_observe_ms) and the wall time with a sync;
  - zk_win_partition with ZK_WIN_TRACE_TABLE by phase (zk_win_phase_ms) and as a whole call;
  - WindowedAggregateJob(order="rows") on the clustered batch cut into four at record positions that
    fall inside traces, WindowedAggregateJob(order="any") on the shuffled batch, and order="whole" on
    the uncut clustered batch beside them.
Writes <out>/table_bench.json and <out>/table_bench.txt. Needs a gfx950 device."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "windows"))
    a = ap.parse_args()

    import torch

    from zipkin_amd import DepsContext, DeviceColumns, WindowedAggregateJob, WindowPartition, tracegen_params
    from zipkin_amd.aggregates import Dictionary
    from zipkin_amd.columns import COLUMNS
    from zipkin_amd.windows import _timed_min_max

    if not torch.cuda.is_available():
        raise SystemExit("window_table_bench needs a HIP device")
    S = a.services
    ctx = DepsContext(S, device=0, timing=True)
    p = tracegen_params(a.seed, int(a.records / 15) + 1000, target_records=a.records, max_depth=a.max_depth,
                        num_services=S)
    cols = DeviceColumns(a.records, device="cuda:0")
    n, ntr = ctx.tracegen_device(p, cols)
    ctx.sync()
    cols = cols.slice(0, n)
    out = DeviceColumns(n, device="cuda:0")
    perm = torch.randperm(n, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(a.seed))
    shuf = DeviceColumns(n, device="cuda:0")
    for k, _ in COLUMNS:
        getattr(shuf, k).copy_(getattr(cols, k)[perm])
    del perm
    torch.cuda.synchronize()
    res = {"records": n, "traces": ntr, "services": S, "seed": a.seed, "device": torch.cuda.get_device_name(0)}
    runs = a.runs + 1

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def copy():
        for k, _ in COLUMNS:
            getattr(out, k).copy_(getattr(cols, k))

    res["d2d_copy_ms"] = summary(wall(copy) for _ in range(runs))
    times = []
    for _ in range(runs):
        ctx.reset()
        ctx.accumulate(shuf, clustered=False, verify=False)
        times.append(ctx.timing()["cluster_ms"])
    res["cluster_ms_shuffled"] = summary(times)
    ctx.reset()
    ctx.close()

    lo, hi = _timed_min_max(cols)
    win_us = 3_600_000_000
    origin = lo // win_us * win_us
    W = (hi - origin) // win_us + 1
    res["W"] = W
    with WindowPartition(window_us=win_us, origin_us=origin, num_windows=W, device=0, timing=True) as h:
        # the yardstick: the existing clustered partition (no table)
        walls, phases = [], []
        for _ in range(runs):
            walls.append(wall(lambda: h.partition(cols, out=out)))
            phases.append(h.phase_ms())
        y = {"wall_ms": summary(walls), "device_ms": summary(sum(x.values()) for x in phases)}
        for k in h.PHASES:
            y[k + "_ms"] = summary(x[k] for x in phases)
        res["clustered_partition"] = y

        for label, batch in (("clustered", cols), ("shuffled", shuf)):
            r = {}
            h.reset_table()
            h.observe(batch)  # (sizes the table; the runs below start from this allocation)
            r["table"] = h.table_info()
            for mode in ("insert", "present"):
                walls, phases = [], []
                for _ in range(runs):
                    if mode == "insert":
                        h.reset_table()
                    walls.append(wall(lambda: h.observe(batch, sync=False)))
                    phases.append(h.observe_ms())
                o = {"wall_ms": summary(walls)}
                for k in h.OBSERVE_PHASES:
                    o[k + "_ms"] = summary(x[k] for x in phases)
                r["observe_" + mode] = o
            walls, phases, cnt = [], [], None
            for _ in range(runs):
                walls.append(wall(lambda: h.partition(batch, out=out, table=True, clustered=label == "clustered")))
                phases.append(h.phase_ms())
            _, _, cnt = h.partition(batch, out=out, table=True, clustered=label == "clustered")
            t = {"wall_ms": summary(walls), "device_ms": summary(sum(x.values()) for x in phases), "counts": cnt}
            for k in h.PHASES:
                t[k + "_ms"] = summary(x[k] for x in phases)
            r["table_partition"] = t
            res[label] = r

    del out
    names = Dictionary([f"svc{i}" for i in range(S)])
    rows4 = [cols.slice(n * k // 4 + (3 if k else 0), n * (k + 1) // 4 + (3 if k < 3 else 0)) for k in range(4)]
    for label, batches, order in (("job_whole_uncut", [cols], "whole"), ("job_rows_cut_in_four", rows4, "rows"),
                                  ("job_any_shuffled", [shuf], "any")):
        job = WindowedAggregateJob(names, window_us=win_us, device=0, verify=False, order=order)
        times = [wall(lambda: job.run(batches, num_services=S)) for _ in range(runs)]
        res[label + "_ms"] = summary(times)
        res[label + "_windows"] = len(job.stats)
        job.close()

    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "table_bench.json").write_text(json.dumps(res, indent=1) + "\n")
    fmt = lambda d: f"{d['median']:9.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    lines = [f"window_table_bench: {n} records, {ntr} traces, S = {S}, seed {a.seed}, {res['device']}; 1-hour windows, W = {W}; "
             f"ms, median [min, max] of {a.runs} runs, first call apart",
             " yardsticks (same session and batch)",
             f"  d2d copy of the seven columns (96 B/record)    {fmt(res['d2d_copy_ms'])}",
             f"  cluster_ms (P0-P2) of the shuffled batch       {fmt(res['cluster_ms_shuffled'])}"]
    y = res["clustered_partition"]
    for k in ("time", "resolve", "hist", "scan", "scatter", "final"):
        lines.append(f"  clustered partition (no table): k_win_{k:<8} {fmt(y[k + '_ms'])}")
    lines.append(f"  clustered partition (no table): device sum     {fmt(y['device_ms'])}")
    lines.append(f"  clustered partition (no table): wall with sync {fmt(y['wall_ms'])}")
    for label in ("clustered", "shuffled"):
        r = res[label]
        lines.append(f" the {label} batch: table {r['table']['slots']} slots, {r['table']['traces']} traces, "
                     f"{r['table']['bytes'] / 2**20:.0f} MiB")
        for mode, what in (("insert", "empty table, every trace inserted"), ("present", "every trace already present")):
            o = r["observe_" + mode]
            lines.append(f"  zk_win_observe, {what}")
            lines.append(f"    k_wt_runs                                    {fmt(o['runs_ms'])}")
            lines.append(f"    sizing (count to the host; no growth)        {fmt(o['grow_ms'])}")
            lines.append(f"    k_wt_observe                                 {fmt(o['insert_ms'])}")
            lines.append(f"    wall with a sync                             {fmt(o['wall_ms'])}")
        t = r["table_partition"]
        lines.append("  zk_win_partition with ZK_WIN_TRACE_TABLE")
        lines.append(f"    k_wt_lookup                                  {fmt(t['time_ms'])}")
        for k in ("hist", "scan", "scatter", "final"):
            lines.append(f"    k_win_{k:<8}                               {fmt(t[k + '_ms'])}")
        lines.append(f"    device sum                                   {fmt(t['device_ms'])}")
        lines.append(f"    wall with its sync                           {fmt(t['wall_ms'])}")
        lines.append(f"    unobserved_records {t['counts']['unobserved_records']}, partitioned runs {t['counts']['partitioned_runs']}")
    lines.append(" jobs (run() as a whole: window choice, observe, partition, a step per window, finalize to the host)")
    for label in ("job_whole_uncut", "job_rows_cut_in_four", "job_any_shuffled"):
        lines.append(f"  {label:<22} ({res[label + '_windows']} windows)        {fmt(res[label + '_ms'])}")
    (outdir / "table_bench.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
