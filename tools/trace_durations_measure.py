#!/usr/bin/env python3
"""Measurement of the trace duration index, recorded, not gated: no number here has an
earlier one to compare with, and bench.py does not run it.

Workload: the C2 batch on the device (bench.py's: --records 1e8, S = 500, seed 2), trace-clustered as
TraceGen makes it. Reported as the median and range of --runs runs, the first call apart:
  - zk_td_observe by pass (zk_td_observe_ms) on an empty table of the size it needs (reset between
    runs, so every run inserts every trace) and on a table that already holds the batch, with bytes/s
    at the 28 B per record it reads; beside it zk_win_observe, the same structure at 20 B per record,
    on the same batch, alternating with it, and the ratio of the two against 28 / 20;
  - zk_td_top (zk_td_top_ms: the handle's stream from the first pass to the last copy) for each order
    at k = 100 and k = 4096 over that table, with the table's bytes and the share of --peak-tbs TB/s
    that three whole-table passes (the bound of DESIGN.md §5d) in that time come to, and the wall time of
    the call.
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

TABLE_PASSES = 3  # zk_td_top reads the table at most three times (include/zkduration.h)


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "trace_durations"))
    a = ap.parse_args()

    import torch

    from zipkin_amd import DepsContext, DeviceColumns, TraceDurationIndex, WindowPartition, tracegen_params
    from zipkin_amd.durations import ORDERS

    if not torch.cuda.is_available():
        raise SystemExit("trace_durations_measure needs a HIP device")
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
    res = {"records": n, "traces": ntr, "services": S, "seed": a.seed, "device": torch.cuda.get_device_name(0),
           "peak_tbs": a.peak_tbs, "table_passes_counted": TABLE_PASSES}
    runs = a.runs + 1

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    with TraceDurationIndex(device=0, timing=True) as td, \
            WindowPartition(window_us=3_600_000_000, origin_us=0, num_windows=1, device=0, timing=True) as win:
        td.observe(cols)   # (sizes the tables; the runs below start from these allocations)
        win.observe(cols)
        res["td_table"] = td.info()
        res["win_table"] = win.table_info()
        for mode in ("insert", "present"):
            rows = {"td": ([], []), "win": ([], [])}
            for _ in range(runs):  # the two alternate, so that whatever else the machine does meets both
                for name, h, reset in (("td", td, td.reset), ("win", win, win.reset_table)):
                    if mode == "insert":
                        reset()
                    rows[name][0].append(wall(lambda: h.observe(cols, sync=False)))
                    rows[name][1].append(h.observe_ms())
            for name, per in (("td", 28), ("win", 20)):
                walls, phases = rows[name]
                o = {"wall_ms": summary(walls), "bytes_per_record": per}
                for k in td.OBSERVE_PHASES:
                    o[k + "_ms"] = summary(x[k] for x in phases)
                o["device_ms"] = summary(sum(x.values()) for x in phases)
                # the run count reads trace_id (8 B), the inserts the rest and trace_id again
                o["insert_gbs"] = n * per / (o["insert_ms"]["median"] * 1e-3) / 1e9
                res[f"{name}_observe_{mode}"] = o
            t, w = res[f"td_observe_{mode}"], res[f"win_observe_{mode}"]
            res[f"ratio_insert_pass_{mode}"] = t["insert_ms"]["median"] / w["insert_ms"]["median"]
            res[f"ratio_device_{mode}"] = t["device_ms"]["median"] / w["device_ms"]["median"]
        res["ratio_of_bytes"] = 28 / 20

        tb = res["td_table"]["bytes"]
        res["top"] = {}
        for order in sorted(ORDERS):
            for k in (100, 4096):
                walls, dev = [], []
                for _ in range(runs):
                    walls.append(wall(lambda: td.top(order, k)))
                    dev.append(td.top_ms())
                d = {"stream_ms": summary(dev), "wall_ms": summary(walls), "matched": td.matched}
                d["share_of_peak"] = TABLE_PASSES * tb / (d["stream_ms"]["median"] * 1e-3) / (a.peak_tbs * 1e12)
                res["top"][f"{order}_k{k}"] = d

    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "measure.json").write_text(json.dumps(res, indent=1) + "\n")
    fmt = lambda d: f"{d['median']:9.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    lines = [f"trace_durations_measure: {n} records, {ntr} traces, S = {S}, seed {a.seed}, {res['device']}; "
             f"ms, median [min, max] of {a.runs} runs, first call apart",
             f" duration table: {res['td_table']['slots']} slots, {res['td_table']['traces']} traces, "
             f"{res['td_table']['bytes'] / 2**20:.0f} MiB; trace-time table: {res['win_table']['bytes'] / 2**20:.0f} MiB"]
    for mode, what in (("insert", "empty table, every trace inserted"), ("present", "every trace already present")):
        lines.append(f" observe, {what}")
        for name, label in (("td", "zk_td_observe  (28 B/record)"), ("win", "zk_win_observe (20 B/record)")):
            o = res[f"{name}_observe_{mode}"]
            lines.append(f"  {label}: run count   {fmt(o['runs_ms'])}")
            lines.append(f"  {label}: sizing      {fmt(o['grow_ms'])}")
            lines.append(f"  {label}: inserts     {fmt(o['insert_ms'])}   {o['insert_gbs']:.0f} GB/s")
            lines.append(f"  {label}: device sum  {fmt(o['device_ms'])}")
            lines.append(f"  {label}: wall, sync  {fmt(o['wall_ms'])}")
        lines.append(f"  td / win: insert pass {res[f'ratio_insert_pass_{mode}']:.3f}, device sum {res[f'ratio_device_{mode}']:.3f} "
                     f"(bytes read: 28 / 20 = 1.400)")
    lines.append(f" zk_td_top over the table ({tb / 2**20:.0f} MiB; share of {a.peak_tbs:g} TB/s = {TABLE_PASSES} table passes in the stream time)")
    for key, d in res["top"].items():
        lines.append(f"  {key:<22} stream {fmt(d['stream_ms'])}   {100 * d['share_of_peak']:.1f} %   wall {fmt(d['wall_ms'])}")
    (outdir / "measure.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
