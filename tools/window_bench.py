#!/usr/bin/env python3
"""Measurement of the trace-time partition and the windowed job, recorded, not gated.

Workload: the C2 batch on the device (bench.py's: --records 1e8, S = 500, seed 2), windows of one
hour and of ten minutes. Reported, by HIP events or a host clock around synchronous calls, as the
median and range of --runs runs with the first call apart:
  - every pass of zk_win_partition (zk_win_phase_ms) and the whole call (wall, with its sync);
  - two yardsticks of the same session and batch: a device-to-device copy of the seven columns
    (96 B per record, the floor of the scatter) and zk_timing.cluster_ms of the same batch
    accumulated without ZK_BATCH_TRACE_CLUSTERED (P0-P2, which move every record twice);
  - the plain C2 step (reset + accumulate + finalize into device buffers), serial and pipelined
    over four table/stream sets as bench.py's default;
  - the windowed job: partition + one such step per window (its slices copied where they start on
    an odd record), and the per-window fixed cost (the same step on a 1024-record slice).
Writes <out>/window_bench.json and <out>/window_bench.txt. Needs a gfx950 device."""
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
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": len(xs)}


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

    from zipkin_amd import DepsContext, DeviceColumns, WindowPartition, tracegen_params
    from zipkin_amd.columns import COLUMNS
    from zipkin_amd.windows import _timed_min_max, window_slice

    if not torch.cuda.is_available():
        raise SystemExit("window_bench needs a HIP device")
    dev = torch.device("cuda", 0)
    S, cells = a.services, a.services * a.services
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx = DepsContext(S, device=0, stream=stream.cuda_stream, timing=True)
    p = tracegen_params(a.seed, int(a.records / 15) + 1000, target_records=a.records, max_depth=a.max_depth,
                        num_services=S)
    cols = DeviceColumns(a.records, device="cuda:0")
    n, ntr = ctx.tracegen_device(p, cols)
    ctx.sync()
    cols = cols.slice(0, n)
    out = DeviceColumns(n, device="cuda:0")
    tab = {"m0": torch.empty(cells, dtype=torch.int64, device=dev), "present": torch.empty(cells, dtype=torch.uint8, device=dev)}
    for k in ("m1", "m2", "m3", "m4"):
        tab[k] = torch.empty(cells, dtype=torch.float64, device=dev)
    res = {"records": n, "traces": ntr, "services": S, "seed": a.seed, "device": torch.cuda.get_device_name(0)}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def step(c):
        ctx.reset()
        ctx.accumulate(c, clustered=True, verify=False)
        ctx.finalize(out_device=tab)

    # yardstick: device-to-device copy of the seven columns
    def copy():
        for k, _ in COLUMNS:
            getattr(out, k).copy_(getattr(cols, k))

    times = [wall(copy) for _ in range(a.runs + 1)]
    res["d2d_copy_ms"] = {"first": times[0], **summary(times[1:])}
    # yardstick: the clustering pass of the same batch (accumulate without ZK_BATCH_TRACE_CLUSTERED)
    times = []
    for _ in range(a.runs + 1):
        ctx.reset()
        ctx.accumulate(cols, clustered=False, verify=False)
        times.append(ctx.timing()["cluster_ms"])
    res["cluster_ms"] = {"first": times[0], **summary(times[1:])}
    # the plain serial C2 step
    times = [wall(lambda: step(cols)) for _ in range(a.runs + 1)]
    res["plain_step_ms"] = {"first": times[0], **summary(times[1:])}
    # the plain pipelined C2 step, as bench.py runs it by default: four table/stream sets, batch k's
    # join overlapping the tails of the batches before it, every batch finalized inside the window
    sets = [(ctx, stream, tab)]
    for _ in range(3):
        s2 = torch.cuda.Stream(device=dev)
        sets.append((DepsContext(S, device=0, stream=s2.cuda_stream), s2, {k: torch.empty_like(v) for k, v in tab.items()}))
    pending = []

    def pipelined(steps):
        for k in range(steps):
            c, s, o = sets[k % len(sets)]
            torch.cuda.set_stream(s)
            c.reset()
            c.accumulate(cols, clustered=True, verify=False)
            pending.append((c, s, o))
            if len(pending) > len(sets) - 1:
                pc, ps, po = pending.pop(0)
                torch.cuda.set_stream(ps)
                pc.finalize(out_device=po)
        while pending:
            pc, ps, po = pending.pop(0)
            torch.cuda.set_stream(ps)
            pc.finalize(out_device=po)
        torch.cuda.set_stream(stream)

    times = [wall(lambda: pipelined(20)) / 20 for _ in range(a.runs + 1)]
    res["pipelined_step_ms"] = {"first": times[0], **summary(times[1:])}
    for c, _, _ in sets[1:]:
        c.close()
    small = cols.slice(0, 1024)
    times = [wall(lambda: step(small)) for _ in range(a.runs + 1)]
    res["per_window_fixed_ms"] = {"first": times[0], **summary(times[1:])}

    lo, hi = _timed_min_max(cols)
    res["windows"] = {}
    for label, win_us in (("1h", 3_600_000_000), ("10min", 600_000_000)):
        origin = lo // win_us * win_us
        W = (hi - origin) // win_us + 1
        with WindowPartition(window_us=win_us, origin_us=origin, num_windows=W, device=0, timing=True) as h:
            walls, phases, parts = [], [], None
            for _ in range(a.runs + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                parts = h.partition(cols, out=out)
                walls.append((time.perf_counter() - t0) * 1e3)
                phases.append(h.phase_ms())
            _, off, cnt = parts
            r = {"W": W, "origin_us": origin, "plan": h.plan(n), "counts": cnt,
                 "windows_with_records": int(sum(1 for w in range(W) if off[w + 1] > off[w])),
                 "odd_starts": int(sum(1 for w in range(W) if off[w + 1] > off[w] and int(off[w]) % 2)),
                 "partition_wall_ms": {"first": walls[0], **summary(walls[1:])},
                 "partition_device_ms": {"first": sum(phases[0].values()), **summary(sum(x.values()) for x in phases[1:])}}
            for k in h.PHASES:
                r[k + "_ms"] = {"first": phases[0][k], **summary(x[k] for x in phases[1:])}

            def job():
                _, o, _ = h.partition(cols, out=out)
                for w in range(W):
                    if o[w + 1] > o[w]:
                        step(window_slice(out, int(o[w]), int(o[w + 1])))

            times = [wall(job) for _ in range(a.runs + 1)]
            r["windowed_job_ms"] = {"first": times[0], **summary(times[1:])}
        res["windows"][label] = r

    ctx.close()
    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "window_bench.json").write_text(json.dumps(res, indent=1) + "\n")
    fmt = lambda d: f"{d['median']:9.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    lines = [f"window_bench: {n} records, {ntr} traces, S = {S}, seed {a.seed}, {res['device']}; ms, median [min, max] of "
             f"{a.runs} runs, first call apart",
             f"  d2d copy of the seven columns (96 B/record)  {fmt(res['d2d_copy_ms'])}",
             f"  cluster_ms (P0-P2 of the unclustered batch)  {fmt(res['cluster_ms'])}",
             f"  plain serial step (reset+accumulate+finalize) {fmt(res['plain_step_ms'])}",
             f"  plain pipelined step (4 table sets, 20 steps) {fmt(res['pipelined_step_ms'])}",
             f"  per-window fixed cost (1024-record step)     {fmt(res['per_window_fixed_ms'])}"]
    for label, r in res["windows"].items():
        lines.append(f"  windows of {label}: W = {r['W']}, {r['windows_with_records']} with records, {r['odd_starts']} start on an "
                     f"odd record; plan (chunk, range, ranges) = {tuple(r['plan'])}")
        for k in ("time", "resolve", "hist", "scan", "scatter", "final"):
            lines.append(f"    k_win_{k:<8}                               {fmt(r[k + '_ms'])}")
        lines.append(f"    partition, device (sum of the passes)       {fmt(r['partition_device_ms'])}")
        lines.append(f"    zk_win_partition, wall with its sync        {fmt(r['partition_wall_ms'])}")
        lines.append(f"    windowed job (partition + a step per window) {fmt(r['windowed_job_ms'])}")
    (outdir / "window_bench.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
