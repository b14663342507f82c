#!/usr/bin/env python3
"""Measurement of merged traces on the device, recorded, not gated: bench.py does not run it.

Workload: tools/span_summary_measure.py's: the C2 batch on the device (bench.py's: --records 1e8, S = 500,
seed 2) and asks of 100 and 4096 ids drawn from the batch, over one segment and over 64 segments of the same
records. Per ask, alternating in one process so that both paths meet the same machine state, the median and
range of --runs runs, the first call apart:
  - host (the BASELINE): getTraceCombosByIds(ids), the default path: zk_sp_gather, then Trace, TraceSummary.of
    and toSpanDepths in Python, which is getTracesByIds + toSpanDepths as they were before zk_sp_traces: the
    wall time of the call, and zk_sp_query_ms of its zk_sp_gather;
  - device: getTraceCombosByIds(ids, on_device=True): the wall time of the call, and zk_sp_query_ms of its
    last zk_sp_traces (the filling call: count pass, prefix sum, write pass, k_sp_trace, the heads' copy, the
    spans' and services' copy; the sizing call before it runs the same passes without the last copy and is in
    the wall time only);
  - traces(ids) alone (the two C calls and the numpy arrays, no Python objects): wall time;
  - summaries(ids) alone, for k_sp_summarize's stream time on the same ask beside k_sp_trace's: wall time and
    zk_sp_query_ms of its filling call.
The two paths' answers are compared on every ask (spans, summary, depths, root-most span, serviceCounts).
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


def summary(xs):
    xs = list(xs)
    return {"first": xs[0], "median": statistics.median(xs[1:]), "min": min(xs[1:]), "max": max(xs[1:]), "runs": len(xs) - 1}


def view(c):
    root = c.trace.getRootMostSpan()
    return (c.trace.spans, c.summary, c.span_depths, None if root is None else root.id, c.trace.serviceCounts())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--services", type=int, default=500)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "span_trace"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from zipkin_amd import DepsContext, DeviceColumns, TraceSpanStore, _abi, tracegen_params

    if not torch.cuda.is_available():
        raise SystemExit("span_trace_measure needs a HIP device")
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
    res = {"records": n, "traces": ntr, "services": S, "seed": a.seed, "device": torch.cuda.get_device_name(0)}
    runs = a.runs + 1

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # the asked ids: distinct trace ids of the batch, spread over it (tools/span_store_measure.py's)
    step = max(1, n // 4096)
    pick = cols.trace_id[::step][:8192].contiguous().cpu().numpy().view(np.uint64)
    pick = pick[np.sort(np.unique(pick, return_index=True)[1])][:4096]
    asks = {100: pick[:: max(1, len(pick) // 100)][:100].copy(), len(pick): pick}

    res["asks"] = {}
    with TraceSpanStore(device=0, timing=True) as sp:
        for segs in ("1seg", "64seg"):
            sp.reset()
            k = 1 if segs == "1seg" else 64
            for j in range(k):
                sp.observe(cols.slice(j * n // k, (j + 1) * n // k), sync=False)
            res["store_" + segs] = sp.info()
            for label, ids in asks.items():
                dev_w, dev_s, raw_w, sum_w, sum_s, host_w, host_s = [], [], [], [], [], [], []
                for _ in range(runs):  # the paths alternate
                    dev_w.append(wall(lambda: sp.getTraceCombosByIds(ids, on_device=True)))
                    dev_s.append(sp.query_ms())
                    raw_w.append(wall(lambda: sp.traces(ids)))
                    sum_w.append(wall(lambda: sp.summaries(ids)))
                    sum_s.append(sp.query_ms())
                    host_w.append(wall(lambda: sp.getTraceCombosByIds(ids)))
                    host_s.append(sp.query_ms())
                heads, spans, services = sp.traces(ids)
                same = [view(c) for c in sp.getTraceCombosByIds(ids, on_device=True)] == [view(c) for c in sp.getTraceCombosByIds(ids)]
                res["asks"][f"{segs}_ids{label}"] = {
                    "ids": len(ids), "rows": int(heads["fragments"].sum()), "spans": int(len(spans)), "services": int(len(services)),
                    "overflow": int(((heads["state"] & _abi.ZK_SP_TR_OVERFLOW) != 0).sum()),
                    "longest_trace": int(heads["fragments"].max()), "deepest": int(spans["depth"].max()), "answers_equal": bool(same),
                    "device_wall_ms": summary(dev_w), "device_stream_ms": summary(dev_s), "traces_wall_ms": summary(raw_w),
                    "summaries_wall_ms": summary(sum_w), "summaries_stream_ms": summary(sum_s),
                    "host_wall_ms": summary(host_w), "host_stream_ms": summary(host_s)}

    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "measure.json").write_text(json.dumps(res, indent=1) + "\n")
    fmt = lambda d: f"{d['median']:9.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    lines = [f"span_trace_measure: {n} records, {ntr} traces, S = {S}, seed {a.seed}, {res['device']}; "
             f"ms, median [min, max] of {a.runs} runs, first call apart; the paths alternate in one process",
             " host = getTraceCombosByIds(ids), the default path (the baseline); device = getTraceCombosByIds(ids, on_device=True); "
             "traces = traces(ids) alone; summaries = summaries(ids) alone"]
    for key, d in res["asks"].items():
        lines += [f" {key}: {d['ids']} ids, {d['rows']} rows, {d['spans']} spans, {d['services']} (span, service) pairs, longest trace "
                  f"{d['longest_trace']} rows, deepest span {d['deepest']}, {d['overflow']} above the bound, answers equal: {d['answers_equal']}",
                  f"  host      stream (zk_sp_gather)     {fmt(d['host_stream_ms'])}   wall {fmt(d['host_wall_ms'])}",
                  f"  device    stream (zk_sp_traces)     {fmt(d['device_stream_ms'])}   wall {fmt(d['device_wall_ms'])}",
                  f"  traces                                                                 wall {fmt(d['traces_wall_ms'])}",
                  f"  summaries stream (zk_sp_summaries)  {fmt(d['summaries_stream_ms'])}   wall {fmt(d['summaries_wall_ms'])}"]
    (outdir / "measure.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
