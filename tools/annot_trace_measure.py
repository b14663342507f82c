#!/usr/bin/env python3
"""Measurement of the time-skew-adjusted traces on the device, recorded, not gated by bench.py.

Workload: tools/annot_adjust_measure.py's, the same batch and the same 4096 ids. The C2 batch on the device
(bench.py's: --records 1e8, S = 500, seed 2) in a span store, and an OPENING and a CLOSING annotation row per
record in an annotation store, as two segments. In one process and one session, alternating, the median and
range of --runs runs with the first call apart:
  - getTraceCombosByIds(adjust=TIME_SKEW, annotations=): the host path, the parent commit's only way to
    answer, against adjust_on_device=True; wall time;
  - getTraceTimelinesByIds(adjust=TIME_SKEW, annotations=): the same two paths; wall time;
  - the raw call zk_an_adjusted_traces (sizing and filling), wall time, and its filling call's stream time:
    zk_an_query_ms (this handle's passes, the emitting k_an_adjust among them) and zk_sp_query_ms (zk_sp_traces'
    passes on the span store's stream);
  - zk_an_adjusted_summaries of the same ids in the same session, stream time: the difference is the emission.
Both paths' lists are compared equal before anything is timed. Writes <out>/measure.json and <out>/measure.txt.
Needs a gfx950 device."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SKEW = ("TIME_SKEW",)


def summary(xs):
    xs = list(xs)
    return {"first": xs[0], "median": statistics.median(xs[1:]), "min": min(xs[1:]), "max": max(xs[1:]), "runs": len(xs) - 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--services", type=int, default=500)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--label", default="", help="a word for the report's first line, e.g. 'rehearsal'")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "annot_trace"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from zipkin_amd import DepsContext, DeviceAnnotationRows, DeviceColumns, TraceAnnotationStore, TraceSpanStore, _abi, tracegen_params

    if not torch.cuda.is_available():
        raise SystemExit("annot_trace_measure needs a HIP device")
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

    # the rows: an opening and a closing one per record (tools/annot_store_measure.py's)
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
    res = {"records": n, "traces": ntr, "services": S, "seed": a.seed, "device": torch.cuda.get_device_name(0), "label": a.label}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    step = max(1, n // 4096)
    pick = cols.trace_id[::step][:8192].contiguous().cpu().numpy().view(np.uint64)
    ids = pick[np.sort(np.unique(pick, return_index=True)[1])][:4096]

    with TraceAnnotationStore(device=0, timing=True) as an, TraceSpanStore(device=0, timing=True) as sp:
        sp.observe(cols)
        an.observe(opening)
        an.observe(closing)
        res["span_store"], res["annotation_store"] = sp.info(), an.info()
        # the answers first: the new path gives the host path's lists
        def combo_view(c):
            t = c.trace
            return ([tuple(x) for x in t.spans], [x.annotations for x in t.spans], t.annotations, t.getRootMostSpan(), t.toSpanDepths(),
                    c.summary, c.timeline, c.span_depths)

        want = sp.getTraceCombosByIds(ids, adjust=SKEW, annotations=an)
        got = sp.getTraceCombosByIds(ids, adjust=SKEW, annotations=an, adjust_on_device=True)
        if [combo_view(c) for c in got] != [combo_view(c) for c in want]:
            raise SystemExit("the device path's combos differ from the host path's")
        if sp.getTraceTimelinesByIds(ids, adjust=SKEW, annotations=an, adjust_on_device=True) != \
                sp.getTraceTimelinesByIds(ids, adjust=SKEW, annotations=an):
            raise SystemExit("the device path's timelines differ from the host path's")
        del want, got
        heads, spans, services, rows = an.adjusted_traces(sp, ids)
        q = {"ids": len(ids), "found": int(((heads["state"] & _abi.ZK_SP_TR_FOUND) != 0).sum()),
             "span_rows": int(heads["fragments"].sum()), "annotation_rows": int(an.gather(ids)[0].sum()),
             "spans": int(len(spans)), "services": int(len(services)), "rows": int(len(rows)),
             "injected_rows": int(spans["injected"].sum()),
             "overflowed": int(((heads["state"] & _abi.ZK_AN_ADJ_OVERFLOW) != 0).sum()),
             "annotated": int(((heads["state"] & _abi.ZK_AN_ADJ_ANNOTATED) != 0).sum())}
        del heads, spans, services, rows
        names = ("combos_host", "combos_device", "timelines_host", "timelines_device", "raw", "an_ms", "sp_ms", "sum_an_ms", "sum_sp_ms")
        t = {k: [] for k in names}
        for _ in range(a.runs + 1):  # the paths alternate, so that whatever else the machine does meets all
            t["combos_host"].append(wall(lambda: sp.getTraceCombosByIds(ids, adjust=SKEW, annotations=an)))
            t["combos_device"].append(wall(lambda: sp.getTraceCombosByIds(ids, adjust=SKEW, annotations=an, adjust_on_device=True)))
            t["timelines_host"].append(wall(lambda: sp.getTraceTimelinesByIds(ids, adjust=SKEW, annotations=an)))
            t["timelines_device"].append(wall(lambda: sp.getTraceTimelinesByIds(ids, adjust=SKEW, annotations=an, adjust_on_device=True)))
            t["raw"].append(wall(lambda: an.adjusted_traces(sp, ids)))
            t["an_ms"].append(an.query_ms())
            t["sp_ms"].append(sp.query_ms())
            an.adjusted_summaries(sp, ids)
            t["sum_an_ms"].append(an.query_ms())
            t["sum_sp_ms"].append(sp.query_ms())
        q["combos_host_wall_ms"] = summary(t["combos_host"])
        q["combos_device_wall_ms"] = summary(t["combos_device"])
        q["timelines_host_wall_ms"] = summary(t["timelines_host"])
        q["timelines_device_wall_ms"] = summary(t["timelines_device"])
        q["raw_call_wall_ms"] = summary(t["raw"])
        q["an_stream_ms"] = summary(t["an_ms"])
        q["sp_stream_ms"] = summary(t["sp_ms"])
        q["stream_ms"] = summary(x + y for x, y in zip(t["an_ms"], t["sp_ms"]))
        q["summaries_an_stream_ms"] = summary(t["sum_an_ms"])
        q["summaries_stream_ms"] = summary(x + y for x, y in zip(t["sum_an_ms"], t["sum_sp_ms"]))
        q["combos_ratio_host_over_device"] = q["combos_host_wall_ms"]["median"] / q["combos_device_wall_ms"]["median"]
        q["timelines_ratio_host_over_device"] = q["timelines_host_wall_ms"]["median"] / q["timelines_device_wall_ms"]["median"]
        res["queries"] = q

    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "measure.json").write_text(json.dumps(res, indent=1) + "\n")
    fmt = lambda d: f"{d['median']:10.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    lines = [f"annot_trace_measure{' (' + a.label + ')' if a.label else ''}: {n} records, {ntr} traces, S = {S}, seed {a.seed}, "
             f"{res['device']}; ms, median [min, max] of {a.runs} runs, first call apart",
             f" span store: {res['span_store']['entries']} entries in {res['span_store']['segments']} segment(s); annotation store: "
             f"{res['annotation_store']['entries']} rows in {res['annotation_store']['segments']} segments",
             f" {q['ids']} ids: {q['found']} found, {q['span_rows']} span rows, {q['annotation_rows']} annotation rows; emitted "
             f"{q['spans']} spans, {q['services']} services, {q['rows']} rows, {q['injected_rows']} of them injected; "
             f"{q['annotated']} annotated, {q['overflowed']} overflowed",
             " the two paths alternating, the answers equal",
             f"  getTraceCombosByIds, host path (the baseline), wall     {fmt(q['combos_host_wall_ms'])}",
             f"  getTraceCombosByIds, adjust_on_device=True, wall        {fmt(q['combos_device_wall_ms'])}   "
             f"{q['combos_ratio_host_over_device']:.1f} x faster",
             f"  getTraceTimelinesByIds, host path (the baseline), wall  {fmt(q['timelines_host_wall_ms'])}",
             f"  getTraceTimelinesByIds, adjust_on_device=True, wall     {fmt(q['timelines_device_wall_ms'])}   "
             f"{q['timelines_ratio_host_over_device']:.1f} x faster",
             f"  zk_an_adjusted_traces (both calls), wall                {fmt(q['raw_call_wall_ms'])}",
             f"  its filling call: zk_an_query_ms                        {fmt(q['an_stream_ms'])}",
             f"                    zk_sp_query_ms (zk_sp_traces' passes) {fmt(q['sp_stream_ms'])}",
             f"                    both streams                          {fmt(q['stream_ms'])}",
             " zk_an_adjusted_summaries, the same ids, the same session",
             f"  its filling call: zk_an_query_ms                        {fmt(q['summaries_an_stream_ms'])}",
             f"                    both streams                          {fmt(q['summaries_stream_ms'])}",
             " not measured: traces near the bounds (2048 spans or rows): this batch's traces are short"]
    (outdir / "measure.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
