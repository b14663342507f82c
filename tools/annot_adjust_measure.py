#!/usr/bin/env python3
"""Measurement of the time-skew-adjusted summaries on the device, recorded, not gated by bench.py.

Workload: tools/annot_store_measure.py's. The C2 batch on the device (bench.py's: --records 1e8, S = 500, seed 2)
in a span store, and an OPENING and a CLOSING annotation row per record in an annotation store (cs / sr at
first_ts, cr / ss at last_ts; the host's ipv4 is 10.0.0.0 + the record's service id), as two segments. 4096 ids
drawn from the batch are asked. In one process and one session, alternating, the median and range of --runs
runs with the first call apart:
  - the host path getTraceSummariesByIds(adjust=TIME_SKEW, annotations=): the parent commit's code, the baseline;
  - the new path getTraceSummariesByIds(adjust=TIME_SKEW, annotations=, adjust_on_device=True), wall time;
  - the new path's stream time: zk_an_query_ms (this handle's passes, k_an_adjust among them) and zk_sp_query_ms
    (zk_sp_traces' passes on the span store's stream) of the raw call's filling call;
  - zk_sp_summaries of the same ids (stream time and the wall time of on_device=True), the unadjusted yardstick.
Both paths' answers are compared before anything is timed. Writes <out>/measure.json and <out>/measure.txt. Needs
a gfx950 device."""
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "annot_adjust"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from zipkin_amd import DepsContext, DeviceAnnotationRows, DeviceColumns, TraceAnnotationStore, TraceSpanStore, _abi, tracegen_params

    if not torch.cuda.is_available():
        raise SystemExit("annot_adjust_measure needs a HIP device")
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
        # the answers first: the new path gives the host path's list
        want = sp.getTraceSummariesByIds(ids, adjust=SKEW, annotations=an)
        got = sp.getTraceSummariesByIds(ids, adjust=SKEW, annotations=an, adjust_on_device=True)
        if got != want:
            raise SystemExit("the device path's summaries differ from the host path's")
        heads, ents = an.adjusted_summaries(sp, ids)
        q = {"ids": len(ids), "summaries": len(want), "entries": int(len(ents["first"])),
             "span_rows": int(heads["fragments"].sum()), "annotation_rows": int(an.gather(ids)[0].sum()),
             "adjusted_spans": int(heads["spans"].sum()),
             "overflowed": int(((heads["state"] & _abi.ZK_AN_ADJ_OVERFLOW) != 0).sum()),
             "annotated": int(((heads["state"] & _abi.ZK_AN_ADJ_ANNOTATED) != 0).sum())}
        host, dev, an_ms, sp_ms, raw, plain_wall, plain_ms = [], [], [], [], [], [], []
        for _ in range(a.runs + 1):  # the paths alternate, so that whatever else the machine does meets all
            host.append(wall(lambda: sp.getTraceSummariesByIds(ids, adjust=SKEW, annotations=an)))
            dev.append(wall(lambda: sp.getTraceSummariesByIds(ids, adjust=SKEW, annotations=an, adjust_on_device=True)))
            raw.append(wall(lambda: an.adjusted_summaries(sp, ids)))
            an_ms.append(an.query_ms())
            sp_ms.append(sp.query_ms())
            plain_wall.append(wall(lambda: sp.getTraceSummariesByIds(ids, on_device=True)))
            sp.summaries(ids)
            plain_ms.append(sp.query_ms())
        q["host_path_wall_ms"] = summary(host)
        q["device_path_wall_ms"] = summary(dev)
        q["raw_call_wall_ms"] = summary(raw)
        q["an_stream_ms"] = summary(an_ms)
        q["sp_stream_ms"] = summary(sp_ms)
        q["stream_ms"] = summary(x + y for x, y in zip(an_ms, sp_ms))
        q["zk_sp_summaries_wall_ms"] = summary(plain_wall)
        q["zk_sp_summaries_stream_ms"] = summary(plain_ms)
        q["wall_ratio_host_over_device"] = q["host_path_wall_ms"]["median"] / q["device_path_wall_ms"]["median"]
        res["queries"] = q

    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "measure.json").write_text(json.dumps(res, indent=1) + "\n")
    fmt = lambda d: f"{d['median']:10.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    lines = [f"annot_adjust_measure{' (' + a.label + ')' if a.label else ''}: {n} records, {ntr} traces, S = {S}, seed {a.seed}, "
             f"{res['device']}; ms, median [min, max] of {a.runs} runs, first call apart",
             f" span store: {res['span_store']['entries']} entries in {res['span_store']['segments']} segment(s); annotation store: "
             f"{res['annotation_store']['entries']} rows in {res['annotation_store']['segments']} segments",
             f" {q['ids']} ids: {q['summaries']} summaries, {q['span_rows']} span rows, {q['annotation_rows']} annotation rows, "
             f"{q['adjusted_spans']} spans after the adjuster, {q['entries']} entries; {q['annotated']} annotated, {q['overflowed']} overflowed",
             " getTraceSummariesByIds(adjust=TIME_SKEW, annotations=), the two paths alternating, the answers equal",
             f"  host path (the baseline), wall               {fmt(q['host_path_wall_ms'])}",
             f"  adjust_on_device=True, wall                  {fmt(q['device_path_wall_ms'])}   "
             f"{q['wall_ratio_host_over_device']:.1f} x faster",
             f"  zk_an_adjusted_summaries (both calls), wall  {fmt(q['raw_call_wall_ms'])}",
             f"  its filling call: zk_an_query_ms             {fmt(q['an_stream_ms'])}",
             f"                    zk_sp_query_ms (zk_sp_traces' passes) {fmt(q['sp_stream_ms'])}",
             f"                    both streams               {fmt(q['stream_ms'])}",
             " unadjusted, the same ids",
             f"  getTraceSummariesByIds(on_device=True), wall {fmt(q['zk_sp_summaries_wall_ms'])}",
             f"  zk_sp_summaries: zk_sp_query_ms              {fmt(q['zk_sp_summaries_stream_ms'])}"]
    (outdir / "measure.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
