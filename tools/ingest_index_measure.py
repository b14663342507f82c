#!/usr/bin/env python3
"""Measurement of the device decoder's index pass, recorded, not gated: bench.py does not
run it, and no number here has an earlier one to compare with.

Workload: the ingest benchmark's stored fragments (bench.py's generator, imported: a ~200k-fragment set
of Snappy(thrift Span) from tracegen records, replicated on the device to --fragments). In one process,
warmed, the calls alternate run by run so that whatever else the machine does meets all of them; reported
as the median and range of --runs runs, the first call apart:
  - zk_ingest_dev_spans, zk_ingest_dev_spans_items, zk_ingest_dev_spans_indexed without and with items
    (wall time of the wrapper's call: it allocates the item / entry tensors; the decode waits for its
    results), the index pass's own time between its first and last launch by device events
    (zk_ingest_dev_index_stats) and the slices it ran in;
  - zk_ax_observe of the entry columns the indexed call left in HBM, into an emptied index;
  - the path this replaces, on the fragment set as the benchmark's cpu_baseline takes it: the host decoder
    zk_ingest_spans_indexed (its own pool of up to 16 threads, warm) plus zk_ax_observe from the host columns
    it fills, as fragments per second of both steps together against the device's two steps together.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=20_000_000)
    ap.add_argument("--services", type=int, default=500)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ingest_index"))
    a = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("ingest_index_measure needs a HIP device")
    import bench
    from zipkin_amd import DeviceColumns, TraceAnnotationIndex, tracegen_host
    from zipkin_amd.ingest import DeviceSpanDecoder, SpanDecoder

    dev = torch.device("cuda", 0)
    base = tracegen_host(a.seed, 9000, max_depth=a.max_depth, num_services=a.services)
    blobs = bench._thrift_fragments(base, a.services)
    m = len(blobs)
    reps = max(1, a.fragments // m)
    n = m * reps
    lens = np.array([len(b) for b in blobs], np.int64)
    buf = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).to(dev).repeat(reps)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(np.tile(lens, reps))
    off = torch.from_numpy(offs).to(dev)
    S = max(4096, a.services)
    dec = DeviceSpanDecoder(S)
    cols = DeviceColumns(n, device="cuda:0")
    runs = a.runs + 1

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    calls = {
        "spans": lambda: dec.decode_device(buf, off, n, out=cols),
        "spans_items": lambda: dec.decode_device(buf, off, n, out=cols, items=True, item_cap=2 * n),
        "spans_indexed": lambda: dec.decode_device(buf, off, n, out=cols, indexed=True, index_cap=2 * n + 16),
        "spans_indexed_items": lambda: dec.decode_device(buf, off, n, out=cols, items=True, item_cap=2 * n, indexed=True,
                                                         index_cap=2 * n + 16),
    }
    ms = {k: [] for k in calls}
    pass_ms = {"spans_indexed": [], "spans_indexed_items": []}
    obs_wall, obs_dev = [], []
    slices = entries = 0
    with TraceAnnotationIndex(S, device=0, timing=True) as ax:
        for _ in range(runs):
            for k, fn in calls.items():
                t, r = wall(fn)
                assert r[1] == 0 and r[0].n == n
                ms[k].append(t)
                if k in pass_ms:
                    st = dec.index_stats()
                    pass_ms[k].append(st["pass_ms"])
                    slices = st["slices"]
                if k == "spans_indexed":
                    ent = r[2]
                    entries = len(ent)
                    ax.reset()
                    obs_wall.append(wall(lambda: ax.observe(ent, sync=True))[0])
                    obs_dev.append(sum(ax.observe_ms().values()))
                del r
        # the path the device call replaces: the host decoder's entries, observed from host columns
        hd = SpanDecoder()
        _, _, hitems = hd.decode_indexed(blobs, item_cap=2 * m + 16)
        host_dec, host_obs = [], []
        for _ in range(runs):
            t0 = time.perf_counter()
            _, _, hitems = hd.decode_indexed(blobs, item_cap=2 * m + 16)
            host_dec.append((time.perf_counter() - t0) * 1e3)
            ax.reset()
            host_obs.append(wall(lambda: ax.observe(hitems, sync=True))[0])
    host_entries = len(hitems)
    res = {"fragments": n, "set": m, "replicas": reps, "input_bytes": int(offs[-1]), "entries": entries,
           "entries_per_fragment": entries / n, "slices": slices, "device": torch.cuda.get_device_name(0), "seed": a.seed,
           "services": a.services,
           "calls_ms": {k: summary(v) for k, v in ms.items()},
           "index_pass_ms": {k: summary(v) for k, v in pass_ms.items()},
           "ax_observe_device_columns": {"wall_ms": summary(obs_wall), "device_ms": summary(obs_dev)},
           "host_path": {"fragments": m, "entries": host_entries, "cpu": bench.cpu_model(),
                         "zk_ingest_spans_indexed_ms": summary(host_dec), "ax_observe_host_columns_ms": summary(host_obs)}}
    d_ms = res["calls_ms"]["spans_indexed"]["median"] + res["ax_observe_device_columns"]["wall_ms"]["median"]
    h_ms = res["host_path"]["zk_ingest_spans_indexed_ms"]["median"] + res["host_path"]["ax_observe_host_columns_ms"]["median"]
    res["device_fragments_per_s"] = n / (d_ms * 1e-3)
    res["host_fragments_per_s"] = m / (h_ms * 1e-3)
    res["device_over_host"] = res["device_fragments_per_s"] / res["host_fragments_per_s"]
    assert host_entries * reps == entries, "the device call and the host decoder give different entry counts"

    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "measure.json").write_text(json.dumps(res, indent=1) + "\n")
    fmt = lambda d: f"{d['median']:10.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    c, p, h = res["calls_ms"], res["index_pass_ms"], res["host_path"]
    lines = [f"ingest_index_measure: {n} fragments ({m} x {reps}), {res['input_bytes'] / n:.1f} B each compressed, {entries} entries "
             f"({res['entries_per_fragment']:.3f} per fragment), {res['device']}; ms, median [min, max] of {a.runs} runs, first call apart",
             f" zk_ingest_dev_spans                        {fmt(c['spans'])}",
             f" zk_ingest_dev_spans_items                  {fmt(c['spans_items'])}",
             f" zk_ingest_dev_spans_indexed                {fmt(c['spans_indexed'])}",
             f"   its index pass (device events)           {fmt(p['spans_indexed'])}   in {slices} slices",
             f" zk_ingest_dev_spans_indexed with items     {fmt(c['spans_indexed_items'])}",
             f"   its index pass (device events)           {fmt(p['spans_indexed_items'])}",
             f" zk_ax_observe of the device columns, wall  {fmt(res['ax_observe_device_columns']['wall_ms'])}",
             f"   its passes (device)                      {fmt(res['ax_observe_device_columns']['device_ms'])}",
             f" host path on the {m}-fragment set ({h['cpu']}, up to 16 threads, warm):",
             f"   zk_ingest_spans_indexed                  {fmt(h['zk_ingest_spans_indexed_ms'])}",
             f"   zk_ax_observe of the host columns, wall  {fmt(h['ax_observe_host_columns_ms'])}",
             f" decode + observe: device {res['device_fragments_per_s']:.4g} fragments/s, host {res['host_fragments_per_s']:.4g} "
             f"fragments/s: {res['device_over_host']:.1f} x"]
    (outdir / "measure.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
