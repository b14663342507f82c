#!/usr/bin/env python3
"""Measurement of the device decoder's rows pass, recorded, not gated: bench.py does not run
it, and no number here has an earlier one to compare with.

Workload: the ingest benchmark's stored fragments, the set tools/ingest_index_measure.py uses (bench.py's
generator, imported: a ~200k-fragment set of Snappy(thrift Span) from tracegen records, replicated on the
device to --fragments). Before anything is timed the device call's rows of one replica are compared, equal
and in order, with the host decoder's (service ids through names). Then, in one process, warmed, the calls
alternate run by run so that whatever else the machine does meets all of them; reported as the median and
range of --runs runs, the first call apart:
  - zk_ingest_dev_spans, zk_ingest_dev_spans_annotated with strings and with ZK_INGEST_NO_ROW_STRINGS (wall
    time of the wrapper's call: it allocates the row tensors; the decode waits for its results), the rows
    pass's own time between its first and last launch by device events (zk_ingest_dev_rows_stats) and the
    slices it ran in;
  - zk_ingest_dev_spans_indexed and its index pass, for scale;
  - zk_an_observe of the row columns the annotated call left in HBM, into an emptied store;
  - the path this replaces, on the fragment set as the benchmark's cpu_baseline takes it: the host decoder
    zk_ingest_spans_annotated (its own pool of up to 16 threads, warm) plus zk_an_observe from the host
    columns it fills, as fragments per second of both steps together against the device's two steps.
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ingest_annot"))
    a = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("ingest_annot_measure needs a HIP device")
    import bench
    from zipkin_amd import AnnotationRows, DeviceColumns, TraceAnnotationStore, tracegen_host
    from zipkin_amd.annotstore import ROW_COLUMNS
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

    # the two paths give the same rows (one replica, a decoder of its own), before anything is timed
    hd = SpanDecoder()
    _, hrej, hrows = hd.decode_annotated(blobs, row_cap=16 * m + 16)
    chk = DeviceSpanDecoder(S)
    _, drej, drows = chk.decode_device(buf, off, m, annotated=True, row_cap=16 * m + 16)
    host_rows = len(hrows)
    assert hrej == drej == 0 and len(drows) == host_rows

    def named(rows, names):
        nm = np.array(names + [""], dtype=object)
        svc = np.where(rows.bits & 8, rows.service_id, len(names))
        return [rows.trace_id, rows.span_id, rows.ts, rows.value, rows.ipv4, rows.bits], nm[svc].tolist()

    dh = AnnotationRows(*[getattr(drows, k).cpu().numpy().view(dt) for k, dt in ROW_COLUMNS])
    (hc, hn), (dc, dn) = named(hrows, hd.service_names()), named(dh, chk.service_names())
    assert all(np.array_equal(x, y) for x, y in zip(hc, dc)) and hn == dn, "the device call and the host decoder give different rows"
    assert all(chk.string(int(h)) == hd.string(int(h)) for h in np.unique(hrows.value)), "a row value's text differs"
    chk.close()
    del drows, dh

    dec = DeviceSpanDecoder(S)
    cols = DeviceColumns(n, device="cuda:0")
    runs = a.runs + 1
    rcap = host_rows * reps + 16

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    calls = {
        "spans": lambda: dec.decode_device(buf, off, n, out=cols),
        "spans_annotated": lambda: dec.decode_device(buf, off, n, out=cols, annotated=True, row_cap=rcap),
        "spans_annotated_no_strings": lambda: dec.decode_device(buf, off, n, out=cols, annotated=True, row_cap=rcap,
                                                                row_strings=False),
        "spans_indexed": lambda: dec.decode_device(buf, off, n, out=cols, indexed=True, index_cap=2 * n + 16),
    }
    ms = {k: [] for k in calls}
    pass_ms = {"spans_annotated": [], "spans_annotated_no_strings": [], "spans_indexed": []}
    obs_wall, obs_dev = [], []
    slices = rows = 0
    with TraceAnnotationStore(device=0, timing=True) as an:
        for _ in range(runs):
            for k, fn in calls.items():
                t, r = wall(fn)
                assert r[1] == 0 and r[0].n == n
                ms[k].append(t)
                if k == "spans_indexed":
                    pass_ms[k].append(dec.index_stats()["pass_ms"])
                elif k in pass_ms:
                    st = dec.rows_stats()
                    pass_ms[k].append(st["pass_ms"])
                    slices = st["slices"]
                if k == "spans_annotated":
                    got = r[2]
                    rows = len(got)
                    an.reset()
                    obs_wall.append(wall(lambda: an.observe(got, sync=True))[0])
                    obs_dev.append(sum(an.observe_ms().values()))
                del r
        # the path the device call replaces: the host decoder's rows, observed from host columns
        host_dec, host_obs = [], []
        for _ in range(runs):
            t0 = time.perf_counter()
            _, _, hrows = hd.decode_annotated(blobs, row_cap=16 * m + 16)
            host_dec.append((time.perf_counter() - t0) * 1e3)
            an.reset()
            host_obs.append(wall(lambda: an.observe(hrows, sync=True))[0])
    assert host_rows * reps == rows, "the device call and the host decoder give different row counts"
    res = {"fragments": n, "set": m, "replicas": reps, "input_bytes": int(offs[-1]), "rows": rows,
           "rows_per_fragment": rows / n, "slices": slices, "device": torch.cuda.get_device_name(0), "seed": a.seed,
           "services": a.services,
           "calls_ms": {k: summary(v) for k, v in ms.items()},
           "pass_ms": {k: summary(v) for k, v in pass_ms.items()},
           "an_observe_device_columns": {"wall_ms": summary(obs_wall), "device_ms": summary(obs_dev)},
           "host_path": {"fragments": m, "rows": host_rows, "cpu": bench.cpu_model(),
                         "zk_ingest_spans_annotated_ms": summary(host_dec), "an_observe_host_columns_ms": summary(host_obs)}}
    d_ms = res["calls_ms"]["spans_annotated"]["median"] + res["an_observe_device_columns"]["wall_ms"]["median"]
    h_ms = res["host_path"]["zk_ingest_spans_annotated_ms"]["median"] + res["host_path"]["an_observe_host_columns_ms"]["median"]
    res["device_fragments_per_s"] = n / (d_ms * 1e-3)
    res["host_fragments_per_s"] = m / (h_ms * 1e-3)
    res["device_over_host"] = res["device_fragments_per_s"] / res["host_fragments_per_s"]
    res["index_pass_over_rows_pass"] = res["pass_ms"]["spans_indexed"]["median"] / res["pass_ms"]["spans_annotated"]["median"]

    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "measure.json").write_text(json.dumps(res, indent=1) + "\n")
    fmt = lambda d: f"{d['median']:10.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    c, p, h = res["calls_ms"], res["pass_ms"], res["host_path"]
    lines = [f"ingest_annot_measure: {n} fragments ({m} x {reps}), {res['input_bytes'] / n:.1f} B each compressed, {rows} rows "
             f"({res['rows_per_fragment']:.3f} per fragment), {res['device']}; ms, median [min, max] of {a.runs} runs, first call apart",
             " rows of one replica: device == host, in order, ids through names, every value's text equal",
             f" zk_ingest_dev_spans                          {fmt(c['spans'])}",
             f" zk_ingest_dev_spans_annotated                {fmt(c['spans_annotated'])}",
             f"   its rows pass (device events)              {fmt(p['spans_annotated'])}   in {slices} slices",
             f" ... with ZK_INGEST_NO_ROW_STRINGS            {fmt(c['spans_annotated_no_strings'])}",
             f"   its rows pass (device events)              {fmt(p['spans_annotated_no_strings'])}",
             f" zk_ingest_dev_spans_indexed (for scale)      {fmt(c['spans_indexed'])}",
             f"   its index pass (device events)             {fmt(p['spans_indexed'])}   {res['index_pass_over_rows_pass']:.1f} x the rows pass",
             f" zk_an_observe of the device columns, wall    {fmt(res['an_observe_device_columns']['wall_ms'])}",
             f"   its passes (device)                        {fmt(res['an_observe_device_columns']['device_ms'])}",
             f" host path on the {m}-fragment set ({h['cpu']}, up to 16 threads, warm):",
             f"   zk_ingest_spans_annotated                  {fmt(h['zk_ingest_spans_annotated_ms'])}",
             f"   zk_an_observe of the host columns, wall    {fmt(h['an_observe_host_columns_ms'])}",
             f" decode + observe: device {res['device_fragments_per_s']:.4g} fragments/s, host {res['host_fragments_per_s']:.4g} "
             f"fragments/s: {res['device_over_host']:.1f} x"]
    (outdir / "measure.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
