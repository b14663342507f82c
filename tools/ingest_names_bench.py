#!/usr/bin/env python3
"""Cost of ZK_INGEST_SPAN_NAMES on the device decoder, on bench.py's ingest fragments (its
synthesiser, imported: ~200k Snappy(thrift Span) fragments from tracegen records, replicated on the
device to --fragments; every span of that set is named "rpc").

One names-capable decoder per entry point (zk_ingest_dev_spans, zk_ingest_dev_spans_items). Each is
warmed without the flag, then decodes with it:
  cold    the first batch with the flag: the dictionary is empty, so every fragment's name misses the
          table, is copied to the scratch and goes through the second publish list, D3 and D4 (this
          batch also grows the per-batch arrays by the span names' columns)
  steady  the following batches: every name resolves inside the decode kernel
and the flag-less decode on the same decoder (the kNames = false kernels) is timed the same way.
Per decode, HIP events on the decoder's stream, the median of --steps after --warmup.

Prints one JSON line with the times in ms and the ratios names / plain.

    python tools/ingest_names_bench.py [--fragments N] [--steps K] [--warmup W]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=20_000_000)
    ap.add_argument("--services", type=int, default=500)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from zipkin_amd import tracegen_host
    from zipkin_amd.ingest import DeviceSpanDecoder

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
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

    def timed(dec, cols, items, span_names):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        r = dec.decode_device(buf, off, n, out=cols, items=items, item_cap=2 * n if items else None,
                              span_names=span_names)
        ev1.record(stream)
        torch.cuda.synchronize()
        assert r[1] == 0 and r[0].n == n
        return r[0], ev0.elapsed_time(ev1)

    def median(dec, cols, items, span_names):
        ts = []
        for i in range(a.warmup + a.steps):
            cols, t = timed(dec, cols, items, span_names)
            if i >= a.warmup:
                ts.append(t)
        return cols, {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}

    out = {"fragments": n, "bytes_in": int(offs[-1]), "distinct_span_names": 1, "steps": a.steps, "warmup": a.warmup}
    for items in (False, True):
        dec = DeviceSpanDecoder(max(4096, a.services), max_span_names=1024, stream=stream.cuda_stream)
        cols, plain = median(dec, None, items, False)
        assert dec.num_span_names == 0
        cols, cold = timed(dec, cols, items, True)
        assert dec.num_span_names == 1
        cols, steady = median(dec, cols, items, True)
        cols, plain_after = median(dec, cols, items, False)
        high = cols.flags[:4096].cpu().numpy().astype(np.uint32) >> 16
        assert not high.any()  # the flag-less decode writes no name bits
        key = "spans_items" if items else "spans"
        out[key] = {"plain": plain, "plain_after_names": plain_after, "names_cold_ms": cold, "names_steady": steady,
                    "steady_over_plain": steady["median_ms"] / plain["median_ms"],
                    "cold_over_plain": cold / plain["median_ms"]}
        dec.close()
        del cols
    print(json.dumps(out))


if __name__ == "__main__":
    main()
