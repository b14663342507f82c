#!/usr/bin/env python3
"""Cost of the per-link duration histogram (zk_lh_*) on the C2 batch: 1e8 records, 500 services,
seed 2, generated on the device (zk_tracegen_device), accumulated clustered and unverified as bench.py
does, timed with the ctx's HIP events (zk_config.timing).

Prints one JSON line: per accumulate, join_ms / reduce_ms (K2 + K3) without a handle and with one
bound, link_hist_ms (k_lh_tiles), its ratio to reduce_ms and to one read of the batch's links at the
rate the reduce moves its own traffic (K2 reads and writes every link, K3 reads it: 24 B per link in
reduce_ms), and the wall time of zk_lh_quantiles_all over all S x S edges. Each figure is the median
of --steps serial steps after --warmup unrecorded ones.

    python tools/link_hist_bench.py [--records N] [--services S] [--sub-bits M] [--steps K]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--services", type=int, default=500)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--sub-bits", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import torch

    from zipkin_amd import DepsContext, DeviceColumns, tracegen_params
    from zipkin_amd.realtime import LinkHistogram

    S = a.services
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = DepsContext(S, stream=stream.cuda_stream, timing=True)
    p = tracegen_params(a.seed, a.records // 15 + 1000, target_records=a.records, max_depth=6, num_services=S)
    cols = DeviceColumns(a.records)
    n, _ = ctx.tracegen_device(p, cols)
    torch.cuda.synchronize()

    def steps(reset_extra=None):
        rows = []
        for i in range(a.warmup + a.steps):
            ctx.reset()
            if reset_extra:
                reset_extra()
            ctx.accumulate(cols, clustered=True, verify=False, n=n)
            t = ctx.timing()  # (syncs) the last accumulate's events
            if i >= a.warmup:
                rows.append(t)
        return {k: statistics.median(r[k] for r in rows) for k in ("join_ms", "reduce_ms", "link_hist_ms")}, \
               {k: [min(r[k] for r in rows), max(r[k] for r in rows)] for k in ("join_ms", "reduce_ms", "link_hist_ms")}

    unbound, unbound_range = steps()
    links = ctx.stats()["joined_links"]
    lh = LinkHistogram(S, stream=stream.cuda_stream, sub_bits=a.sub_bits)
    lh.bind(ctx)
    bound, bound_range = steps(lh.reset)
    # the query over every edge: wall time, the first call (it allocates its buffers) apart
    qt = []
    for _ in range(4):
        t0 = time.perf_counter()
        lo, hi, cnt = lh.quantiles_all((0.5, 0.99))
        qt.append((time.perf_counter() - t0) * 1e3)
    assert int(cnt.sum()) == links, (int(cnt.sum()), links)
    reduce_rate = links * 24 / (bound["reduce_ms"] * 1e-3)  # B/s over K2's read + write and K3's read
    one_read_ms = links * 8 / reduce_rate * 1e3
    out = {
        "records": n, "services": S, "sub_bits": lh.m, "bins": lh.bins, "links": links,
        "hist_bytes": S * S * lh.bins * 4,
        "unbound_ms": unbound, "unbound_min_max": unbound_range,
        "bound_ms": bound, "bound_min_max": bound_range,
        "link_hist_over_reduce": bound["link_hist_ms"] / bound["reduce_ms"],
        "reduce_rate_GBs": reduce_rate / 1e9,
        "one_read_of_links_ms": one_read_ms,
        "link_hist_over_one_read": bound["link_hist_ms"] / one_read_ms,
        "quantiles_all_first_ms": qt[0], "quantiles_all_ms": statistics.median(qt[1:]),
        "present_edges": int((cnt > 0).sum()),
    }
    print(json.dumps(out))
    lh.close()
    ctx.close()


if __name__ == "__main__":
    main()
