#!/usr/bin/env python3
"""Cost of a link-histogram snapshot (zk_lh_snapshot / zk_lh_merge) on the C2 batch: 1e8 records, 500
services, sub_bits 4, seed 2, generated on the device and accumulated once into a bound LinkHistogram;
then the same records with their services folded onto 71 of the 500 (service id mod 71), so that only
about 5,000 edges are present -- the shape of a real service graph.

Prints one JSON line per graph: rows, entries and snapshot bytes; the device time of the count pass
(with its scans), the write pass and the copy to the host (HIP events, zk_lh_snapshot_ms); the wall
time of snapshot() (with and without the copy into a bytes object) and, in the same run, of a dense
read() of the whole table -- what there was before snapshots, the number to compare with; and the wall
time of merge() of that snapshot into a fresh handle. Each wall figure is [median, min, max] (ms) of
--steps calls after one unrecorded call (the first allocates the scratch); the device times are medians.

    python tools/link_hist_snapshot_bench.py [--records N] [--services S] [--sub-bits M] [--steps K]
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
    ap.add_argument("--sub-bits", type=int, default=4)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--fold", type=int, default=71, help="services of the sparse graph")
    a = ap.parse_args()

    import numpy as np
    import torch

    from zipkin_amd import DepsContext, DeviceColumns, tracegen_params
    from zipkin_amd.realtime import LinkHistogram, LinkHistogramSnapshot

    S = a.services
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = DepsContext(S, stream=stream.cuda_stream)
    p = tracegen_params(a.seed, a.records // 15 + 1000, target_records=a.records, max_depth=6, num_services=S)
    cols = DeviceColumns(a.records)
    n, _ = ctx.tracegen_device(p, cols)
    torch.cuda.synchronize()
    lh = LinkHistogram(S, stream=stream.cuda_stream, sub_bits=a.sub_bits)
    lh.bind(ctx)
    fresh = LinkHistogram(S, sub_bits=a.sub_bits)

    def med(f):
        f()
        ts = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e3)
        return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]

    def measure(graph):
        ctx.reset()
        lh.reset()
        ctx.accumulate(cols, clustered=True, verify=False, n=n)
        ctx.sync()
        links = ctx.stats()["joined_links"]
        phases = []

        def snap_array():
            lh.snapshot(as_array=True)
            phases.append(lh.snapshot_ms())

        wall_array = med(snap_array)
        wall_bytes = med(lh.snapshot)
        dense = np.empty((S * S, lh.bins), np.uint32)

        def dense_read():  # (into a kept array: no page faults of a new one in the loop)
            lh._check(lh._L.zk_lh_read(lh._h, 0, S * S, dense.ctypes.data))

        wall_dense = med(dense_read)
        wall_dense_new = med(lh.read)
        blob = lh.snapshot()
        snap = LinkHistogramSnapshot(blob)
        assert snap.links == links, (snap.links, links)
        assert len(snap.entries) == int(np.count_nonzero(dense)) and len(snap) == int(dense.any(axis=1).sum())

        def merge():
            fresh.reset()
            fresh.merge(blob)

        wall_merge = med(merge)
        assert np.array_equal(fresh.read(), dense)
        ph = [round(statistics.median(x[k] for x in phases[1:]), 4) for k in range(3)]
        print(json.dumps({
            "graph": graph, "records": n, "services": S, "sub_bits": lh.m, "links": links,
            "rows": len(snap), "entries": len(snap.entries), "snapshot_bytes": len(blob),
            "dense_bytes": S * S * lh.bins * 4,
            "count_and_scan_ms": ph[0], "write_ms": ph[1], "copy_ms": ph[2],
            "snapshot_wall_ms": wall_array, "snapshot_to_bytes_wall_ms": wall_bytes,
            "dense_read_wall_ms": wall_dense, "dense_read_new_array_wall_ms": wall_dense_new,
            "merge_wall_ms": wall_merge,
        }), flush=True)

    measure("C2")
    cols.service_id.remainder_(a.fold)  # the same records, services folded onto `fold` ids
    torch.cuda.synchronize()
    measure(f"sparse ({a.fold} of {S} services)")
    fresh.close()
    lh.close()
    ctx.close()


if __name__ == "__main__":
    main()
