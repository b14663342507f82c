#!/usr/bin/env python3
"""Measurement of the combined rows pass, recorded, not gated: bench.py does not run it.

Workload: the fragment set of tools/ingest_annot_measure.py (bench.py's generator: ~200k Snappy(thrift Span)
fragments, three time annotations and ONE binary annotation each, replicated on the device to --fragments), so the
lines compare with profiles/ingest_annot/. Before anything is timed the combined call's binary rows of one
replica are compared, equal and in order, with the host decoder's (service ids through names), and every key and
value answers with the host's bytes. Then, in one process, warmed, the calls alternate run by run; reported as
the median and range of --runs runs, the first call apart:
  - binary rows per fragment and distinct values;
  - zk_ingest_dev_spans_annotated_binary (wall time of the wrapper's call) and its rows pass between its first
    and last launch by device events (zk_ingest_dev_rows_stats), with strings and with ZK_INGEST_NO_ROW_STRINGS;
  - zk_ingest_dev_spans_annotated alone and its rows pass: the combined pass over the annotated-only pass is the
    price of the second list over one shared decompression;
  - zk_bn_observe of the binary row columns the call left in HBM, into an emptied store;
  - the host decoder's combined call zk_ingest_spans_annotated_binary on the fragment set, and zk_bn_observe from
    its host columns; the end-to-end rate of both paths (decode + both observes).

--ab LIB: the A/B of the EXISTING call zk_ingest_dev_spans_annotated between this tree's library and LIB (the
parent commit's, built beside it: tools/build_variant.py parent --rev <parent>). The two libraries alternate,
--runs child processes each, every child under its own time limit; a child loads ONE library through plain
ctypes (the parent's lacks the new symbols the binding checks), warms the call and reports the median of
--calls calls and of their rows passes. The new median is set against the parent's [min, max] of the same run.
Writes <out>/ingest_ab.txt and adds "ab" to measure.json when that exists.

Writes <out>/measure.json and <out>/measure.txt. Needs a gfx950 device."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def summary(xs):
    xs = list(xs)
    return {"first": xs[0], "median": statistics.median(xs[1:]), "min": min(xs[1:]), "max": max(xs[1:]), "runs": len(xs) - 1}


def fragment_set(a):
    import numpy as np

    import bench
    from zipkin_amd import tracegen_host

    base = tracegen_host(a.seed, 9000, max_depth=a.max_depth, num_services=a.services)
    blobs = bench._thrift_fragments(base, a.services)
    return blobs, np.array([len(b) for b in blobs], np.int64)


def on_device(blob_bytes, lens, fragments):
    import numpy as np
    import torch

    dev = torch.device("cuda", 0)
    m = len(lens)
    reps = max(1, fragments // m)
    n = m * reps
    buf = torch.from_numpy(np.frombuffer(blob_bytes, np.uint8).copy()).to(dev).repeat(reps)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(np.tile(lens, reps))
    return buf, torch.from_numpy(offs).to(dev), n, reps, int(offs[-1])


# ---- the A/B child: one library, the annotated call alone, through plain ctypes ------------------------------------
class _Rows(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("trace_id", "span_id", "ts", "value", "ipv4", "service_id", "bits")] + [("cap", C.c_uint64), ("n", C.c_uint64)]


class _Cols(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("trace_id", "span_id", "parent_id", "first_ts", "last_ts", "service_id", "flags")]


def child(a):
    import numpy as np
    import torch

    z = np.load(a.child)
    buf, off, n, reps, _ = on_device(z["bytes"].tobytes(), z["lens"], a.fragments)
    L = C.CDLL(a.lib)
    P, U64P = C.c_void_p, C.POINTER(C.c_uint64)
    L.zk_ingest_dev_create.argtypes = [C.c_int32, P, C.c_uint32, C.POINTER(P)]
    L.zk_ingest_dev_destroy.argtypes = [P]
    L.zk_ingest_dev_spans_annotated.argtypes = [P, P, P, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(_Cols), U64P, U64P, P, C.POINTER(_Rows)]
    L.zk_ingest_dev_rows_stats.argtypes = [P, C.POINTER(C.c_double), U64P]
    h = P()
    assert L.zk_ingest_dev_create(0, None, max(4096, a.services), C.byref(h)) == 0
    cap = 4 * n + 16
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device="cuda")  # noqa: E731
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device="cuda")  # noqa: E731
    ct = [i64(n) for _ in range(5)] + [i32(n), i32(n)]
    rt = [i64(cap) for _ in range(4)] + [i32(cap) for _ in range(3)]
    cols = _Cols(*[t.data_ptr() for t in ct])
    wall, pas = [], []
    for _ in range(a.calls + 2):  # two warming calls
        rows = _Rows(*[t.data_ptr() for t in rt], cap, 0)
        nout, nrej = C.c_uint64(), C.c_uint64()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = L.zk_ingest_dev_spans_annotated(h, buf.data_ptr(), off.data_ptr(), n, 1, 0, C.byref(cols), C.byref(nout), C.byref(nrej), None,
                                             C.byref(rows))
        wall.append((time.perf_counter() - t0) * 1e3)
        assert st == 0 and nout.value == n and nrej.value == 0, (st, nout.value, nrej.value)
        ms, sl = C.c_double(), C.c_uint64()
        assert L.zk_ingest_dev_rows_stats(h, C.byref(ms), C.byref(sl)) == 0
        pas.append(ms.value)
    L.zk_ingest_dev_destroy(h)
    print(json.dumps({"call_ms": statistics.median(wall[2:]), "pass_ms": statistics.median(pas[2:]), "rows": int(rows.n), "fragments": n,
                      "slices": int(sl.value)}))


def ab(a):
    import numpy as np

    blobs, lens = fragment_set(a)
    tree = str(ROOT / "zipkin_amd" / "libzkagg.so")
    libs = {"parent": str(Path(a.ab).resolve()), "tree": tree}
    got = {k: [] for k in libs}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "set.npz")
        np.savez(path, bytes=np.frombuffer(b"".join(blobs), np.uint8), lens=lens)
        for r in range(a.runs):
            for k, lib in libs.items():
                p = subprocess.run([sys.executable, __file__, "--child", path, "--lib", lib, "--fragments", str(a.fragments), "--calls",
                                    str(a.calls), "--services", str(a.services)], capture_output=True, text=True, timeout=a.child_timeout)
                if p.returncode != 0:  # (nothing more is started after a failure)
                    raise SystemExit(f"A/B child ({k}, run {r}) ended with {p.returncode}:\n{p.stdout}\n{p.stderr}")
                got[k].append(json.loads(p.stdout.strip().splitlines()[-1]))
    res = {"runs": a.runs, "calls_per_run": a.calls, "fragments": got["tree"][0]["fragments"], "rows": got["tree"][0]["rows"]}
    for k in libs:
        for f in ("call_ms", "pass_ms"):
            xs = [g[f] for g in got[k]]
            res[f"{k}_{f}"] = {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}
    assert got["tree"][0]["rows"] == got["parent"][0]["rows"]
    for f in ("call_ms", "pass_ms"):
        t, p = res[f"tree_{f}"]["median"], res[f"parent_{f}"]
        res[f"{f}_verdict"] = "inside the parent's range" if p["min"] <= t <= p["max"] else ("below the parent's minimum" if t < p["min"] else
                                                                                              "ABOVE the parent's maximum")
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    fmt = lambda d: f"{d['median']:9.3f}  [{d['min']:.3f}, {d['max']:.3f}]"  # noqa: E731
    lines = [f"zk_ingest_dev_spans_annotated, parent commit's library against this tree's: {res['fragments']} fragments, {res['rows']} rows; the two "
             f"alternate, {a.runs} processes each; per process the median of {a.calls} warm calls; ms, median [min, max] over the processes",
             f" parent  call {fmt(res['parent_call_ms'])}   rows pass {fmt(res['parent_pass_ms'])}",
             f" tree    call {fmt(res['tree_call_ms'])}   rows pass {fmt(res['tree_pass_ms'])}",
             f" the tree's median call is {res['call_ms_verdict']}; its median rows pass is {res['pass_ms_verdict']}"]
    (out / "ingest_ab.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    mj = out / "measure.json"
    if mj.exists():
        j = json.loads(mj.read_text())
        j["ab"] = res
        mj.write_text(json.dumps(j, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=20_000_000)
    ap.add_argument("--services", type=int, default=500)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ingest_binary"))
    ap.add_argument("--ab", default=None, help="the parent commit's library: run the A/B of zk_ingest_dev_spans_annotated instead")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=120)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("ingest_binary_measure needs a HIP device")
    if a.ab:
        return ab(a)
    import bench
    from zipkin_amd import DeviceColumns, TraceAnnotationStore, TraceBinaryAnnotationStore
    from zipkin_amd.ingest import DeviceSpanDecoder, SpanDecoder

    blobs, lens = fragment_set(a)
    m = len(blobs)
    buf, off, n, reps, in_bytes = on_device(b"".join(blobs), lens, a.fragments)
    S = max(4096, a.services)

    # the two paths give the same binary rows (one replica, a decoder of its own), before anything is timed
    hd = SpanDecoder()
    _, hrej, hrows, hb = hd.decode_annotated(blobs, row_cap=16 * m + 16, binary=True, binary_cap=16 * m + 16)
    chk = DeviceSpanDecoder(S)
    _, drej, drows, db = chk.decode_device(buf, off, m, annotated=True, row_cap=16 * m + 16, binary=True, binary_cap=16 * m + 16)
    assert hrej == drej == 0 and len(drows) == len(hrows) and len(db) == len(hb)
    dbh = db.to_host()

    def named(rows, names):
        nm = np.array(names + [""], dtype=object)
        svc = np.where(rows.bits & 8, rows.service_id, len(names))
        return [rows.trace_id, rows.span_id, rows.key, rows.value, rows.ipv4, rows.bits], nm[svc].tolist()

    (hc, hn), (dc, dn) = named(hb, hd.service_names()), named(dbh, chk.service_names())
    assert all(np.array_equal(x, y) for x, y in zip(hc, dc)) and hn == dn, "the device call and the host decoder give different binary rows"
    distinct = np.unique(np.concatenate([hb.key, hb.value]))
    assert all(chk.bytes(int(h)) == hd.bytes(int(h)) for h in distinct), "a key's or value's bytes differ"
    host_b, host_t, distinct_values = len(hb), len(hrows), len(np.unique(hb.value))
    chk.close()
    del drows, db, dbh

    dec = DeviceSpanDecoder(S)
    cols = DeviceColumns(n, device="cuda:0")
    runs = a.runs + 1
    rcap, bcap = host_t * reps + 16, host_b * reps + 16

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    calls = {
        "spans_annotated": lambda: dec.decode_device(buf, off, n, out=cols, annotated=True, row_cap=rcap),
        "spans_annotated_binary": lambda: dec.decode_device(buf, off, n, out=cols, annotated=True, row_cap=rcap, binary=True, binary_cap=bcap),
        "spans_annotated_binary_no_strings": lambda: dec.decode_device(buf, off, n, out=cols, annotated=True, row_cap=rcap, binary=True,
                                                                       binary_cap=bcap, row_strings=False),
    }
    ms = {k: [] for k in calls}
    pass_ms = {k: [] for k in calls}
    obs_wall, obs_dev, an_wall = [], [], []
    slices = {}
    brows = 0
    with TraceBinaryAnnotationStore(device=0, timing=True) as bn, TraceAnnotationStore(device=0, timing=True) as an:
        for _ in range(runs):
            for k, fn in calls.items():
                t, r = wall(fn)
                assert r[1] == 0 and r[0].n == n
                ms[k].append(t)
                st = dec.rows_stats()
                pass_ms[k].append(st["pass_ms"])
                slices[k] = st["slices"]
                if k == "spans_annotated_binary":
                    brows = len(r[3])
                    bn.reset()
                    an.reset()
                    obs_wall.append(wall(lambda: bn.observe(r[3], sync=True))[0])
                    obs_dev.append(sum(bn.observe_ms().values()))
                    an_wall.append(wall(lambda: an.observe(r[2], sync=True))[0])
                del r
        # the host decoder's combined call, observed from host columns
        host_dec, host_obs, host_an = [], [], []
        for _ in range(runs):
            t0 = time.perf_counter()
            _, _, hrows, hb = hd.decode_annotated(blobs, row_cap=16 * m + 16, binary=True, binary_cap=16 * m + 16)
            host_dec.append((time.perf_counter() - t0) * 1e3)
            bn.reset()
            an.reset()
            host_obs.append(wall(lambda: bn.observe(hb, sync=True))[0])
            host_an.append(wall(lambda: an.observe(hrows, sync=True))[0])
    assert host_b * reps == brows, "the device call and the host decoder give different row counts"
    res = {"fragments": n, "set": m, "replicas": reps, "input_bytes": in_bytes, "binary_rows": brows, "binary_rows_per_fragment": brows / n,
           "time_rows": host_t * reps, "distinct_values": distinct_values, "distinct_keys_and_values": int(len(distinct)), "slices": slices,
           "device": torch.cuda.get_device_name(0), "seed": a.seed, "services": a.services,
           "calls_ms": {k: summary(v) for k, v in ms.items()}, "pass_ms": {k: summary(v) for k, v in pass_ms.items()},
           "bn_observe_device_columns": {"wall_ms": summary(obs_wall), "device_ms": summary(obs_dev)},
           "an_observe_device_columns": {"wall_ms": summary(an_wall)},
           "host_path": {"fragments": m, "binary_rows": host_b, "time_rows": host_t, "cpu": bench.cpu_model(),
                         "zk_ingest_spans_annotated_binary_ms": summary(host_dec), "bn_observe_host_columns_ms": summary(host_obs),
                         "an_observe_host_columns_ms": summary(host_an)}}
    p = res["pass_ms"]
    res["combined_pass_over_annotated_pass"] = p["spans_annotated_binary"]["median"] / p["spans_annotated"]["median"]
    d_ms = (res["calls_ms"]["spans_annotated_binary"]["median"] + res["bn_observe_device_columns"]["wall_ms"]["median"] +
            res["an_observe_device_columns"]["wall_ms"]["median"])
    h = res["host_path"]
    h_ms = h["zk_ingest_spans_annotated_binary_ms"]["median"] + h["bn_observe_host_columns_ms"]["median"] + h["an_observe_host_columns_ms"]["median"]
    res["device_fragments_per_s"] = n / (d_ms * 1e-3)
    res["host_fragments_per_s"] = m / (h_ms * 1e-3)
    res["device_over_host"] = res["device_fragments_per_s"] / res["host_fragments_per_s"]

    outdir = Path(a.out)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "measure.json").write_text(json.dumps(res, indent=1) + "\n")
    fmt = lambda d: f"{d['median']:10.3f}  [{d['min']:.3f}, {d['max']:.3f}]  first {d['first']:.3f}"  # noqa: E731
    c = res["calls_ms"]
    lines = [f"ingest_binary_measure: {n} fragments ({m} x {reps}), {in_bytes / n:.1f} B each compressed, {brows} binary rows "
             f"({res['binary_rows_per_fragment']:.3f} per fragment; {distinct_values} distinct values, {len(distinct)} distinct keys and values), "
             f"{res['time_rows']} time rows, {res['device']}; ms, median [min, max] of {a.runs} runs, first call apart",
             " binary rows of one replica: device == host, in order, ids through names, every key's and value's bytes equal",
             f" zk_ingest_dev_spans_annotated_binary         {fmt(c['spans_annotated_binary'])}",
             f"   its rows pass, both lists (device events)  {fmt(p['spans_annotated_binary'])}   in {slices['spans_annotated_binary']} slices",
             f" ... with ZK_INGEST_NO_ROW_STRINGS            {fmt(c['spans_annotated_binary_no_strings'])}",
             f"   its rows pass (device events)              {fmt(p['spans_annotated_binary_no_strings'])}",
             f" zk_ingest_dev_spans_annotated alone          {fmt(c['spans_annotated'])}",
             f"   its rows pass (device events)              {fmt(p['spans_annotated'])}   in {slices['spans_annotated']} slices",
             f" combined rows pass / annotated-only rows pass: {res['combined_pass_over_annotated_pass']:.3f} x",
             f" zk_bn_observe of the device columns, wall    {fmt(res['bn_observe_device_columns']['wall_ms'])}",
             f"   its passes (device)                        {fmt(res['bn_observe_device_columns']['device_ms'])}",
             f" zk_an_observe of the time rows, wall         {fmt(res['an_observe_device_columns']['wall_ms'])}",
             f" host path on the {m}-fragment set ({h['cpu']}, up to 16 threads, warm):",
             f"   zk_ingest_spans_annotated_binary           {fmt(h['zk_ingest_spans_annotated_binary_ms'])}",
             f"   zk_bn_observe of the host columns, wall    {fmt(h['bn_observe_host_columns_ms'])}",
             f"   zk_an_observe of the host columns, wall    {fmt(h['an_observe_host_columns_ms'])}",
             f" decode + both observes: device {res['device_fragments_per_s']:.4g} fragments/s, host {res['host_fragments_per_s']:.4g} "
             f"fragments/s: {res['device_over_host']:.1f} x"]
    (outdir / "measure.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
