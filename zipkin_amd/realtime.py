"""RtSketch: per-service distinct traces (HyperLogLog) and duration quantiles (include/zksketch.h).

The realtime aggregates the reference declares but never implements (RealtimeAggregates.scala:26-38,
QueryService.scala:416-430): fed either from already-merged spans (`accumulate_merged`) or, bound
to a DepsContext, from the same K1 pass over span fragments that feeds the dependency path
(`bind`). Host-side names map service ids back to names, as for the dependency table.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi


def _ptr(a) -> int:
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


class RtSketch:
    def __init__(self, num_services: int, *, device: int = 0, stream: int | None = None, hll_p: int = 0,
                 sub_bits: int = 0, seed: int = 0):
        self._L = _abi.lib()
        cfg = _abi.zk_rt_config()
        cfg.num_services = num_services
        cfg.device = device
        cfg.stream = stream
        cfg.hll_p = hll_p
        cfg.sub_bits = sub_bits
        cfg.seed = seed
        h = C.c_void_p()
        st = self._L.zk_rt_create(C.byref(cfg), C.byref(h))
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, _abi.status_str(st))
        self._h = h
        self.num_services = num_services
        self.seed = seed
        r, b = C.c_uint32(), C.c_uint32()
        self._check(self._L.zk_rt_geometry(h, C.byref(r), C.byref(b)))
        self.registers, self.bins = r.value, b.value
        self.p = self.registers.bit_length() - 1
        self.m = sub_bits or 7
        self._bound = None

    def _check(self, st: int) -> None:
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_rt_last_error(self._h).decode() or _abi.status_str(st))

    def close(self) -> None:
        if getattr(self, "_h", None):
            if self._bound is not None:
                self.unbind()
            self._L.zk_rt_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def reset(self) -> None:
        self._check(self._L.zk_rt_reset(self._h))

    def bind(self, ctx, only: bool = False) -> None:
        """Feed this sketch from every later ctx.accumulate (only=True: skip the dependency path)."""
        mode = _abi.ZK_RT_ONLY if only else _abi.ZK_RT_WITH_DEPS
        st = self._L.zk_rt_bind(ctx.handle, self._h, mode)
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_last_error(ctx.handle).decode())
        self._bound = ctx

    def unbind(self) -> None:
        if self._bound is not None:
            self._L.zk_rt_bind(self._bound.handle, None, 0)
            self._bound = None

    def accumulate_merged(self, service_id, trace_id, duration) -> None:
        n = len(service_id)
        if hasattr(service_id, "data_ptr"):
            flags, s, t, d = _abi.ZK_BATCH_DEVICE_PTRS, service_id, trace_id, duration
        else:
            flags = 0
            s = np.ascontiguousarray(service_id, dtype=np.uint32)
            t = np.asarray(trace_id)
            t = np.ascontiguousarray(t.view(np.uint64) if t.dtype == np.int64 else t, dtype=np.uint64)
            d = np.ascontiguousarray(duration, dtype=np.int64)
        self._check(self._L.zk_rt_accumulate_merged(self._h, _ptr(s), _ptr(t), _ptr(d), n, flags))
        if flags:  # device batches the stream may still read (see DepsContext._hold)
            inflight = self.__dict__.setdefault("_inflight", [])
            inflight.append((s, t, d))
            if len(inflight) > 8:
                self._check(self._L.zk_rt_dropped(self._h, None, None))  # (synchronises the stream)
                inflight.clear()

    def distinct_traces(self) -> np.ndarray:
        out = np.zeros(self.num_services, np.float64)
        self._check(self._L.zk_rt_distinct_traces(self._h, out.ctypes.data))
        return out

    def quantiles(self, service: int, qs=(0.5, 0.99)):
        """([(lo, hi)] bin bounds holding each nearest-rank quantile, count)."""
        q = np.ascontiguousarray(qs, dtype=np.float64)
        lo = np.zeros(len(q), np.int64)
        hi = np.zeros(len(q), np.int64)
        cnt = C.c_uint64()
        self._check(self._L.zk_rt_quantiles(self._h, service, q.ctypes.data, len(q), lo.ctypes.data, hi.ctypes.data,
                                            C.byref(cnt)))
        return [(int(a), int(b)) for a, b in zip(lo, hi)], int(cnt.value)

    def quantiles_all(self, qs=(0.5, 0.99)):
        """(lo int64[S, nq], hi int64[S, nq], count uint64[S]) for every service at once
        (zk_rt_quantiles_all: one device pass and one copy)."""
        q = np.ascontiguousarray(qs, dtype=np.float64)
        S = self.num_services
        lo = np.zeros((S, len(q)), np.int64)
        hi = np.zeros((S, len(q)), np.int64)
        cnt = np.zeros(S, np.uint64)
        self._check(self._L.zk_rt_quantiles_all(self._h, q.ctypes.data, len(q), lo.ctypes.data, hi.ctypes.data,
                                                cnt.ctypes.data_as(_abi._U64P)))
        return lo, hi, cnt

    def tdigest(self, service: int, compression: float = 200.0, qs=(0.5, 0.99)):
        """(centroid means, centroid weights, t-digest estimates of qs, count) of one service's
        duration digest (zk_rt_tdigest: a merging t-digest over the exact histogram)."""
        q = np.ascontiguousarray(qs, dtype=np.float64)
        val = np.zeros(len(q), np.float64)
        n, cnt = C.c_uint32(), C.c_uint64()
        self._check(self._L.zk_rt_tdigest(self._h, service, compression, None, None, 0, C.byref(n), None, 0, None,
                                          None))
        mean = np.zeros(n.value, np.float64)
        weight = np.zeros(n.value, np.float64)
        self._check(self._L.zk_rt_tdigest(self._h, service, compression, mean.ctypes.data, weight.ctypes.data, n.value,
                                          C.byref(n), q.ctypes.data, len(q), val.ctypes.data, C.byref(cnt)))
        return mean, weight, val, int(cnt.value)

    def read(self):
        """(registers uint8[S, 2^p], histogram uint32[S, bins]) host copies."""
        regs = np.zeros((self.num_services, self.registers), np.uint8)
        hist = np.zeros((self.num_services, self.bins), np.uint32)
        self._check(self._L.zk_rt_read(self._h, regs.ctypes.data, hist.ctypes.data))
        return regs, hist

    def dropped(self) -> tuple[int, int]:
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._L.zk_rt_dropped(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def partial(self):
        """(registers ptr, bytes, histogram ptr, bytes): device buffers for MAX / SUM all-reduce."""
        rp, rb, hp, hb = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        self._check(self._L.zk_rt_partial(self._h, C.byref(rp), C.byref(rb), C.byref(hp), C.byref(hb)))
        return int(rp.value), int(rb.value), int(hp.value), int(hb.value)


class RealtimeLinks:
    """The realtime link store (zk_rl_*): every join row (parent service, child service, child
    duration, traceId, rpc = the child span's name id) of the dependency path since the last reset,
    kept in HBM and queried by server (child) service and rpc -- the state behind RealtimeAggregates (GpuRealtimeAggregates below in
    zipkin_amd/aggregates.py). Bound to a DepsContext, K1 writes the rows beside its links."""

    def __init__(self, num_services: int, *, device: int = 0, stream: int | None = None):
        self._L = _abi.lib()
        cfg = _abi.zk_rl_config()
        cfg.num_services = num_services
        cfg.device = device
        cfg.stream = stream
        h = C.c_void_p()
        st = self._L.zk_rl_create(C.byref(cfg), C.byref(h))
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, _abi.status_str(st))
        self._h = h
        self.num_services = num_services
        self._bound = None

    def _check(self, st: int) -> None:
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_rl_last_error(self._h).decode() or _abi.status_str(st))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.unbind()
            self._L.zk_rl_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bind(self, ctx) -> None:
        st = self._L.zk_rl_bind(ctx.handle, self._h)
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_last_error(ctx.handle).decode())
        self._bound = ctx

    def unbind(self) -> None:
        if self._bound is not None and getattr(self._bound, "_h", None):
            self._L.zk_rl_bind(self._bound.handle, None)
        self._bound = None

    def reset(self) -> None:
        self._check(self._L.zk_rl_reset(self._h))

    def count(self) -> tuple[int, int]:
        """(rows in the window, rows dropped past its capacity -- always 0)."""
        n, d = C.c_uint64(), C.c_uint64()
        self._check(self._L.zk_rl_count(self._h, C.byref(n), C.byref(d)))
        return int(n.value), int(d.value)

    def server_links(self, server: int):
        """(parent ids uint32, durations int64 us, traceIds uint64) of every row whose child service
        is `server`, ordered by (parent, duration, traceId)."""
        n = C.c_uint64()
        self._check(self._L.zk_rl_server_links(self._h, server, None, None, None, 0, C.byref(n)))
        m = int(n.value)
        par = np.zeros(max(1, m), np.uint32)
        dur = np.zeros(max(1, m), np.int64)
        tid = np.zeros(max(1, m), np.uint64)
        if m:
            self._check(self._L.zk_rl_server_links(self._h, server, par.ctypes.data, dur.ctypes.data, tid.ctypes.data,
                                                   m, C.byref(n)))
        return par[:m], dur[:m], tid[:m]

    def server_rpc_links(self, server: int, rpc: int | None = None):
        """(parent ids uint32, durations int64 us, traceIds uint64, rpc ids uint32) of the rows whose
        child service is `server` and whose rpc id -- the child span's name id, bits 16..31 of the
        record flags, 0 = no name -- is `rpc` (None: any rpc), ordered by (parent, duration, traceId,
        rpc). The filter runs on the device (zk_rl_server_rpc_links)."""
        r = _abi.ZK_RL_ANY_RPC if rpc is None else int(rpc)
        if not 0 <= r <= _abi.ZK_RL_ANY_RPC:
            raise _abi.ZkError(_abi.ZK_ERR_INVALID_ARG, "rpc name id out of range")
        n = C.c_uint64()
        self._check(self._L.zk_rl_server_rpc_links(self._h, server, r, None, None, None, None, 0, C.byref(n)))
        m = int(n.value)
        par = np.zeros(max(1, m), np.uint32)
        dur = np.zeros(max(1, m), np.int64)
        tid = np.zeros(max(1, m), np.uint64)
        ids = np.zeros(max(1, m), np.uint32)
        if m:
            self._check(self._L.zk_rl_server_rpc_links(self._h, server, r, par.ctypes.data, dur.ctypes.data,
                                                       tid.ctypes.data, ids.ctypes.data, m, C.byref(n)))
        return par[:m], dur[:m], tid[:m], ids[:m]


def link_hist_bins(m: int) -> int:
    """Bins of the log-linear duration histogram with m mantissa bits over [0, 2^40) us."""
    return (41 - m) << m


def link_hist_bin_bounds(b: int, m: int) -> tuple[int, int]:
    """[lo, hi] (us, inclusive) of bin b: the value itself below 2^m, else (exponent, top m mantissa
    bits) -- the layout of zk_rt's histogram, which zk_lh shares."""
    if b < (1 << m):
        return b, b
    e = (b >> m) + m - 1
    lo = ((1 << m) | (b & ((1 << m) - 1))) << (e - m)
    return lo, lo + (1 << (e - m)) - 1


class LinkHistogram:
    """Per-link duration histogram (zk_lh_*): for every (parent, child) edge of the dependency graph
    the exact count of its links' child durations per log-linear bin, hence the p50/p99 a
    DependencyLink's Moments cannot give. Bound to a DepsContext, every later accumulate feeds it from
    the links the dependency path reduces anyway. State: uint32[S * S, bins] in HBM (S * S * bins * 4
    bytes: 592 MB at S = 500 with the default sub_bits = 4), summed across traceId shards like the
    table (partial() / Comm.allreduce_lh)."""

    def __init__(self, num_services: int, *, device: int = 0, stream: int | None = None, sub_bits: int = 0):
        self._L = _abi.lib()
        cfg = _abi.zk_lh_config()
        cfg.num_services = num_services
        cfg.device = device
        cfg.stream = stream
        cfg.sub_bits = sub_bits
        h = C.c_void_p()
        st = self._L.zk_lh_create(C.byref(cfg), C.byref(h))
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, _abi.status_str(st))
        self._h = h
        self.num_services = num_services
        self.m = sub_bits or 4
        self.bins = self.geometry()
        self._bound = None

    def _check(self, st: int) -> None:
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_lh_last_error(self._h).decode() or _abi.status_str(st))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.unbind()
            self._L.zk_lh_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def geometry(self) -> int:
        """Bins per edge: (41 - m) << m."""
        b = C.c_uint32()
        self._check(self._L.zk_lh_geometry(self._h, C.byref(b)))
        return int(b.value)

    def bind(self, ctx) -> None:
        st = self._L.zk_lh_bind(ctx.handle, self._h)
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_last_error(ctx.handle).decode())
        self._bound = ctx

    def unbind(self) -> None:
        if self._bound is not None and getattr(self._bound, "_h", None):
            self._L.zk_lh_bind(self._bound.handle, None)
        self._bound = None

    def reset(self) -> None:
        self._check(self._L.zk_lh_reset(self._h))

    def quantiles(self, parent: int, child: int, qs=(0.5, 0.99)):
        """([(lo, hi)] bin bounds holding each nearest-rank quantile of one edge, its link count)."""
        q = np.ascontiguousarray(qs, dtype=np.float64)
        lo = np.zeros(len(q), np.int64)
        hi = np.zeros(len(q), np.int64)
        cnt = C.c_uint64()
        self._check(self._L.zk_lh_quantiles(self._h, parent, child, q.ctypes.data, len(q), lo.ctypes.data,
                                            hi.ctypes.data, C.byref(cnt)))
        return [(int(a), int(b)) for a, b in zip(lo, hi)], int(cnt.value)

    def quantiles_all(self, qs=(0.5, 0.99)):
        """(lo int64[S * S, nq], hi int64[S * S, nq], count uint64[S * S]) of every edge, cell =
        parent * S + child, in one device pass (zk_lh_quantiles_all)."""
        q = np.ascontiguousarray(qs, dtype=np.float64)
        cells = self.num_services * self.num_services
        lo = np.zeros((cells, len(q)), np.int64)
        hi = np.zeros((cells, len(q)), np.int64)
        cnt = np.zeros(cells, np.uint64)
        self._check(self._L.zk_lh_quantiles_all(self._h, q.ctypes.data, len(q), lo.ctypes.data, hi.ctypes.data,
                                                cnt.ctypes.data_as(_abi._U64P)))
        return lo, hi, cnt

    def read(self, first_cell: int = 0, n_cells: int | None = None) -> np.ndarray:
        """Host copy uint32[n_cells, bins] of the rows of cells [first_cell, first_cell + n_cells)."""
        if n_cells is None:
            n_cells = self.num_services * self.num_services - first_cell
        out = np.zeros((max(n_cells, 0), self.bins), np.uint32)
        self._check(self._L.zk_lh_read(self._h, first_cell, n_cells, out.ctypes.data))
        return out

    def partial(self) -> tuple[int, int]:
        """(device pointer, bytes) of the histogram: the buffer a u32 SUM all-reduce merges in place."""
        p, b = C.c_void_p(), C.c_uint64()
        self._check(self._L.zk_lh_partial(self._h, C.byref(p), C.byref(b)))
        return int(p.value or 0), int(b.value)

    def dropped(self) -> int:
        """Links dropped for a duration >= 2^40 us while bound, since reset."""
        d = C.c_uint64()
        self._check(self._L.zk_lh_dropped(self._h, C.byref(d)))
        return int(d.value)

    def snapshot(self, as_array: bool = False) -> bytes:
        """The canonical sparse snapshot of the state (zk_lh_snapshot: the present bins only,
        compacted on the device): what a store keeps beside a Dependencies record, and what merge(),
        LinkHistogramSnapshot.plus and a host without a GPU read back. as_array: the uint8 array the
        library wrote, without the copy into a bytes object."""
        n = C.c_uint64()
        self._check(self._L.zk_lh_snapshot(self._h, None, 0, C.byref(n)))
        buf = np.empty(n.value, np.uint8)
        self._check(self._L.zk_lh_snapshot(self._h, buf.ctypes.data, n.value, C.byref(n)))
        return buf[: n.value] if as_array else buf[: n.value].tobytes()

    def snapshot_ms(self) -> tuple[float, float, float]:
        """Device ms of the last snapshot(): (count pass and scans, write pass, copy to the host)."""
        out = (C.c_double * 3)()
        self._check(self._L.zk_lh_snapshot_ms(self._h, out))
        return float(out[0]), float(out[1]), float(out[2])

    def merge(self, blob) -> None:
        """Add a snapshot into the table (zk_lh_merge). Refused, with the table unchanged: a malformed
        blob or another sub_bits (ZK_ERR_INVALID_ARG), a service id >= num_services
        (ZK_ERR_SERVICE_RANGE), more than 2^32 - 1 records and merged links since reset
        (ZK_ERR_CAPACITY)."""
        raw = bytes(blob.blob if isinstance(blob, LinkHistogramSnapshot) else blob)
        self._check(self._L.zk_lh_merge(self._h, raw, len(raw)))


_SNAP_ROW = np.dtype([("parent", "<u4"), ("child", "<u4"), ("first", "<u8")])


def _two_phase(call) -> bytes:
    """A two-phase blob output (size, then bytes) of a host snapshot function."""
    n = C.c_uint64()
    st = call(None, 0, C.byref(n))
    if st == _abi.ZK_OK:
        buf = (C.c_uint8 * max(1, n.value))()
        st = call(buf, n.value, C.byref(n))
    if st != _abi.ZK_OK:
        raise _abi.ZkError(st, _abi.status_str(st))
    return bytes(buf)[: n.value]


class LinkHistogramSnapshot:
    """A link-histogram snapshot on the host (include/zksketch.h, zk_lh_snapshot_*): validated on
    construction (ZK_ERR_INVALID_ARG for a malformed blob) and parsed into numpy views -- the header
    fields, `rows` (parent, child, first) and `entries` ((bin << 32) | count). plus, remap and quantiles
    go through the library's host-only calls: no device is needed."""

    def __init__(self, blob):
        self.blob = bytes(blob)
        L = _abi.lib()
        st = L.zk_lh_snapshot_validate(self.blob, len(self.blob))
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, "malformed link-histogram snapshot")
        head = np.frombuffer(self.blob, "<u4", 4, 0)
        self.m, self.bins = int(head[2]), int(head[3])
        n = np.frombuffer(self.blob, "<u8", 4, 16)
        self.links, self.dropped = int(n[2]), int(n[3])
        self.rows = np.frombuffer(self.blob, _SNAP_ROW, int(n[0]), 64)
        self.entries = np.frombuffer(self.blob, "<u8", int(n[1]), 64 + 16 * int(n[0]))

    def __len__(self) -> int:
        return len(self.rows)

    def __eq__(self, other):
        return isinstance(other, LinkHistogramSnapshot) and self.blob == other.blob

    def __hash__(self):
        return hash(self.blob)

    def plus(self, other: "LinkHistogramSnapshot") -> "LinkHistogramSnapshot":
        """The snapshot of the summed state (ZK_ERR_CAPACITY when a counter would pass 2^32 - 1)."""
        a, b = self.blob, other.blob
        L = _abi.lib()
        return LinkHistogramSnapshot(_two_phase(lambda o, c, n: L.zk_lh_snapshot_plus(a, len(a), b, len(b), o, c, n)))

    def remap(self, ids) -> "LinkHistogramSnapshot":
        """Every service id i replaced by ids[i], the rows re-sorted."""
        a = self.blob
        m = np.ascontiguousarray(ids, dtype=np.uint32)
        L = _abi.lib()
        return LinkHistogramSnapshot(_two_phase(
            lambda o, c, n: L.zk_lh_snapshot_remap(a, len(a), m.ctypes.data, len(m), o, c, n)))

    def quantiles(self, qs=(0.5, 0.99)):
        """(lo int64[rows, nq], hi int64[rows, nq], count uint64[rows]) in row order: the bin bounds
        holding each row's nearest-rank quantiles (as LinkHistogram.quantiles_all for the present cells)."""
        q = np.ascontiguousarray(qs, dtype=np.float64)
        lo = np.zeros((len(self.rows), len(q)), np.int64)
        hi = np.zeros((len(self.rows), len(q)), np.int64)
        cnt = np.zeros(len(self.rows), np.uint64)
        st = _abi.lib().zk_lh_snapshot_quantiles(self.blob, len(self.blob), q.ctypes.data, len(q), lo.ctypes.data,
                                                 hi.ctypes.data, cnt.ctypes.data_as(_abi._U64P))
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, _abi.status_str(st))
        return lo, hi, cnt
