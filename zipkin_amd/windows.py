"""Dependencies per time window (include/zkwindow.h): the device trace-time partition and the job
that turns its slices into one Dependencies record per window.

ZipkinAggregateJob turns its whole input into Dependencies(0, now, links). WindowedAggregateJob
gives every trace a time (the smallest first_ts of its timed fragments), partitions each batch by
window on the device (WindowPartition: a stable partition, so every window's slice is again a
trace-clustered batch of whole traces, and it never leaves HBM) and runs the unchanged dependency
path once per window.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _abi
from .columns import COLUMNS, DeviceColumns, SpanColumns


class WindowPartition:
    """A zk_win handle: windows [origin_us + w * window_us, origin_us + (w + 1) * window_us), w < num_windows."""

    def __init__(self, *, window_us: int, origin_us: int = 0, num_windows: int = 1, device: int = 0,
                 stream: int | None = None, timing: bool = False):
        self._L = _abi.lib()
        cfg = _abi.zk_win_config()
        cfg.timing = 1 if timing else 0
        cfg.device = device
        cfg.num_windows = num_windows
        cfg.stream = stream
        cfg.origin_us = origin_us
        cfg.window_us = window_us
        h = C.c_void_p()
        st = self._L.zk_win_create(C.byref(cfg), C.byref(h))
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, _abi.status_str(st))
        self._h = h
        self.device = device
        self.origin_us, self.window_us, self.num_windows = int(origin_us), int(window_us), int(num_windows)

    def _check(self, st: int) -> None:
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_win_last_error(self._h).decode() or _abi.status_str(st))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.zk_win_destroy(self._h)
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

    def set_windows(self, origin_us: int, window_us: int, num_windows: int) -> None:
        """Re-aim the handle (zk_win_set_windows)."""
        self._check(self._L.zk_win_set_windows(self._h, origin_us, window_us, num_windows))
        self.origin_us, self.window_us, self.num_windows = int(origin_us), int(window_us), int(num_windows)

    def index(self, t: int) -> int:
        """The window of trace time t by the handle's rule, num_windows for before / after (zk_win_index)."""
        return window_index(t, self.origin_us, self.window_us, self.num_windows)

    def plan(self, n: int) -> tuple[int, int, int]:
        """(records per LDS chunk, records per workgroup range, ranges) for n records (zk_win_plan)."""
        return plan(n)

    PHASES = ("time", "resolve", "hist", "scan", "scatter", "final")

    def phase_ms(self) -> dict:
        """Device time (ms) of each pass of the last partition (zk_win_phase_ms; a handle made with timing=True)."""
        out = (C.c_double * len(self.PHASES))()
        self._check(self._L.zk_win_phase_ms(self._h, out))
        return dict(zip(self.PHASES, out))

    OBSERVE_PHASES = ("runs", "grow", "insert")

    def observe(self, cols, *, sync: bool = True) -> None:
        """Fold a batch (host SpanColumns or DeviceColumns, any order) into the handle's trace-time
        table (zk_win_observe): traceId -> the smallest first_ts over its timed fragments, over every
        batch observed since reset_table(). Observing a batch again changes nothing. sync=False
        leaves the inserts queued on the handle's stream: device columns must then stay as they are
        until the next call that synchronises (table_info, trace_times, partition, observe)."""
        import torch

        flags = 0
        ab = cols.abi()
        if isinstance(cols, DeviceColumns):
            flags |= _abi.ZK_BATCH_DEVICE_PTRS
            torch.cuda.current_stream(self.device).synchronize()  # (torch may still be writing the batch)
        self._check(self._L.zk_win_observe(self._h, C.byref(ab), flags))
        if sync:
            self.table_info()

    def observe_ms(self) -> dict:
        """Device time (ms) of the passes of the last observe (zk_win_observe_ms; timing=True)."""
        out = (C.c_double * len(self.OBSERVE_PHASES))()
        self._check(self._L.zk_win_observe_ms(self._h, out))
        return dict(zip(self.OBSERVE_PHASES, out))

    def reset_table(self) -> None:
        """Empty the trace-time table; its allocation is kept (zk_win_table_reset)."""
        self._check(self._L.zk_win_table_reset(self._h))

    def reserve(self, traces: int) -> None:
        """Grow the table to at least 2 * traces slots now (zk_win_table_reserve); never shrinks."""
        self._check(self._L.zk_win_table_reserve(self._h, traces))

    def table_info(self) -> dict:
        """{"slots", "traces", "bytes"} of the trace-time table (zk_win_table_info); synchronises."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._L.zk_win_table_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"slots": int(a.value), "traces": int(b.value), "bytes": int(c.value)}

    def trace_times(self, ids):
        """(times int64, found bool) of the table for an array of traceIds (zk_win_table_lookup);
        times[i] means nothing where found[i] is False."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
        t = np.zeros(len(ids), np.int64)
        f = np.zeros(len(ids), np.uint8)
        self._check(self._L.zk_win_table_lookup(self._h, ids.ctypes.data_as(C.POINTER(C.c_uint64)), len(ids), 0,
                                                t.ctypes.data_as(C.POINTER(C.c_int64)),
                                                f.ctypes.data_as(C.POINTER(C.c_uint8))))
        return t, f.astype(bool)

    def partition(self, cols, *, hold_last: bool = False, out: Optional[DeviceColumns] = None, clustered: bool = True,
                  table: bool = False):
        """Partition one batch (host SpanColumns or DeviceColumns) by window: a trace-clustered batch
        of whole traces, or with table=True (every batch observed before) any batch, clustered or not.

        Returns (out, offsets, counts): `out` the records in window order then the rest (DeviceColumns
        of the batch's size, allocated unless given; out.n = the records written), `offsets` a uint64
        array of num_windows + 2 entries (window w is out[offsets[w]:offsets[w + 1]], the rest
        out[offsets[W]:offsets[W + 1]]), `counts` the zk_win_counts as a dict. hold_last leaves the
        batch's last run out (counts["held_from"] is its first record). With table=True the counts also
        hold "unobserved_records". The call is synchronous."""
        import torch

        flags = _abi.ZK_BATCH_TRACE_CLUSTERED if clustered else 0
        if hold_last:
            flags |= _abi.ZK_WIN_HOLD_LAST
        if table:
            flags |= _abi.ZK_WIN_TRACE_TABLE
        if isinstance(cols, DeviceColumns):
            ab = cols.abi()
            flags |= _abi.ZK_BATCH_DEVICE_PTRS
        else:
            ab = cols.abi()
        n = int(ab.n)
        if out is None:
            out = DeviceColumns(n, device=f"cuda:{self.device}")
        elif out.capacity < n:
            raise ValueError("out is smaller than the batch")
        # torch's stream may still be writing the batch or using the memory `out` was given
        torch.cuda.current_stream(self.device).synchronize()
        ob = out.abi(n)
        offsets = np.zeros(self.num_windows + 2, np.uint64)
        cnt = _abi.zk_win_counts()
        self._check(self._L.zk_win_partition(self._h, C.byref(ab), flags, C.byref(ob),
                                             offsets.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(cnt)))
        out.n = int(offsets[-1])
        return out, offsets, cnt.as_dict(table)


def window_slice(out: DeviceColumns, a: int, b: int) -> DeviceColumns:
    """Records [a, b) of a partitioned batch as columns DepsContext.accumulate takes.

    The join reads two records per lane, so zk_deps_accumulate wants device columns that start on a
    16-byte (u64 columns) / 8-byte (u32 columns) boundary: an even record of an aligned buffer. A part
    whose first record is even is returned as a view; one that starts on an odd record is copied,
    device to device, into fresh columns (the copy has completed when this returns)."""
    import torch

    v = out.slice(a, b)
    if all(getattr(v, k).data_ptr() % (2 * np.dtype(dt).itemsize) == 0 for k, dt in COLUMNS):
        return v
    c = DeviceColumns(b - a, device=str(out.trace_id.device))
    for k, _ in COLUMNS:
        getattr(c, k).copy_(getattr(v, k))
    torch.cuda.current_stream(out.trace_id.device).synchronize()
    return c


def _concat_slices(slices) -> DeviceColumns:
    """The records of [(partitioned batch, a, b)] back to back in fresh device columns (one slice that
    window_slice would take in place is used in place)."""
    import torch

    if len(slices) == 1:
        return window_slice(*slices[0])
    dev = slices[0][0].trace_id.device
    c = DeviceColumns(sum(b - a for _, a, b in slices), device=str(dev))
    at = 0
    for p, a, b in slices:
        for k, _ in COLUMNS:
            getattr(c, k)[at:at + b - a].copy_(getattr(p, k)[a:b])
        at += b - a
    torch.cuda.current_stream(dev).synchronize()
    return c


def window_index(t: int, origin_us: int, window_us: int, num_windows: int) -> int:
    """zk_win_index: the window rule on the host (no device)."""
    w = C.c_uint32()
    st = _abi.lib().zk_win_index(t, origin_us, window_us, num_windows, C.byref(w))
    if st != _abi.ZK_OK:
        raise _abi.ZkError(st, _abi.status_str(st))
    return int(w.value)


def plan(n: int) -> tuple[int, int, int]:
    """zk_win_plan without a handle: the geometry depends on n alone."""
    c, r, k = C.c_uint64(), C.c_uint64(), C.c_uint64()
    st = _abi.lib().zk_win_plan(None, n, C.byref(c), C.byref(r), C.byref(k))
    if st != _abi.ZK_OK:
        raise _abi.ZkError(st, _abi.status_str(st))
    return int(c.value), int(r.value), int(k.value)


def _timed_min_max(cols):
    """(min, max) of first_ts over the timed fragments of a batch, or None when it has none."""
    if isinstance(cols, DeviceColumns):
        import torch

        n = cols.n
        timed = (cols.flags[:n] & _abi.ZK_F_HAS_ANNOTATIONS) != 0
        if not bool(timed.any()):
            return None
        ts = cols.first_ts[:n]
        big, small = torch.iinfo(torch.int64).max, torch.iinfo(torch.int64).min
        return int(torch.where(timed, ts, big).min()), int(torch.where(timed, ts, small).max())
    timed = (cols.flags & np.uint32(_abi.ZK_F_HAS_ANNOTATIONS)) != 0
    if not timed.any():
        return None
    ts = cols.first_ts[timed]
    return int(ts.min()), int(ts.max())


class WindowedAggregateJob:
    """ZipkinAggregateJob per time window: one Dependencies record per window instead of one for all.

    run(batches) takes host SpanColumns or DeviceColumns batches. A trace belongs to the window of its
    trace time, the smallest first_ts of its fragments that carry annotations. `order` says what the
    batches promise:
      "whole"  (default) each batch is trace-clustered and holds whole traces. The trace time comes from
               the batch itself; a trace that recurs in a later batch is ZK_ERR_NOT_CLUSTERED (verify).
      "rows"   each batch is trace-clustered, but the input is cut into batches anywhere, also inside a
               trace (what a streaming reader of row-per-trace storage feeds).
      "any"    records in any order; a trace's fragments may lie in several batches.
    "rows" and "any" take the trace time from the partition's trace-time table: run() resets it,
    observes every batch, then partitions every batch with table=True (a ValueError if a batch's
    records were not all observed). For "rows" a window's slices are accumulated in batch order with
    clustered=True, continues=True: a cut trace ends one slice and begins the next, and the dependency
    path joins it. For "any" a window's slices of all batches are concatenated in HBM and accumulated
    once with clustered=False (the group join; nothing merges unclustered batches across accumulate
    calls) and without verification, which needs trace runs.

    origin_us=None: the job reads the smallest and largest timed first_ts of the batches, sets origin =
    floor(min / window_us) * window_us and the number of windows from the largest; with origin_us given
    only the number of windows comes from the data (traces before it go to the rest). More than
    max_windows windows raises ValueError.

    Every batch is partitioned on the device (the partitioned copies stay in HBM, 48 B per record);
    then, for each window with records, the context (and the link histogram) is reset, that window's
    slice of every batch is accumulated with clustered=True (window_slice: in place, or through an
    aligned copy when it starts on an odd record) and the table finalized. run() returns the
    list of Dependencies(origin + w * window_us, origin + (w + 1) * window_us, links), ascending; a
    window without links is omitted (the reference writes nothing for it). stats[w] holds each window's
    counters; rest the runs and records before the origin, after the last window and without a time
    (these are not accumulated). With an `aggregates` sink each record is stored through
    storeDependencies; with link_quantiles it is stored with that window's link-histogram snapshot
    (link_histograms[w]), so getLinkDurations(start, end) answers per window. verify=True checks on the
    device that no trace recurs inside a window, within a batch or across batches
    (ZK_ERR_NOT_CLUSTERED). One context and one histogram handle serve all windows."""

    def __init__(self, services, *, window_us: int, origin_us: Optional[int] = None, max_windows: int = 1024,
                 device: int = 0, strict: bool = True, aggregates=None, verify: bool = True,
                 link_quantiles: Optional[Sequence[float]] = None, order: str = "whole"):
        if order not in ("whole", "rows", "any"):
            raise ValueError('order is "whole", "rows" or "any"')
        self.order = order
        if window_us <= 0:
            raise ValueError("window_us must be positive")
        if not 1 <= max_windows <= _abi.ZK_WIN_MAX_WINDOWS:
            raise ValueError(f"max_windows is 1..{_abi.ZK_WIN_MAX_WINDOWS}")
        self.services = services
        self.window_us = int(window_us)
        self.origin_us = None if origin_us is None else int(origin_us)
        self.max_windows = int(max_windows)
        self.device = device
        self.strict = strict
        self.aggregates = aggregates
        self.verify = verify
        self.link_quantiles = None if link_quantiles is None else tuple(float(q) for q in link_quantiles)
        self.stats: dict = {}
        self.rest: dict = {}
        self.link_histograms: dict = {}
        self.origin: Optional[int] = None
        self.num_windows = 0
        self._ctx = self._lh = self._win = None

    def close(self) -> None:
        for k in ("_lh", "_ctx", "_win"):
            o = getattr(self, k)
            if o is not None:
                o.close()
                setattr(self, k, None)

    def _choose_windows(self, batches) -> None:
        lo = hi = None
        for b in batches:
            mm = _timed_min_max(b)
            if mm is not None:
                lo = mm[0] if lo is None else min(lo, mm[0])
                hi = mm[1] if hi is None else max(hi, mm[1])
        if self.origin_us is not None:
            origin = self.origin_us
        else:
            origin = 0 if lo is None else lo // self.window_us * self.window_us  # (Python's floor division)
        if origin < -(2 ** 63):
            raise ValueError("the first window starts before the smallest int64 time")
        W = 1 if hi is None or hi < origin else (hi - origin) // self.window_us + 1
        if W > self.max_windows:
            raise ValueError(f"{W} windows of {self.window_us} us from {origin} > max_windows {self.max_windows}")
        self.origin, self.num_windows = origin, W

    def run(self, batches, num_services: Optional[int] = None) -> List["Dependencies"]:
        from .aggregates import Dependencies, _store, links_from_table
        from .context import DepsContext

        if isinstance(batches, SpanColumns) or hasattr(batches, "abi"):
            batches = [batches]
        batches = list(batches)
        S = num_services or max(1, len(self.services))
        self._choose_windows(batches)
        origin, W, win_us = self.origin, self.num_windows, self.window_us
        if self._win is None:
            self._win = WindowPartition(window_us=win_us, origin_us=origin, num_windows=W, device=self.device)
        else:
            self._win.set_windows(origin, win_us, W)
        if self._ctx is None or self._ctx.num_services != S:
            for k in ("_lh", "_ctx"):
                if getattr(self, k) is not None:
                    getattr(self, k).close()
                    setattr(self, k, None)
            self._ctx = DepsContext(S, device=self.device, strict=self.strict)
            if self.link_quantiles is not None:
                from .realtime import LinkHistogram

                self._lh = LinkHistogram(S, device=self.device)
                self._lh.bind(self._ctx)
        if self.order == "whole":
            parts = [self._win.partition(b) for b in batches]
        else:
            self._win.reset_table()
            for b in batches:
                self._win.observe(b)
            parts = [self._win.partition(b, table=True, clustered=self.order == "rows") for b in batches]
            missed = sum(c["unobserved_records"] for _, _, c in parts)
            if missed:
                raise ValueError(f"{missed} timed records of traces the trace-time table does not hold")
        self.rest = {k: sum(c[k] for _, _, c in parts) for k in
                     ("before_runs", "before_records", "after_runs", "after_records", "untimed_runs", "untimed_records")}
        self.stats, self.link_histograms = {}, {}
        ctx, out = self._ctx, []
        for w in range(W):
            slices = [(p, int(off[w]), int(off[w + 1])) for p, off, _ in parts if off[w + 1] > off[w]]
            if not slices:
                continue
            ctx.reset()
            if self._lh is not None:
                self._lh.reset()
            if self.order == "whole":
                for p, a, b in slices:
                    ctx.accumulate(window_slice(p, a, b), clustered=True, verify=self.verify)
            elif self.order == "rows":
                for p, a, b in slices:
                    ctx.accumulate(window_slice(p, a, b), clustered=True, continues=True, verify=self.verify)
            else:
                ctx.accumulate(_concat_slices(slices), clustered=False, verify=False)
            table = ctx.finalize()
            self.stats[w] = ctx.stats()
            links = links_from_table(table, self.services)
            if not links:
                continue
            deps = Dependencies(origin + w * win_us, origin + (w + 1) * win_us, links)
            hist = None
            if self._lh is not None:
                hist = self.link_histograms[w] = self._lh.snapshot()
            if self.aggregates is not None:
                _store(self.aggregates, deps, hist)
            out.append(deps)
        return out
