"""The trace duration index (include/zkduration.h): getTracesDuration and the k slowest, fastest,
newest or oldest traces of a time range, from one table in HBM.

TraceDurationIndex folds batches of span fragments into traceId -> (start, end): start the smallest
first_ts and end the largest last_ts over the trace's fragments that carry annotations. It stands
behind the reference's SpanStore.getTracesDuration and QueryService.sortTraceIds; top() is the
selection a duration index answers without reading every row.
"""
from __future__ import annotations

import ctypes as C
import heapq
from typing import Iterable, List, NamedTuple, Optional, Sequence

import numpy as np

from . import _abi
from .columns import DeviceColumns

INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1

# the names of top()'s orders -> the ordinals of the query service's Order enum
ORDERS = {
    "timestamp-desc": _abi.ZK_TD_TIMESTAMP_DESC,
    "timestamp-asc": _abi.ZK_TD_TIMESTAMP_ASC,
    "duration-asc": _abi.ZK_TD_DURATION_ASC,
    "duration-desc": _abi.ZK_TD_DURATION_DESC,
}


class TraceIdDuration(NamedTuple):
    """The reference's TraceIdDuration(traceId, duration, startTimestamp)."""
    trace_id: int
    duration: int
    start_timestamp: int


def _order(order: str) -> int:
    try:
        return ORDERS[order]
    except KeyError:
        raise ValueError(f"order is one of {sorted(ORDERS)}") from None


def _sort_key(order: str):
    """The key under which `sorted` gives top()'s order: the order's field, descending for the DESC
    orders, then the traceId ascending."""
    _order(order)
    field = (lambda t: t.duration) if order.startswith("duration") else (lambda t: t.start_timestamp)
    sign = -1 if order.endswith("desc") else 1
    return lambda t: (sign * field(t), t.trace_id)


def merge_top(lists: Iterable[Sequence[TraceIdDuration]], k: int, order: str) -> List[TraceIdDuration]:
    """The k first, in `order`, of the union of per-shard top() results. TraceId-hash shards hold
    disjoint traces, so the k best of the union are among the shards' k best; ties are broken by
    traceId, as on the device."""
    key = _sort_key(order)
    return heapq.nsmallest(k, (t for l in lists for t in l), key=key)


class TraceDurationIndex:
    """A zk_td handle. `with TraceDurationIndex() as idx:` frees it on exit."""

    def __init__(self, device: int = 0, timing: bool = False, *, stream: int | None = None):
        self._L = _abi.lib()
        cfg = _abi.zk_td_config()
        cfg.device = device
        cfg.timing = 1 if timing else 0
        cfg.stream = stream
        h = C.c_void_p()
        st = self._L.zk_td_create(C.byref(cfg), C.byref(h))
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, _abi.status_str(st))
        self._h = h
        self.device = device
        self.matched = 0  # traces in the range of the last top()

    def _check(self, st: int) -> None:
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_td_last_error(self._h).decode() or _abi.status_str(st))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.zk_td_destroy(self._h)
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

    OBSERVE_PHASES = ("runs", "grow", "insert")
    EXPIRE_PHASES = ("count", "size", "rebuild")

    def observe(self, cols, *, sync: bool = True) -> None:
        """Fold a batch (host SpanColumns or DeviceColumns, any order) into the index (zk_td_observe).
        Observing a batch again changes nothing. sync=False leaves the inserts queued on the handle's
        stream: device columns must then stay as they are until the next call that synchronises
        (info, lookup, getTracesDuration, top, expire, observe)."""
        flags = 0
        ab = cols.abi()
        if isinstance(cols, DeviceColumns):
            import torch

            flags |= _abi.ZK_BATCH_DEVICE_PTRS
            torch.cuda.current_stream(self.device).synchronize()  # (torch may still be writing the batch)
        self._check(self._L.zk_td_observe(self._h, C.byref(ab), flags))
        if sync:
            self.info()

    def reset(self) -> None:
        """Empty the index; its allocation is kept (zk_td_reset)."""
        self._check(self._L.zk_td_reset(self._h))

    def reserve(self, traces: int) -> None:
        """Grow the table to at least 2 * traces slots now (zk_td_reserve); never shrinks."""
        self._check(self._L.zk_td_reserve(self._h, traces))

    def expire(self, min_end: int) -> int:
        """Remove every trace whose end < min_end, by the trace's own end time (zk_td_expire); a trace
        that ends at min_end stays. Returns the number removed. When something goes the survivors are
        rebuilt into a table sized for them (the one operation that may shrink it; a reserve() hint
        does not survive it). Synchronises."""
        n = C.c_uint64()
        self._check(self._L.zk_td_expire(self._h, int(min_end), C.byref(n)))
        return int(n.value)

    def info(self) -> dict:
        """{"slots", "traces", "bytes"} of the table (zk_td_info); synchronises."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._L.zk_td_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"slots": int(a.value), "traces": int(b.value), "bytes": int(c.value)}

    def lookup(self, ids):
        """(start int64, duration int64, found bool) for an array of traceIds, in the order asked
        (zk_td_lookup); start[i] and duration[i] mean nothing where found[i] is False. `ids` is anything
        numpy turns into uint64, or a torch int64 tensor on the handle's device (the ids' bit patterns)."""
        flags = 0
        if hasattr(ids, "data_ptr"):
            import torch

            if ids.dtype != torch.int64 or not ids.is_contiguous() or ids.device.index != self.device:
                raise ValueError("device ids: a contiguous int64 tensor on the handle's device")
            torch.cuda.current_stream(self.device).synchronize()
            n, ptr, flags = int(ids.numel()), ids.data_ptr(), _abi.ZK_BATCH_DEVICE_PTRS
        else:
            ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
            n, ptr = len(ids), ids.ctypes.data
        s = np.zeros(n, np.int64)
        d = np.zeros(n, np.int64)
        f = np.zeros(n, np.uint8)
        self._check(self._L.zk_td_lookup(self._h, ptr, n, flags, s.ctypes.data_as(C.POINTER(C.c_int64)),
                                         d.ctypes.data_as(C.POINTER(C.c_int64)), f.ctypes.data_as(C.POINTER(C.c_uint8))))
        return s, d, f.astype(bool)

    def getTracesDuration(self, ids) -> List[TraceIdDuration]:
        """SpanStore.getTracesDuration: one TraceIdDuration per asked id the index holds, in the order
        asked (an id it does not hold yields nothing; a duplicate is answered as often as asked)."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
        s, d, f = self.lookup(ids)
        return [TraceIdDuration(int(i), int(dd), int(ss)) for i, ss, dd, ff in zip(ids.tolist(), s.tolist(), d.tolist(), f) if ff]

    def top(self, order: str, k: int, start: Optional[int] = None, end: Optional[int] = None) -> List[TraceIdDuration]:
        """The first k traces in `order` ("duration-desc", "duration-asc", "timestamp-desc",
        "timestamp-asc") among those whose start lies in [start, end], both inclusive (None: the end of
        int64); equal keys by traceId ascending (zk_td_top). `matched` holds the number of traces in
        the range after the call."""
        o = _order(order)
        lo = INT64_MIN if start is None else int(start)
        hi = INT64_MAX if end is None else int(end)
        cap = max(1, min(int(k), _abi.ZK_TD_MAX_TOP))
        ids = np.zeros(cap, np.uint64)
        s = np.zeros(cap, np.int64)
        d = np.zeros(cap, np.int64)
        n, m = C.c_uint32(), C.c_uint64()
        self._check(self._L.zk_td_top(self._h, o, lo, hi, k, ids.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      s.ctypes.data_as(C.POINTER(C.c_int64)), d.ctypes.data_as(C.POINTER(C.c_int64)),
                                      C.byref(n), C.byref(m)))
        self.matched = int(m.value)
        c = int(n.value)
        return [TraceIdDuration(i, dd, ss) for i, ss, dd in zip(ids[:c].tolist(), s[:c].tolist(), d[:c].tolist())]

    def sortTraceIds(self, ids, limit: int, order: Optional[str]) -> List[int]:
        """QueryService.sortTraceIds: order=None returns the ids untouched; otherwise the ids the index
        holds, sorted by the reference's comparison (a stable sort: ties keep the asked order, as with
        the in-memory store), cut to `limit`. The sort runs on the host: its n is a query's limit."""
        if order is None:
            return list(ids)
        _order(order)
        found = self.getTracesDuration(ids)
        field = (lambda t: t.duration) if order.startswith("duration") else (lambda t: t.start_timestamp)
        found.sort(key=field, reverse=order.endswith("desc"))  # (reverse keeps the order of equal keys)
        return [t.trace_id for t in found[:limit]]

    def observe_ms(self) -> dict:
        """Device time (ms) of the passes of the last observe (zk_td_observe_ms; timing=True)."""
        out = (C.c_double * len(self.OBSERVE_PHASES))()
        self._check(self._L.zk_td_observe_ms(self._h, out))
        return dict(zip(self.OBSERVE_PHASES, out))

    def expire_ms(self) -> dict:
        """Device time (ms) of the passes of the last expire (zk_td_expire_ms; timing=True)."""
        out = (C.c_double * len(self.EXPIRE_PHASES))()
        self._check(self._L.zk_td_expire_ms(self._h, out))
        return dict(zip(self.EXPIRE_PHASES, out))

    def top_ms(self) -> float:
        """Time (ms) on the handle's stream of the last top (zk_td_top_ms; timing=True)."""
        ms = C.c_double()
        self._check(self._L.zk_td_top_ms(self._h, C.byref(ms)))
        return float(ms.value)
