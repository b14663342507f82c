"""The trace-id index by service and span name (include/zkindex.h): getTraceIdsByName, getSpanNames and
getAllServiceNames from segments in HBM.

TraceNameIndex keeps one entry (service, span-name id, last timestamp, traceId) per indexed span
fragment, grouped by service, and answers the call every query of the reference's query service begins
with: the newest `limit` trace ids of a service, optionally of one span name, at or before end_ts
(SpanStore.getTraceIdsByName; QueryService.getTraceIdsByServiceName / getTraceIdsBySpanName). With a
TraceDurationIndex over the same batches, "the 100 slowest recent traces of service X, rpc Y" runs on
the device from stored bytes.
"""
from __future__ import annotations

import ctypes as C
import heapq
from typing import Iterable, List, NamedTuple, Optional, Sequence, Union

import numpy as np

from . import _abi
from .columns import DeviceColumns

INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1


class IndexedTraceId(NamedTuple):
    """The reference's IndexedTraceId(traceId, timestamp)."""
    trace_id: int
    timestamp: int


def _index_key(t) -> tuple:
    """The index's order: timestamp descending, then traceId ascending (unsigned)."""
    return (-t[1], t[0])


def merge_trace_ids(lists: Iterable[Sequence[IndexedTraceId]], limit: int) -> List[IndexedTraceId]:
    """The first `limit`, in the index's order, of the union of per-shard (or per-id) getTraceIdsByName
    results; duplicates are kept. TraceId-hash shards hold disjoint traces, so the `limit` best of the
    union are among each shard's `limit` best (the argument of durations.merge_top)."""
    return heapq.nsmallest(max(0, int(limit)), (IndexedTraceId(*t) for l in lists for t in l), key=_index_key)


def _fold_ids(names: Optional[Sequence[str]], wanted: str, base: int) -> List[int]:
    """The ids (index + base) of the dictionary's entries that equal `wanted` case-insensitively: the
    reference lowercases names, the decoders' dictionaries do not, so several ids may match."""
    if names is None:
        raise ValueError("a name as a string needs the dictionary (services= / span_names=)")
    w = wanted.lower()
    return [i + base for i, n in enumerate(names) if n.lower() == w]


class TraceNameIndex:
    """A zk_ix handle. `with TraceNameIndex(S) as idx:` frees it on exit.

    client_service: the id of the service literally called "client", whose client-side spans the
    reference does not index (shouldIndex); None switches the rule off. services / span_names: the
    decoders' dictionaries (index i of services is service id i, index i of span_names is name id
    i + 1); with them `service` and `span_name` may be strings, matched case-insensitively."""

    OBSERVE_PHASES = ("count", "size", "scatter")
    EXPIRE_PHASES = ("count", "size", "rewrite")

    def __init__(self, num_services: int, device: int = 0, client_service: Optional[int] = None, timing: bool = False,
                 stream: Optional[int] = None, services: Optional[Sequence[str]] = None,
                 span_names: Optional[Sequence[str]] = None):
        self._L = _abi.lib()
        cfg = _abi.zk_ix_config()
        cfg.device = device
        cfg.num_services = num_services
        cfg.client_service = _abi.ZK_IX_NO_CLIENT if client_service is None else int(client_service)
        cfg.timing = 1 if timing else 0
        cfg.stream = stream
        h = C.c_void_p()
        st = self._L.zk_ix_create(C.byref(cfg), C.byref(h))
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, _abi.status_str(st))
        self._h = h
        self.device = device
        self.num_services = int(num_services)
        self.services = None if services is None else list(services)
        self.span_names = None if span_names is None else list(span_names)
        self.matched = 0  # matching entries of the last getTraceIdsByName

    def _check(self, st: int) -> None:
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_ix_last_error(self._h).decode() or _abi.status_str(st))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.zk_ix_destroy(self._h)
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

    # ---- writing ---------------------------------------------------------------------------------------
    def observe(self, cols, *, sync: bool = True) -> None:
        """Add a batch's entries (host SpanColumns or DeviceColumns, any order) as one segment
        (zk_ix_observe). Observing a batch again adds its entries again. sync=False leaves the scatter
        queued on the handle's stream: device columns must then stay as they are until the next call
        that synchronises (info, getTraceIdsByName, getSpanNames, compact, expire, observe)."""
        flags = 0
        ab = cols.abi()
        if isinstance(cols, DeviceColumns):
            import torch

            flags |= _abi.ZK_BATCH_DEVICE_PTRS
            torch.cuda.current_stream(self.device).synchronize()  # (torch may still be writing the batch)
        self._check(self._L.zk_ix_observe(self._h, C.byref(ab), flags))
        if sync:
            self.info()

    def reset(self) -> None:
        """Empty the index (zk_ix_reset)."""
        self._check(self._L.zk_ix_reset(self._h))

    def compact(self) -> None:
        """Merge all segments into one (zk_ix_compact)."""
        self._check(self._L.zk_ix_compact(self._h))

    def expire(self, min_ts: int) -> int:
        """Remove every entry with ts < min_ts, by the entry's own timestamp (zk_ix_expire); an entry at
        min_ts stays. Returns the number removed. Afterwards the index answers as a fresh one that
        observed only the survivors; segments that lose nothing are kept as they are, the survivors of
        the others go into one new segment. Synchronises."""
        n = C.c_uint64()
        self._check(self._L.zk_ix_expire(self._h, int(min_ts), C.byref(n)))
        return int(n.value)

    def info(self) -> dict:
        """{"entries", "segments", "bytes"} (zk_ix_info); synchronises."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._L.zk_ix_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"entries": int(a.value), "segments": int(b.value), "bytes": int(c.value)}

    def service_counts(self) -> np.ndarray:
        """Entries per service id, uint64[num_services] (zk_ix_service_counts: host bookkeeping)."""
        out = np.zeros(self.num_services, np.uint64)
        self._check(self._L.zk_ix_service_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    # ---- names -----------------------------------------------------------------------------------------
    def _service_ids(self, service: Union[int, str]) -> List[int]:
        if isinstance(service, str):
            return [i for i in _fold_ids(self.services, service, 0) if i < self.num_services]
        return [int(service)]

    def _name_ids(self, span_name: Union[None, int, str]) -> List[int]:
        if span_name is None:
            return [_abi.ZK_IX_ANY_NAME]
        if isinstance(span_name, str):
            return [i for i in _fold_ids(self.span_names, span_name, 1) if i <= _abi.ZK_F_NAME_MASK]
        return [int(span_name)]

    # ---- reading ---------------------------------------------------------------------------------------
    def trace_ids(self, service: int, name: int, end_ts: int, limit: int):
        """zk_ix_trace_ids for one service id and one name id (or ZK_IX_ANY_NAME):
        (rows [IndexedTraceId], matched)."""
        cap = max(1, min(int(limit), _abi.ZK_IX_MAX_LIMIT))
        ids = np.zeros(cap, np.uint64)
        ts = np.zeros(cap, np.int64)
        n, m = C.c_uint32(), C.c_uint64()
        self._check(self._L.zk_ix_trace_ids(self._h, service, name, end_ts, limit, ids.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            ts.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(n), C.byref(m)))
        c = int(n.value)
        return [IndexedTraceId(i, t) for i, t in zip(ids[:c].tolist(), ts[:c].tolist())], int(m.value)

    def getTraceIdsByName(self, service: Union[int, str], span_name: Union[None, int, str], end_ts: int,
                          limit: int) -> List[IndexedTraceId]:
        """SpanStore.getTraceIdsByName: the newest `limit` (traceId, timestamp) of `service`, of
        `span_name` when it is not None, with timestamp <= end_ts; timestamp descending, equal
        timestamps by traceId ascending. `matched` holds the number of matching entries after the call.
        A string that no dictionary entry matches yields []; one that several ids match is asked per id
        and the answers are merged (merge_trace_ids)."""
        self.matched = 0
        lists = []
        for s in self._service_ids(service):
            for nm in self._name_ids(span_name):
                rows, m = self.trace_ids(s, nm, int(end_ts), int(limit))
                lists.append(rows)
                self.matched += m
        if len(lists) == 1:
            return lists[0]
        return merge_trace_ids(lists, limit)

    def span_name_ids(self, service: int) -> List[int]:
        """zk_ix_span_names: the distinct non-zero name ids of one service id, ascending."""
        cap = _abi.ZK_F_NAME_MASK
        out = np.zeros(cap, np.uint16)
        n = C.c_uint32()
        self._check(self._L.zk_ix_span_names(self._h, service, out.ctypes.data_as(C.POINTER(C.c_uint16)), cap, C.byref(n)))
        return out[:int(n.value)].tolist()

    def getSpanNames(self, service: Union[int, str]) -> set:
        """SpanStore.getSpanNames: the span names of the service's entries: lowercased strings with a
        span_names dictionary, else name ids. An unknown service string yields set()."""
        ids = set()
        for s in self._service_ids(service):
            ids.update(self.span_name_ids(s))
        if self.span_names is None:
            return ids
        if ids and max(ids) > len(self.span_names):
            raise ValueError("a name id beyond the span_names dictionary")
        return {self.span_names[i - 1].lower() for i in ids}

    def getAllServiceNames(self) -> set:
        """SpanStore.getAllServiceNames: the services that have entries: lowercased strings with a
        services dictionary, else service ids."""
        ids = np.flatnonzero(self.service_counts()).tolist()
        if self.services is None:
            return set(ids)
        if ids and max(ids) >= len(self.services):
            raise ValueError("a service id beyond the services dictionary")
        return {self.services[i].lower() for i in ids}

    # ---- the query service -----------------------------------------------------------------------------
    def getTraceIdsBySpanName(self, service, span_name, end_ts: int, limit: int, order: Optional[str], durations) -> List[int]:
        """QueryService.getTraceIdsBySpanName (:209-234): the index's ids through
        durations.sortTraceIds(ids, limit, order) (a durations.TraceDurationIndex over the same
        batches); order=None returns them as indexed. An empty span name asks the service alone."""
        if service is None or service == "":
            raise ValueError("No service name provided")
        if span_name == "":
            span_name = None
        ids = [t.trace_id for t in self.getTraceIdsByName(service, span_name, end_ts, limit)]
        return durations.sortTraceIds(ids, limit, order) if order is not None else ids

    def getTraceIdsByServiceName(self, service, end_ts: int, limit: int, order: Optional[str], durations) -> List[int]:
        """QueryService.getTraceIdsByServiceName (:236-256)."""
        return self.getTraceIdsBySpanName(service, None, end_ts, limit, order, durations)

    # ---- timing ----------------------------------------------------------------------------------------
    def observe_ms(self) -> dict:
        """Device time (ms) of the passes of the last observe (zk_ix_observe_ms; timing=True)."""
        out = (C.c_double * len(self.OBSERVE_PHASES))()
        self._check(self._L.zk_ix_observe_ms(self._h, out))
        return dict(zip(self.OBSERVE_PHASES, out))

    def expire_ms(self) -> dict:
        """Device time (ms) of the passes of the last expire (zk_ix_expire_ms; timing=True)."""
        out = (C.c_double * len(self.EXPIRE_PHASES))()
        self._check(self._L.zk_ix_expire_ms(self._h, out))
        return dict(zip(self.EXPIRE_PHASES, out))

    def query_ms(self) -> float:
        """Time (ms) on the handle's stream of the last getTraceIdsByName pass (zk_ix_query_ms)."""
        ms = C.c_double()
        self._check(self._L.zk_ix_query_ms(self._h, C.byref(ms)))
        return float(ms.value)
