"""The trace-id index by annotation (include/zkannindex.h): getTraceIdsByAnnotation from segments in
HBM, and the query service's getTraceIds over it and a TraceNameIndex.

TraceAnnotationIndex keeps one entry (service, key hash, value hash, timestamp, traceId) per indexed
time annotation and binary annotation, grouped by service, and answers SpanStore.getTraceIdsByAnnotation:
the newest `limit` trace ids of a service that carry the annotation (and value) at or before end_ts.
The entries come from SpanDecoder.decode_indexed (zk_ingest_spans_indexed) or, for stored bytes already
in HBM, from DeviceSpanDecoder.decode_device(indexed=True) (zk_ingest_dev_spans_indexed):
TraceAnnotationIndex.observe_stored decodes and observes in one step.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _abi
from .nameindex import INT64_MAX, IndexedTraceId, _fold_ids, merge_trace_ids

CORE_ANNOTATIONS = frozenset((b"cs", b"cr", b"sr", b"ss"))  # Constants.CoreAnnotations
TRACE_TIMESTAMP_PADDING_US = 60_000_000                    # Constants.TraceTimestampPadding: 1 minute
_M64 = (1 << 64) - 1

_COLUMNS = (("service", np.uint32), ("key", np.uint64), ("val", np.uint64), ("ts", np.int64), ("trace_id", np.uint64))


def _bytes(s: Union[str, bytes]) -> bytes:
    return s.encode() if isinstance(s, str) else bytes(s)


def key_hash(annotation: Union[str, bytes]) -> int:
    """An entry's key: zk_hash_string of a time annotation's value or a binary annotation's key."""
    b = _bytes(annotation)
    return int(_abi.lib().zk_hash_string(b, len(b)))


def value_hash(value: Union[str, bytes]) -> int:
    """A binary entry's val: zk_index_value_hash = zk_hash_string | 1 (never 0)."""
    b = _bytes(value)
    return int(_abi.lib().zk_index_value_hash(b, len(b)))


class AnnotationItems:
    """The annotation index's entries as five host columns: service uint32, key uint64, val uint64,
    ts int64, trace_id uint64 (zk_ingest_index_items)."""

    def __init__(self, service, key, val, ts, trace_id):
        given = (service, key, val, ts, trace_id)
        for (name, dt), a in zip(_COLUMNS, given):
            setattr(self, name, np.ascontiguousarray(a, dtype=dt))
        if len({len(getattr(self, name)) for name, _ in _COLUMNS}) != 1:
            raise ValueError("the five columns differ in length")

    @classmethod
    def empty(cls, n: int) -> "AnnotationItems":
        return cls(*[np.zeros(n, dt) for _, dt in _COLUMNS])

    @classmethod
    def concat(cls, parts: Sequence["AnnotationItems"]) -> "AnnotationItems":
        return cls(*[np.concatenate([getattr(p, name) for p in parts]) if parts else np.zeros(0, dt) for name, dt in _COLUMNS])

    def __len__(self) -> int:
        return len(self.service)

    def take(self, sel) -> "AnnotationItems":
        return AnnotationItems(*[getattr(self, name)[sel] for name, _ in _COLUMNS])

    def rows(self) -> List[tuple]:
        """[(service, key, val, ts, trace_id)] as Python ints."""
        return list(zip(*[getattr(self, name).tolist() for name, _ in _COLUMNS]))

    def abi(self, cap: Optional[int] = None, n: Optional[int] = None) -> _abi.zk_ingest_index_items:
        return _abi.zk_ingest_index_items(*[getattr(self, name).ctypes.data for name, _ in _COLUMNS],
                                          len(self) if cap is None else cap, len(self) if n is None else n)


class DeviceAnnotationItems:
    """The same five columns as torch tensors on the device (service int32, the rest int64: the bit
    patterns of the unsigned columns)."""

    def __init__(self, service, key, val, ts, trace_id):
        self.service, self.key, self.val, self.ts, self.trace_id = service, key, val, ts, trace_id
        self.device = service.device.index or 0

    @classmethod
    def from_host(cls, items: AnnotationItems, device: int = 0) -> "DeviceAnnotationItems":
        import torch

        dev = f"cuda:{device}"
        cols = [torch.from_numpy(items.service.view(np.int32).copy()).to(dev)]
        cols += [torch.from_numpy(getattr(items, name).view(np.int64).copy()).to(dev) for name in ("key", "val", "ts", "trace_id")]
        return cls(*cols)

    def __len__(self) -> int:
        return int(self.service.numel())

    def abi(self) -> _abi.zk_ingest_index_items:
        n = len(self)
        return _abi.zk_ingest_index_items(self.service.data_ptr(), self.key.data_ptr(), self.val.data_ptr(), self.ts.data_ptr(),
                                          self.trace_id.data_ptr(), n, n)


class TraceAnnotationIndex:
    """A zk_ax handle. `with TraceAnnotationIndex(S) as idx:` frees it on exit.

    services: the decoder's service dictionary (index i is service id i); with it `service` may be a
    string, matched case-insensitively. Annotation and value bytes are matched exactly."""

    OBSERVE_PHASES = ("count", "size", "scatter")
    EXPIRE_PHASES = ("count", "size", "rewrite")

    def __init__(self, num_services: int, device: int = 0, timing: bool = False, stream: Optional[int] = None,
                 services: Optional[Sequence[str]] = None):
        self._L = _abi.lib()
        cfg = _abi.zk_ax_config()
        cfg.device = device
        cfg.num_services = num_services
        cfg.timing = 1 if timing else 0
        cfg.stream = stream
        h = C.c_void_p()
        st = self._L.zk_ax_create(C.byref(cfg), C.byref(h))
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, _abi.status_str(st))
        self._h = h
        self.device = device
        self.num_services = int(num_services)
        self.services = None if services is None else list(services)
        self.matched = 0  # matching entries of the last getTraceIdsByAnnotation
        self._held = None  # device entry columns a queued observe may still read (observe_stored)

    def _check(self, st: int) -> None:
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_ax_last_error(self._h).decode() or _abi.status_str(st))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.zk_ax_destroy(self._h)
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
    def observe(self, items, *, sync: bool = True) -> None:
        """Enter every entry of `items` (AnnotationItems or DeviceAnnotationItems, any order) as one
        segment (zk_ax_observe). Observing a batch again adds its entries again. sync=False leaves the
        scatter queued on the handle's stream: device columns must then stay as they are until the next
        call that synchronises (info, trace_ids, compact, expire, observe)."""
        flags = 0
        ab = items.abi()
        if isinstance(items, DeviceAnnotationItems):
            import torch

            flags |= _abi.ZK_BATCH_DEVICE_PTRS
            torch.cuda.current_stream(self.device).synchronize()  # (torch may still be writing the batch)
        self._check(self._L.zk_ax_observe(self._h, C.byref(ab), flags))
        if sync:
            self.info()

    def observe_stored(self, decoder, buf, offsets, n: int, *, snappy: bool = True, strict: bool = True,
                       client_rule: bool = True):
        """Decode one batch of STORED fragments already in HBM (buf uint8, offsets int64[n + 1]: torch
        tensors on the device) with `decoder` (an ingest.DeviceSpanDecoder whose service ids this index
        takes: num_services >= its max_services) and observe its entries in one step: the twin of
        GpuRealtimeAggregates.accumulate_stored. No entry column is copied to the host. Returns
        (cols, rejected, entries_observed). The entry tensors are kept until this handle's next
        synchronising call (info, trace_ids, compact, expire, observe, observe_stored), as
        zk_ax_observe's device-pointer rule requires."""
        import torch

        if self.num_services < decoder.max_services:
            raise ValueError("an index of %d services cannot take the ids of a decoder of %d"
                             % (self.num_services, decoder.max_services))
        torch.cuda.current_stream(self.device).synchronize()  # (the caller's tensors may still be in flight)
        cols, rejected, entries = decoder.decode_device(buf, offsets, n, snappy=snappy, strict=strict, indexed=True,
                                                        client_rule=client_rule)
        if len(entries):
            self.observe(entries, sync=False)
        self._held = entries
        return cols, rejected, len(entries)

    def reset(self) -> None:
        """Empty the index (zk_ax_reset)."""
        self._check(self._L.zk_ax_reset(self._h))

    def compact(self) -> None:
        """Merge all segments into one (zk_ax_compact)."""
        self._check(self._L.zk_ax_compact(self._h))

    def expire(self, min_ts: int) -> int:
        """Remove every entry with ts < min_ts, by the entry's own timestamp (zk_ax_expire); an entry at
        min_ts stays. Returns the number removed. Afterwards the index answers as a fresh one that
        observed only the survivors; segments that lose nothing are kept as they are, the survivors of
        the others go into one new segment. Synchronises."""
        n = C.c_uint64()
        self._check(self._L.zk_ax_expire(self._h, int(min_ts), C.byref(n)))
        return int(n.value)

    def info(self) -> dict:
        """{"entries", "segments", "bytes"} (zk_ax_info); synchronises."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._L.zk_ax_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self._held = None  # (synchronised: the columns of a queued observe are consumed)
        return {"entries": int(a.value), "segments": int(b.value), "bytes": int(c.value)}

    def service_counts(self) -> np.ndarray:
        """Entries per service id, uint64[num_services] (zk_ax_service_counts: host bookkeeping)."""
        out = np.zeros(self.num_services, np.uint64)
        self._check(self._L.zk_ax_service_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    # ---- reading ---------------------------------------------------------------------------------------
    def trace_ids(self, service_id: int, key_hash: int, val_hash: int, end_ts: int, limit: int):
        """zk_ax_trace_ids for one service id, one key hash and one value hash (or ZK_AX_ANY_VALUE = 0):
        (rows [IndexedTraceId], matched)."""
        cap = max(1, min(int(limit), _abi.ZK_AX_MAX_LIMIT))
        ids = np.zeros(cap, np.uint64)
        ts = np.zeros(cap, np.int64)
        n, m = C.c_uint32(), C.c_uint64()
        self._check(self._L.zk_ax_trace_ids(self._h, service_id, int(key_hash) & _M64, int(val_hash) & _M64, end_ts, limit,
                                            ids.ctypes.data_as(C.POINTER(C.c_uint64)), ts.ctypes.data_as(C.POINTER(C.c_int64)),
                                            C.byref(n), C.byref(m)))
        c = int(n.value)
        return [IndexedTraceId(i, t) for i, t in zip(ids[:c].tolist(), ts[:c].tolist())], int(m.value)

    def _service_ids(self, service: Union[int, str]) -> List[int]:
        if isinstance(service, str):
            return [i for i in _fold_ids(self.services, service, 0) if i < self.num_services]
        return [int(service)]

    def getTraceIdsByAnnotation(self, service: Union[int, str], annotation: Union[str, bytes, int],
                                value: Optional[bytes], end_ts: int, limit: int) -> List[IndexedTraceId]:
        """SpanStore.getTraceIdsByAnnotation: the newest `limit` (traceId, timestamp) of `service` with a
        time annotation of value `annotation` or a binary annotation of key `annotation` (value None), or
        with a binary annotation (annotation, value); timestamp <= end_ts; timestamp descending, equal
        timestamps by traceId ascending. `annotation` may be the key hash itself. A core annotation
        (cs, cr, sr, ss) yields [] without a device call (SpanStore.scala:201). `matched` holds the number
        of matching entries after the call. A service string that no dictionary entry matches yields [];
        one that several ids match is asked per id and the answers are merged (merge_trace_ids)."""
        self.matched = 0
        if isinstance(annotation, int):
            key = annotation
        else:
            if _bytes(annotation) in CORE_ANNOTATIONS:
                return []
            key = key_hash(annotation)
        val = _abi.ZK_AX_ANY_VALUE if value is None else value_hash(value)
        lists = []
        for s in self._service_ids(service):
            rows, m = self.trace_ids(s, key, val, int(end_ts), int(limit))
            lists.append(rows)
            self.matched += m
        if len(lists) == 1:
            return lists[0]
        return merge_trace_ids(lists, limit)

    # ---- the query service -----------------------------------------------------------------------------
    def getTraceIdsByAnnotationOrdered(self, service, annotation, value, end_ts: int, limit: int, order: Optional[str],
                                       durations) -> List[int]:
        """QueryService.getTraceIdsByAnnotation (:259-284): the index's ids through
        durations.sortTraceIds(ids, limit, order) (a durations.TraceDurationIndex over the same
        batches); order=None returns them as indexed. An empty or None annotation raises
        ValueError("No annotation provided"); an empty value asks the annotation alone."""
        if annotation is None or (not isinstance(annotation, int) and len(annotation) == 0):
            raise ValueError("No annotation provided")
        if value is not None and len(value) == 0:
            value = None
        ids = [t.trace_id for t in self.getTraceIdsByAnnotation(service, annotation, value, end_ts, limit)]
        return durations.sortTraceIds(ids, limit, order) if order is not None else ids

    # ---- timing ----------------------------------------------------------------------------------------
    def observe_ms(self) -> dict:
        """Device time (ms) of the passes of the last observe (zk_ax_observe_ms; timing=True)."""
        out = (C.c_double * len(self.OBSERVE_PHASES))()
        self._check(self._L.zk_ax_observe_ms(self._h, out))
        return dict(zip(self.OBSERVE_PHASES, out))

    def expire_ms(self) -> dict:
        """Device time (ms) of the passes of the last expire (zk_ax_expire_ms; timing=True)."""
        out = (C.c_double * len(self.EXPIRE_PHASES))()
        self._check(self._L.zk_ax_expire_ms(self._h, out))
        return dict(zip(self.EXPIRE_PHASES, out))

    def query_ms(self) -> float:
        """Time (ms) on the handle's stream of the last trace_ids pass (zk_ax_query_ms)."""
        ms = C.c_double()
        self._check(self._L.zk_ax_query_ms(self._h, C.byref(ms)))
        return float(ms.value)


def trace_ids_intersect(id_lists: Sequence[Sequence[IndexedTraceId]]) -> List[IndexedTraceId]:
    """QueryService.traceIdsIntersect (:185-207): one row per trace id present in every list, carrying
    its maximum timestamp over all lists; in the order of the first list's first occurrences."""
    if not id_lists:
        return []
    common = set(t[0] for t in id_lists[0])
    for l in id_lists[1:]:
        common &= set(t[0] for t in l)
    best = {}
    for l in id_lists:
        for tid, ts in l:
            if tid in common and (tid not in best or ts > best[tid]):
                best[tid] = ts
    out, seen = [], set()
    for tid, _ in id_lists[0]:
        if tid in common and tid not in seen:
            seen.add(tid)
            out.append(IndexedTraceId(tid, best[tid]))
    return out


def get_trace_ids(names, annotations, service, span_name=None, annotation_list: Optional[Sequence] = None,
                  binary_annotations: Optional[Sequence[Tuple[Union[str, bytes], bytes]]] = None, end_ts: int = 0,
                  limit: int = 10) -> Tuple[List[IndexedTraceId], int]:
    """QueryService.getTraceIds (:97-207) up to, and not including, constructQueryResponse:
    (rows, end_ts_out). `names` answers getTraceIdsByName(service, span_name, end_ts, limit) (a
    TraceNameIndex), `annotations` getTraceIdsByAnnotation(service, annotation, value, end_ts, limit) (a
    TraceAnnotationIndex). The slices are: span_name (when not None), each of annotation_list (value
    None), each (key, value) of binary_annotations.
      - no slice: the service-level call, names.getTraceIdsByName(service, None, end_ts, limit);
      - one slice: that slice at `limit`;
      - several: each is probed at limit 1; the minimum probe timestamp + 60,000,000 us
        (TraceTimestampPadding) becomes the end time; each is then run at `limit` and the results are
        intersected by trace id (trace_ids_intersect). With no common id the result is [] and
        end_ts_out is the maximum over the slices of each slice's minimum timestamp.
    end_ts_out is otherwise the end time the slices ran at. Where the reference throws on the minimum
    or maximum of an empty list, this does not: when every probe is empty the result is ([], end_ts),
    and slices without rows are left out of the maximum."""
    slices = []
    if span_name is not None:
        slices.append(lambda e, l: names.getTraceIdsByName(service, span_name, e, l))
    for a in annotation_list or ():
        slices.append(lambda e, l, a=a: annotations.getTraceIdsByAnnotation(service, a, None, e, l))
    for k, v in binary_annotations or ():
        slices.append(lambda e, l, k=k, v=v: annotations.getTraceIdsByAnnotation(service, k, v, e, l))
    end_ts, limit = int(end_ts), int(limit)
    if not slices:
        return list(names.getTraceIdsByName(service, None, end_ts, limit)), end_ts
    if len(slices) == 1:
        return list(slices[0](end_ts, limit)), end_ts
    probes = [t.timestamp for q in slices for t in q(end_ts, 1)]
    if not probes:
        return [], end_ts
    padded = min(min(probes) + TRACE_TIMESTAMP_PADDING_US, INT64_MAX)  # (the reference's sum would wrap)
    ids = [list(q(padded, limit)) for q in slices]
    common = trace_ids_intersect(ids)
    if not common:
        mins = [min(t.timestamp for t in l) for l in ids if l]
        return [], (max(mins) if mins else end_ts)
    return common, padded
