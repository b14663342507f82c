"""The annotation store by trace id (include/zkannots.h): a span's time annotations in HBM, next to the span
store, so that the time-skew adjuster and the trace timelines of the query service have what the 48-B record
drops: each annotation's own timestamp, the kind of its value and its host.

TraceAnnotationStore keeps every observed 44-B row, grouped by the span store's hash of its trace id, and
hands the rows of asked traces back. A trace's annotations travel as a list of ROWS, tuples (trace_id,
span_id, ts, value, ipv4, service_id, bits) of Python ints, in the header's canonical order. The adjuster and
the timeline over them are in spanstore.py.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from .columns import ADJUSTED_TRACE_HEAD, ADJUSTED_TRACE_SPAN, ENTRY_COLUMNS, SUMMARY_HEAD

_M64 = 2 ** 64 - 1

AnnotationRow = Tuple[int, int, int, int, int, int, int]

ROW_COLUMNS = (("trace_id", np.uint64), ("span_id", np.uint64), ("ts", np.int64), ("value", np.uint64),
               ("ipv4", np.uint32), ("service_id", np.uint32), ("bits", np.uint32))

# zk_an_adjusted_summaries' answer: zk_sp_summary heads with two more state bits, and zk_sp_span_ts entries
ADJUSTED_HEAD, ADJUSTED_ENTRY_COLUMNS = SUMMARY_HEAD, ENTRY_COLUMNS
ADJ_ANNOTATED, ADJ_OVERFLOW = _abi.ZK_AN_ADJ_ANNOTATED, _abi.ZK_AN_ADJ_OVERFLOW

KIND_OTHER, KIND_CS, KIND_CR, KIND_SR, KIND_SS = 0, 1, 2, 3, 4
KIND_NAMES = ("", "cs", "cr", "sr", "ss")
LOOPBACK_IPV4 = (127 << 24) | 1


def annotation_key(row: AnnotationRow) -> tuple:
    """The canonical order inside a trace: (span_id, ts, kind, value, ipv4, port, service_id, HAS_HOST), and
    last the whole bits word."""
    _, sid, ts, value, ipv4, svc, bits = row
    return (sid, ts, bits & _abi.ZK_AN_KIND_MASK, value, ipv4, bits >> _abi.ZK_AN_PORT_SHIFT, svc,
            bits & _abi.ZK_AN_HAS_HOST, bits)


def row_bits(kind: int, has_host: bool, port: int = 0) -> int:
    """The bits word of a row: the kind, ZK_AN_HAS_HOST, the port's 16 bits."""
    return (kind & _abi.ZK_AN_KIND_MASK) | (_abi.ZK_AN_HAS_HOST if has_host else 0) | ((port & 0xFFFF) << _abi.ZK_AN_PORT_SHIFT)


class Endpoint(NamedTuple):
    """An annotation's host: the ipv4's 32 bits and the port's 16 bits as unsigned values, the service id."""
    ipv4: int
    port: int
    service_id: int


class Annotation(NamedTuple):
    """One time annotation of a span. value: zk_hash_string of the text. kind: 0 other, 1 cs, 2 cr, 3 sr,
    4 ss. host: None without one."""
    ts: int
    value: int
    kind: int
    host: Optional[Endpoint]

    @staticmethod
    def of_row(row: AnnotationRow) -> "Annotation":
        _, _, ts, value, ipv4, svc, bits = row
        host = Endpoint(ipv4, bits >> _abi.ZK_AN_PORT_SHIFT, svc) if bits & _abi.ZK_AN_HAS_HOST else None
        return Annotation(ts, value, bits & _abi.ZK_AN_KIND_MASK, host)


class AnnotationRows:
    """The annotation store's rows as seven host columns (zk_an_cols): trace_id, span_id uint64, ts int64,
    value uint64, ipv4, service_id, bits uint32."""

    def __init__(self, trace_id, span_id, ts, value, ipv4, service_id, bits):
        given = (trace_id, span_id, ts, value, ipv4, service_id, bits)
        for (name, dt), a in zip(ROW_COLUMNS, given):
            setattr(self, name, np.ascontiguousarray(a, dtype=dt))
        if len({len(getattr(self, name)) for name, _ in ROW_COLUMNS}) != 1:
            raise ValueError("the seven columns differ in length")

    @classmethod
    def empty(cls, n: int) -> "AnnotationRows":
        return cls(*[np.zeros(n, dt) for _, dt in ROW_COLUMNS])

    @classmethod
    def of_rows(cls, rows: Sequence[AnnotationRow]) -> "AnnotationRows":
        cols = list(zip(*rows)) if len(rows) else [[] for _ in ROW_COLUMNS]
        return cls(*[np.array([int(v) for v in c], dt) for c, (_, dt) in zip(cols, ROW_COLUMNS)])

    @classmethod
    def concat(cls, parts: Sequence["AnnotationRows"]) -> "AnnotationRows":
        return cls(*[np.concatenate([getattr(p, name) for p in parts]) if parts else np.zeros(0, dt) for name, dt in ROW_COLUMNS])

    def __len__(self) -> int:
        return len(self.trace_id)

    def take(self, sel) -> "AnnotationRows":
        return AnnotationRows(*[getattr(self, name)[sel] for name, _ in ROW_COLUMNS])

    def rows(self) -> List[AnnotationRow]:
        """[(trace_id, span_id, ts, value, ipv4, service_id, bits)] as Python ints."""
        return list(zip(*[getattr(self, name).tolist() for name, _ in ROW_COLUMNS]))

    def abi(self) -> _abi.zk_an_cols:
        return _abi.zk_an_cols(*[getattr(self, name).ctypes.data for name, _ in ROW_COLUMNS])

    def ingest_abi(self, cap: Optional[int] = None, n: Optional[int] = None) -> _abi.zk_ingest_annotation_rows:
        return _abi.zk_ingest_annotation_rows(*[getattr(self, name).ctypes.data for name, _ in ROW_COLUMNS],
                                              len(self) if cap is None else cap, len(self) if n is None else n)


class DeviceAnnotationRows:
    """The same seven columns as torch tensors on the device (the 8-byte columns int64, the 4-byte ones
    int32: the bit patterns of the unsigned columns)."""

    def __init__(self, trace_id, span_id, ts, value, ipv4, service_id, bits):
        self.trace_id, self.span_id, self.ts, self.value = trace_id, span_id, ts, value
        self.ipv4, self.service_id, self.bits = ipv4, service_id, bits
        self.device = trace_id.device.index or 0

    @classmethod
    def from_host(cls, rows: AnnotationRows, device: int = 0) -> "DeviceAnnotationRows":
        import torch

        dev = f"cuda:{device}"
        return cls(*[torch.from_numpy(getattr(rows, name).view(np.int64 if np.dtype(dt).itemsize == 8 else np.int32).copy()).to(dev)
                     for name, dt in ROW_COLUMNS])

    def __len__(self) -> int:
        return int(self.trace_id.numel())

    def abi(self) -> _abi.zk_an_cols:
        return _abi.zk_an_cols(*[getattr(self, name).data_ptr() for name, _ in ROW_COLUMNS])


class TraceAnnotationStore:
    """A zk_an handle. `with TraceAnnotationStore() as store:` frees it on exit. Making one touches no
    device: the first observe that carries rows opens it."""

    OBSERVE_PHASES = ("count", "size", "scatter")
    EXPIRE_PHASES = ("ends", "size", "rewrite")

    def __init__(self, device: int = 0, timing: bool = False, stream: Optional[int] = None, expire_chunk: int = 0):
        self._L = _abi.lib()
        cfg = _abi.zk_an_config()
        cfg.device = device
        cfg.timing = 1 if timing else 0
        cfg.stream = stream
        cfg.expire_chunk = expire_chunk  # expire's entries per range of buckets at most (0: 2^24)
        h = C.c_void_p()
        st = self._L.zk_an_create(C.byref(cfg), C.byref(h))
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, _abi.status_str(st))
        self._h = h
        self.device = device
        self._held = None  # device row columns a queued observe may still read (observe_stored)

    def _check(self, st: int) -> None:
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_an_last_error(self._h).decode() or _abi.status_str(st))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.zk_an_destroy(self._h)
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
    def observe(self, rows, *, sync: bool = True) -> None:
        """Add a batch's rows (AnnotationRows or DeviceAnnotationRows, any order) as one segment
        (zk_an_observe). Observing a batch again adds it again. sync=False leaves the scatter queued on the
        handle's stream: device columns must then stay as they are until the next call that synchronises
        (info, gather, compact, expire, observe)."""
        flags = 0
        ab = rows.abi()
        if isinstance(rows, DeviceAnnotationRows):
            import torch

            flags |= _abi.ZK_BATCH_DEVICE_PTRS
            torch.cuda.current_stream(self.device).synchronize()  # (torch may still be writing the batch)
        self._check(self._L.zk_an_observe(self._h, C.byref(ab), len(rows), flags))
        if sync:
            self.info()

    def observe_stored(self, decoder, buf, offsets, n: int, *, snappy: bool = True, strict: bool = True, spans=None,
                       row_strings: bool = True, binary=None):
        """Decode one batch of STORED fragments already in HBM (buf uint8, offsets int64[n + 1]: torch tensors
        on the device) with `decoder` (an ingest.DeviceSpanDecoder) and observe its annotation rows in one
        step: the twin of TraceAnnotationIndex.observe_stored. No row column is copied to the host. With
        spans= (a spanstore.TraceSpanStore on the same device) the same call's record columns are observed
        there too, so both stores are fed the same batch (zkannots.h "Expiry", the invariant). Returns
        (cols, rejected, rows_observed). The row tensors are kept until this handle's next synchronising call
        (info, gather, compact, expire, observe_stored; observe(sync=True) ends in info), the record columns
        until the span store's next info() or the next observe_stored(spans=) on it: longer than the
        device-pointer rule of zk_an_observe / zk_sp_observe requires, never shorter. row_strings=False leaves the
        values' strings uncaptured (the adjuster and the summaries need no text; a timeline does).
        With binary= (a binannotstore.TraceBinaryAnnotationStore on the same device) the same call's rows pass
        also emits the batch's binary-annotation rows (zk_ingest_dev_spans_annotated_binary) and they are
        observed there, held until that store's next synchronising call; row_strings covers their keys and
        values too."""
        import torch

        torch.cuda.current_stream(self.device).synchronize()  # (the caller's tensors may still be in flight)
        if binary is not None:
            cols, rejected, rows, brows = decoder.decode_device(buf, offsets, n, snappy=snappy, strict=strict, annotated=True,
                                                                row_strings=row_strings, binary=True)
            if len(brows):
                binary.observe(brows, sync=False)
            binary._held = brows
        else:
            cols, rejected, rows = decoder.decode_device(buf, offsets, n, snappy=snappy, strict=strict, annotated=True,
                                                         row_strings=row_strings)
        if len(rows):
            self.observe(rows, sync=False)
        self._held = rows
        if spans is not None:
            if cols.n:
                spans.observe(cols, sync=False)
            spans._held = cols
        return cols, rejected, len(rows)

    def reset(self) -> None:
        """Empty the store (zk_an_reset)."""
        self._check(self._L.zk_an_reset(self._h))

    def compact(self) -> None:
        """Merge all segments into one (zk_an_compact)."""
        self._check(self._L.zk_an_compact(self._h))
        self._held = None  # (synchronised)

    def expire(self, min_end: int, pins: Optional[Dict[int, int]] = None) -> int:
        """Remove every trace whose end (the maximum ts of its rows) is below its cutoff, whole
        (zk_an_expire): the cutoff is min_end, or pins[trace_id] for a pinned trace. The rows removed. More
        than ZK_AN_MAX_PINS pins are refused: a second call would judge the first call's pinned traces by
        the default."""
        pins = {} if pins is None else dict(pins)
        if len(pins) > _abi.ZK_AN_MAX_PINS:
            raise ValueError("more than ZK_AN_MAX_PINS pins in one expiry")
        ids = np.array([int(k) & _M64 for k in pins], np.uint64)
        cuts = np.array([int(v) for v in pins.values()], np.int64)
        removed = C.c_uint64()
        self._check(self._L.zk_an_expire(self._h, int(min_end), ids.ctypes.data if len(ids) else None,
                                         cuts.ctypes.data if len(ids) else None, len(ids), C.byref(removed)))
        self._held = None  # (synchronised)
        return int(removed.value)

    def info(self) -> dict:
        """{"entries", "segments", "bytes"} (zk_an_info); synchronises."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._L.zk_an_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self._held = None  # (synchronised: the columns of a queued observe are consumed)
        return {"entries": int(a.value), "segments": int(b.value), "bytes": int(c.value)}

    # ---- reading ---------------------------------------------------------------------------------------
    def _ask(self, ids):
        """(keep-alive, pointer, n, flags) of an ask: anything numpy turns into uint64, or a torch int64
        tensor on the handle's device (the ids' bit patterns)."""
        if hasattr(ids, "data_ptr"):
            import torch

            if ids.dtype != torch.int64 or not ids.is_contiguous() or ids.device.index != self.device:
                raise ValueError("device ids: a contiguous int64 tensor on the handle's device")
            torch.cuda.current_stream(self.device).synchronize()
            return ids, ids.data_ptr(), int(ids.numel()), _abi.ZK_BATCH_DEVICE_PTRS
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
        return a, a.ctypes.data, len(a), 0

    def gather(self, ids):
        """(counts uint32[n], AnnotationRows) for at most ZK_AN_MAX_IDS ids (zk_an_gather): the sizing call,
        then the call that fills seven columns of exactly the total."""
        keep, ptr, n, flags = self._ask(ids)
        counts = np.zeros(n, np.uint32)
        cp = counts.ctypes.data_as(_abi._U32P)
        total = C.c_uint64()
        st = self._L.zk_an_gather(self._h, ptr, n, flags, cp, None, 0, C.byref(total))
        if st not in (_abi.ZK_OK, _abi.ZK_ERR_CAPACITY):
            self._check(st)
        rows = AnnotationRows.empty(total.value)
        if st == _abi.ZK_ERR_CAPACITY:
            ab = rows.abi()
            self._check(self._L.zk_an_gather(self._h, ptr, n, flags, cp, C.byref(ab), total.value, C.byref(total)))
        self._held = None  # (synchronised)
        return counts, rows

    def _chunks(self, ids):
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
        for a in range(0, len(ids), _abi.ZK_AN_MAX_IDS):
            yield ids[a:a + _abi.ZK_AN_MAX_IDS]

    def getAnnotationsByTraceIds(self, ids) -> List[List[AnnotationRow]]:
        """One list of rows, in canonical order, per asked id, in the order asked: [] for an id without
        rows (the lists line up with the ids, unlike getSpansByTraceIds), a duplicated id answered as often
        as asked. More than ZK_AN_MAX_IDS ids go in chunks."""
        out: List[List[AnnotationRow]] = []
        for part in self._chunks(ids):
            counts, got = self.gather(part)
            rows = got.rows()
            at = 0
            for c in counts.tolist():
                out.append(rows[at:at + c])
                at += c
        return out

    def adjusted_summaries(self, spans, ids):
        """(heads, entries) for at most ZK_AN_MAX_IDS ids (zk_an_adjusted_summaries): the trace summaries after
        the time-skew adjuster, joined on the device from this store's rows and `spans`, a TraceSpanStore on
        the same device. heads: an ADJUSTED_HEAD array in the order asked (state: ZK_SP_SUM_FOUND / _TIMED,
        ADJ_ANNOTATED, ADJ_OVERFLOW); entries: the (service_id, first, last) of all asked traces one after
        another (a dict of three numpy columns of exactly the total). The sizing call, then the call that
        fills."""
        keep, ptr, n, flags = self._ask(ids)
        heads = np.zeros(n, ADJUSTED_HEAD)
        total = C.c_uint64()
        st = self._L.zk_an_adjusted_summaries(self._h, spans._h, ptr, n, flags, heads.ctypes.data, None, 0, C.byref(total))
        if st not in (_abi.ZK_OK, _abi.ZK_ERR_CAPACITY):
            self._check(st)
        cols = {k: np.zeros(total.value, dt) for k, dt in ADJUSTED_ENTRY_COLUMNS}
        if st == _abi.ZK_ERR_CAPACITY:
            out = _abi.zk_sp_span_ts(*[cols[k].ctypes.data for k, _ in ADJUSTED_ENTRY_COLUMNS])
            self._check(self._L.zk_an_adjusted_summaries(self._h, spans._h, ptr, n, flags, heads.ctypes.data, C.byref(out),
                                                         total.value, C.byref(total)))
        return heads, cols

    def adjusted_traces(self, spans, ids):
        """(heads, spans, services, rows) for at most ZK_AN_MAX_IDS ids (zk_an_adjusted_traces): the asked traces
        after the time-skew adjuster, with every span's annotations, joined on the device from this store's rows
        and `spans`, a TraceSpanStore on the same device. heads: an ADJUSTED_TRACE_HEAD array in the order
        asked; spans: an ADJUSTED_TRACE_SPAN array, the traces one after another, each in its adjusted span
        order; services: the spans' service ids, a uint32 column; rows: AnnotationRows, per span in that order
        its annotations in list order, the injected sr / ss of a client-only span behind its own. The sizing
        call, then the call that fills."""
        keep, ptr, n, flags = self._ask(ids)
        heads = np.zeros(n, ADJUSTED_TRACE_HEAD)
        totals = (C.c_uint64 * 3)()
        st = self._L.zk_an_adjusted_traces(self._h, spans._h, ptr, n, flags, heads.ctypes.data, None, 0, None, 0, None, 0, totals)
        if st not in (_abi.ZK_OK, _abi.ZK_ERR_CAPACITY):
            self._check(st)
        out_spans, services = np.zeros(totals[0], ADJUSTED_TRACE_SPAN), np.zeros(totals[1], np.uint32)
        rows = AnnotationRows.empty(totals[2])
        if st == _abi.ZK_ERR_CAPACITY:
            ab = rows.abi()
            self._check(self._L.zk_an_adjusted_traces(self._h, spans._h, ptr, n, flags, heads.ctypes.data, out_spans.ctypes.data,
                                                      len(out_spans), services.ctypes.data, len(services), C.byref(ab), len(rows), totals))
        return heads, out_spans, services, rows

    # ---- timing ----------------------------------------------------------------------------------------
    def observe_ms(self) -> dict:
        """Device time (ms) of the passes of the last observe (zk_an_observe_ms; timing=True)."""
        out = (C.c_double * len(self.OBSERVE_PHASES))()
        self._check(self._L.zk_an_observe_ms(self._h, out))
        return dict(zip(self.OBSERVE_PHASES, out))

    def expire_ms(self) -> dict:
        """Device time (ms) of the passes of the last expire that ran one (zk_an_expire_ms; timing=True)."""
        out = (C.c_double * len(self.EXPIRE_PHASES))()
        self._check(self._L.zk_an_expire_ms(self._h, out))
        return dict(zip(self.EXPIRE_PHASES, out))

    def query_ms(self) -> float:
        """Time (ms) on the handle's stream of the last gather, adjusted_summaries or adjusted_traces (zk_an_query_ms;
        timing=True)."""
        ms = C.c_double()
        self._check(self._L.zk_an_query_ms(self._h, C.byref(ms)))
        return float(ms.value)
