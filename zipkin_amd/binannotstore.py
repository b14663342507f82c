"""The binary-annotation store by trace id (include/zkbinannots.h): a span's key/value annotations (Span
field 8) in HBM, next to the span store and the annotation store, for Trace.getBinaryAnnotations,
getBinaryAnnotationsByKey and the fourth field of a TraceTimeline.

TraceBinaryAnnotationStore keeps every observed 44-B row and hands the rows of asked traces back. The store is
the annotation store's code behind a typed facade (zk_bn_*): same segments, same bucket function, same gather.
A trace's binary annotations travel as a list of ROWS, tuples (trace_id, span_id, key, value, ipv4,
service_id, bits) of Python ints, in the header's canonical order; key and value are zk_hash_string hashes
(the decoders keep the bytes: SpanDecoder.bytes / DeviceSpanDecoder.bytes).
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from .annotstore import Endpoint

_M64 = 2 ** 64 - 1

BinaryAnnotationRow = Tuple[int, int, int, int, int, int, int]

BINARY_ROW_COLUMNS = (("trace_id", np.uint64), ("span_id", np.uint64), ("key", np.uint64), ("value", np.uint64),
                      ("ipv4", np.uint32), ("service_id", np.uint32), ("bits", np.uint32))

TYPE_BOOL, TYPE_BYTES, TYPE_I16, TYPE_I32, TYPE_I64, TYPE_DOUBLE, TYPE_STRING, TYPE_OTHER = range(8)
TYPE_NAMES = ("BOOL", "BYTES", "I16", "I32", "I64", "DOUBLE", "STRING", "OTHER")


def _signed(v: int) -> int:
    v &= _M64
    return v - (1 << 64) if v >> 63 else v


def binary_annotation_key(row: BinaryAnnotationRow) -> tuple:
    """The canonical order inside a trace: (span_id, key as the signed i64 its bits are, type, value, ipv4,
    port, service_id, HAS_HOST), and last the whole bits word."""
    _, sid, key, value, ipv4, svc, bits = row
    return (sid, _signed(key), bits & _abi.ZK_BN_TYPE_MASK, value, ipv4, bits >> _abi.ZK_BN_PORT_SHIFT, svc,
            bits & _abi.ZK_BN_HAS_HOST, bits)


def binary_row_bits(type_: int, has_host: bool, port: int = 0) -> int:
    """The bits word of a row: the type (a value outside 0..6 is ZK_BN_TYPE_OTHER), ZK_BN_HAS_HOST, the port."""
    t = type_ if 0 <= type_ <= 6 else _abi.ZK_BN_TYPE_OTHER
    return t | (_abi.ZK_BN_HAS_HOST if has_host else 0) | ((port & 0xFFFF) << _abi.ZK_BN_PORT_SHIFT)


class BinaryAnnotation(NamedTuple):
    """One binary annotation of a span. key, value: zk_hash_string hashes, or, once resolved through a
    decoder, the key's text and the value's bytes. type: the AnnotationType ordinal (0 BOOL .. 6 STRING, 7
    other). host: None without one; its service_id becomes a name with a services dictionary."""
    key: object
    value: object
    type: int
    host: Optional[Endpoint]
    span_id: int

    @staticmethod
    def of_row(row: BinaryAnnotationRow) -> "BinaryAnnotation":
        _, sid, key, value, ipv4, svc, bits = row
        host = Endpoint(ipv4, bits >> _abi.ZK_BN_PORT_SHIFT, svc) if bits & _abi.ZK_BN_HAS_HOST else None
        return BinaryAnnotation(key, value, bits & _abi.ZK_BN_TYPE_MASK, host, sid)


class BinaryAnnotationRows:
    """The store's rows as seven host columns (zk_bn_cols): trace_id, span_id, key, value uint64, ipv4,
    service_id, bits uint32."""

    def __init__(self, trace_id, span_id, key, value, ipv4, service_id, bits):
        given = (trace_id, span_id, key, value, ipv4, service_id, bits)
        for (name, dt), a in zip(BINARY_ROW_COLUMNS, given):
            setattr(self, name, np.ascontiguousarray(a, dtype=dt))
        if len({len(getattr(self, name)) for name, _ in BINARY_ROW_COLUMNS}) != 1:
            raise ValueError("the seven columns differ in length")

    @classmethod
    def empty(cls, n: int) -> "BinaryAnnotationRows":
        return cls(*[np.zeros(n, dt) for _, dt in BINARY_ROW_COLUMNS])

    @classmethod
    def of_rows(cls, rows: Sequence[BinaryAnnotationRow]) -> "BinaryAnnotationRows":
        cols = list(zip(*rows)) if len(rows) else [[] for _ in BINARY_ROW_COLUMNS]
        return cls(*[np.array([int(v) for v in c], dt) for c, (_, dt) in zip(cols, BINARY_ROW_COLUMNS)])

    @classmethod
    def concat(cls, parts: Sequence["BinaryAnnotationRows"]) -> "BinaryAnnotationRows":
        return cls(*[np.concatenate([getattr(p, name) for p in parts]) if parts else np.zeros(0, dt)
                     for name, dt in BINARY_ROW_COLUMNS])

    def __len__(self) -> int:
        return len(self.trace_id)

    def take(self, sel) -> "BinaryAnnotationRows":
        return BinaryAnnotationRows(*[getattr(self, name)[sel] for name, _ in BINARY_ROW_COLUMNS])

    def rows(self) -> List[BinaryAnnotationRow]:
        """[(trace_id, span_id, key, value, ipv4, service_id, bits)] as Python ints."""
        return list(zip(*[getattr(self, name).tolist() for name, _ in BINARY_ROW_COLUMNS]))

    def abi(self) -> _abi.zk_bn_cols:
        return _abi.zk_bn_cols(*[getattr(self, name).ctypes.data for name, _ in BINARY_ROW_COLUMNS])

    def ingest_abi(self, cap: Optional[int] = None, n: Optional[int] = None) -> _abi.zk_ingest_binary_rows:
        return _abi.zk_ingest_binary_rows(*[getattr(self, name).ctypes.data for name, _ in BINARY_ROW_COLUMNS],
                                          len(self) if cap is None else cap, len(self) if n is None else n)


class DeviceBinaryAnnotationRows:
    """The same seven columns as torch tensors on the device (the 8-byte columns int64, the 4-byte ones
    int32: the bit patterns of the unsigned columns)."""

    def __init__(self, trace_id, span_id, key, value, ipv4, service_id, bits):
        self.trace_id, self.span_id, self.key, self.value = trace_id, span_id, key, value
        self.ipv4, self.service_id, self.bits = ipv4, service_id, bits
        self.device = trace_id.device.index or 0

    @classmethod
    def from_host(cls, rows: BinaryAnnotationRows, device: int = 0) -> "DeviceBinaryAnnotationRows":
        import torch

        dev = f"cuda:{device}"
        return cls(*[torch.from_numpy(getattr(rows, name).view(np.int64 if np.dtype(dt).itemsize == 8 else np.int32).copy()).to(dev)
                     for name, dt in BINARY_ROW_COLUMNS])

    def to_host(self) -> BinaryAnnotationRows:
        return BinaryAnnotationRows(*[getattr(self, name).cpu().numpy().view(dt) for name, dt in BINARY_ROW_COLUMNS])

    def __len__(self) -> int:
        return int(self.trace_id.numel())

    def abi(self) -> _abi.zk_bn_cols:
        return _abi.zk_bn_cols(*[getattr(self, name).data_ptr() for name, _ in BINARY_ROW_COLUMNS])


class TraceBinaryAnnotationStore:
    """A zk_bn handle. `with TraceBinaryAnnotationStore() as store:` frees it on exit. Making one touches no
    device: the first observe that carries rows opens it. There is no expiry (a binary row has no time of its
    own): reset() is the only removal."""

    OBSERVE_PHASES = ("count", "size", "scatter")

    def __init__(self, device: int = 0, timing: bool = False, stream: Optional[int] = None):
        self._L = _abi.lib()
        cfg = _abi.zk_an_config()
        cfg.device = device
        cfg.timing = 1 if timing else 0
        cfg.stream = stream
        h = C.c_void_p()
        st = self._L.zk_bn_create(C.byref(cfg), C.byref(h))
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, _abi.status_str(st))
        self._h = h
        self.device = device
        self._held = None  # device row columns a queued observe may still read (observe_stored)

    def _check(self, st: int) -> None:
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_bn_last_error(self._h).decode() or _abi.status_str(st))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.zk_bn_destroy(self._h)
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
        """Add a batch's rows (BinaryAnnotationRows or DeviceBinaryAnnotationRows, any order) as one segment
        (zk_bn_observe). Observing a batch again adds it again. sync=False leaves the scatter queued on the
        handle's stream: device columns must then stay as they are until the next call that synchronises
        (info, gather, compact, observe)."""
        flags = 0
        ab = rows.abi()
        if isinstance(rows, DeviceBinaryAnnotationRows):
            import torch

            flags |= _abi.ZK_BATCH_DEVICE_PTRS
            torch.cuda.current_stream(self.device).synchronize()  # (torch may still be writing the batch)
        self._check(self._L.zk_bn_observe(self._h, C.byref(ab), len(rows), flags))
        if sync:
            self.info()

    def reset(self) -> None:
        """Empty the store (zk_bn_reset)."""
        self._check(self._L.zk_bn_reset(self._h))

    def compact(self) -> None:
        """Merge all segments into one (zk_bn_compact)."""
        self._check(self._L.zk_bn_compact(self._h))
        self._held = None  # (synchronised)

    def info(self) -> dict:
        """{"entries", "segments", "bytes"} (zk_bn_info); synchronises."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._L.zk_bn_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self._held = None  # (synchronised: the columns of a queued observe are consumed)
        return {"entries": int(a.value), "segments": int(b.value), "bytes": int(c.value)}

    # ---- reading ---------------------------------------------------------------------------------------
    def _ask(self, ids):
        if hasattr(ids, "data_ptr"):
            import torch

            if ids.dtype != torch.int64 or not ids.is_contiguous() or ids.device.index != self.device:
                raise ValueError("device ids: a contiguous int64 tensor on the handle's device")
            torch.cuda.current_stream(self.device).synchronize()
            return ids, ids.data_ptr(), int(ids.numel()), _abi.ZK_BATCH_DEVICE_PTRS
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
        return a, a.ctypes.data, len(a), 0

    def gather(self, ids):
        """(counts uint32[n], BinaryAnnotationRows) for at most ZK_BN_MAX_IDS ids (zk_bn_gather): the sizing
        call, then the call that fills seven columns of exactly the total."""
        keep, ptr, n, flags = self._ask(ids)
        counts = np.zeros(n, np.uint32)
        cp = counts.ctypes.data_as(_abi._U32P)
        total = C.c_uint64()
        st = self._L.zk_bn_gather(self._h, ptr, n, flags, cp, None, 0, C.byref(total))
        if st not in (_abi.ZK_OK, _abi.ZK_ERR_CAPACITY):
            self._check(st)
        rows = BinaryAnnotationRows.empty(total.value)
        if st == _abi.ZK_ERR_CAPACITY:
            ab = rows.abi()
            self._check(self._L.zk_bn_gather(self._h, ptr, n, flags, cp, C.byref(ab), total.value, C.byref(total)))
        self._held = None  # (synchronised)
        return counts, rows

    def getBinaryAnnotationsByTraceIds(self, ids) -> List[List[BinaryAnnotationRow]]:
        """One list of rows, in canonical order, per asked id, in the order asked: [] for an id without rows,
        a duplicated id answered as often as asked. More than ZK_BN_MAX_IDS ids go in chunks."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
        out: List[List[BinaryAnnotationRow]] = []
        for a in range(0, len(ids), _abi.ZK_BN_MAX_IDS):
            counts, got = self.gather(ids[a:a + _abi.ZK_BN_MAX_IDS])
            rows = got.rows()
            at = 0
            for c in counts.tolist():
                out.append(rows[at:at + c])
                at += c
        return out

    # ---- timing ----------------------------------------------------------------------------------------
    def observe_ms(self) -> dict:
        """Device time (ms) of the passes of the last observe (zk_bn_observe_ms; timing=True)."""
        out = (C.c_double * len(self.OBSERVE_PHASES))()
        self._check(self._L.zk_bn_observe_ms(self._h, out))
        return dict(zip(self.OBSERVE_PHASES, out))

    def query_ms(self) -> float:
        """Time (ms) on the handle's stream of the last gather (zk_bn_query_ms; timing=True)."""
        ms = C.c_double()
        self._check(self._L.zk_bn_query_ms(self._h, C.byref(ms)))
        return float(ms.value)
