"""SpanDecoder: stored span fragments (Snappy + TBinaryProtocol thrift Span) -> SpanColumns.

Binds include/zkingest.h. The decoder owns the service-name dictionary; its ids are the
service ids of the columnar records (zkagg.h), the dependency table and the sketches.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np

from . import _abi
from .columns import SpanColumns


def hash_string(s: str | bytes) -> int:
    b = s.encode() if isinstance(s, str) else s
    return int(_abi.lib().zk_hash_string(b, len(b)))


def _pack(blobs):
    """(buf uint8[total], offsets uint64[n + 1], n) of a sequence of bytes objects or of the packed form."""
    if isinstance(blobs, tuple) and len(blobs) == 2 and isinstance(blobs[0], np.ndarray):
        buf = np.ascontiguousarray(blobs[0], dtype=np.uint8)
        offsets = np.ascontiguousarray(blobs[1], dtype=np.uint64)
        return (buf if len(buf) else np.zeros(1, np.uint8)), offsets, len(offsets) - 1
    n = len(blobs)
    offsets = np.zeros(n + 1, np.uint64)
    if n:
        offsets[1:] = np.cumsum([len(b) for b in blobs], dtype=np.uint64)
    return np.frombuffer(b"".join(blobs) or b"\0", dtype=np.uint8), offsets, n


class SpanDecoder:
    def __init__(self):
        self._L = _abi.lib()
        h = C.c_void_p()
        st = self._L.zk_ingest_create(C.byref(h))
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, _abi.status_str(st))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.zk_ingest_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int) -> None:
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_ingest_last_error(self._h).decode() or _abi.status_str(st))

    def decode(self, blobs, *, snappy: bool = True, strict: bool = True, items: bool = False,
               item_cap: int | None = None, one_thread: bool = False, span_names: bool = False):
        """Decode stored fragments: a sequence of bytes objects (one per fragment), or the packed
        form (buf uint8[total], offsets uint64[n + 1]) -- fragment i is buf[offsets[i]:offsets[i+1]].
        Returns (SpanColumns, rejected) or, with items=True, (SpanColumns, rejected,
        (kv_service, kv_key), (ann_service, ann_value)). one_thread: decode on the calling thread
        only (ZK_INGEST_ONE_THREAD; the default splits large batches over up to 16 threads, with the
        same results). span_names: keep the span-name dictionary and write every record's name id
        (id + 1; 0 for "" and "Unknown") into bits 16..31 of flags (ZK_INGEST_SPAN_NAMES)."""
        if isinstance(blobs, tuple) and len(blobs) == 2 and isinstance(blobs[0], np.ndarray):
            buf = np.ascontiguousarray(blobs[0], dtype=np.uint8)
            offsets = np.ascontiguousarray(blobs[1], dtype=np.uint64)
            n = len(offsets) - 1
            if not len(buf):
                buf = np.zeros(1, np.uint8)
        else:
            n = len(blobs)
            offsets = np.zeros(n + 1, np.uint64)
            if n:
                offsets[1:] = np.cumsum([len(b) for b in blobs], dtype=np.uint64)
            buf = np.frombuffer(b"".join(blobs) or b"\0", dtype=np.uint8)
        cols = SpanColumns.empty(n)
        nout, nrej = C.c_uint64(), C.c_uint64()
        it = None
        arrs = None
        if items:
            cap = item_cap if item_cap is not None else max(16, 8 * n)
            arrs = (np.zeros(cap, np.uint32), np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint64))
            it = _abi.zk_ingest_items(arrs[0].ctypes.data, arrs[1].ctypes.data, cap, 0,
                                      arrs[2].ctypes.data, arrs[3].ctypes.data, cap, 0)
        codec = _abi.ZK_CODEC_SNAPPY_THRIFT if snappy else _abi.ZK_CODEC_THRIFT
        flags = (_abi.ZK_INGEST_STRICT if strict else 0) | (_abi.ZK_INGEST_ONE_THREAD if one_thread else 0)
        flags |= _abi.ZK_INGEST_SPAN_NAMES if span_names else 0
        ab = cols.abi()
        self._check(self._L.zk_ingest_spans(self._h, buf.ctypes.data, offsets.ctypes.data, n, codec, flags,
                                            C.byref(ab), C.byref(nout), C.byref(nrej),
                                            C.byref(it) if it is not None else None))
        cols = cols.take(slice(0, nout.value))
        if not items:
            return cols, int(nrej.value)
        kv = (arrs[0][: it.kv_n].copy(), arrs[1][: it.kv_n].copy())
        ann = (arrs[2][: it.ann_n].copy(), arrs[3][: it.ann_n].copy())
        return cols, int(nrej.value), kv, ann

    def decode_indexed(self, blobs, *, snappy: bool = True, strict: bool = True, client_rule: bool = True,
                       span_names: bool = False, item_cap: int | None = None, one_thread: bool = False):
        """decode() that also returns the annotation index's entries (zk_ingest_spans_indexed):
        (SpanColumns, rejected, annindex.AnnotationItems). client_rule=False emits the entries of a
        client-side span of the service "client" too (ZK_INGEST_NO_CLIENT_RULE). item_cap: the entries to
        allow for (default 8 per fragment, at least 16); a batch with more raises ZK_ERR_CAPACITY, and
        the exception's `items` then holds the first item_cap entries."""
        from .annindex import AnnotationItems

        buf, offsets, n = _pack(blobs)
        cols = SpanColumns.empty(n)
        nout, nrej = C.c_uint64(), C.c_uint64()
        cap = int(item_cap) if item_cap is not None else max(16, 8 * n)
        items = AnnotationItems.empty(cap)
        it = items.abi(cap=cap, n=0)
        codec = _abi.ZK_CODEC_SNAPPY_THRIFT if snappy else _abi.ZK_CODEC_THRIFT
        flags = (_abi.ZK_INGEST_STRICT if strict else 0) | (_abi.ZK_INGEST_ONE_THREAD if one_thread else 0)
        flags |= _abi.ZK_INGEST_SPAN_NAMES if span_names else 0
        flags |= 0 if client_rule else _abi.ZK_INGEST_NO_CLIENT_RULE
        ab = cols.abi()
        st = self._L.zk_ingest_spans_indexed(self._h, buf.ctypes.data, offsets.ctypes.data, n, codec, flags,
                                             C.byref(ab), C.byref(nout), C.byref(nrej), C.byref(it))
        items = items.take(slice(0, int(it.n)))
        if st == _abi.ZK_ERR_CAPACITY:
            e = _abi.ZkError(st, self._L.zk_ingest_last_error(self._h).decode() or _abi.status_str(st))
            e.items = items
            raise e
        self._check(st)
        return cols.take(slice(0, nout.value)), int(nrej.value), items

    def decode_annotated(self, blobs, *, snappy: bool = True, strict: bool = True, span_names: bool = False,
                         row_cap: int | None = None, one_thread: bool = False, binary: bool = False,
                         binary_cap: int | None = None):
        """decode() that also returns the annotation store's rows (zk_ingest_spans_annotated):
        (SpanColumns, rejected, annotstore.AnnotationRows), one row per time annotation of every accepted
        span, in record order and the annotation list's order. row_cap: the rows to allow for (default 8
        per fragment, at least 16); a batch with more raises ZK_ERR_CAPACITY, and the exception's `rows`
        then holds the first row_cap rows. A batch that may hold more says so with row_cap.
        binary=True (zk_ingest_spans_annotated_binary) appends the binary-annotation store's rows, a
        binannotstore.BinaryAnnotationRows with one row per binary annotation of every accepted span:
        (cols, rejected, rows, brows). binary_cap: the binary rows to allow for (default 8 per fragment, at
        least 16); the two capacities are judged independently, and the exception of a short one carries
        `rows` and `brows`, each the prefix that fitted."""
        from .annotstore import AnnotationRows
        from .binannotstore import BinaryAnnotationRows

        buf, offsets, n = _pack(blobs)
        cols = SpanColumns.empty(n)
        nout, nrej = C.c_uint64(), C.c_uint64()
        cap = int(row_cap) if row_cap is not None else max(16, 8 * n)
        rows = AnnotationRows.empty(cap)
        an = rows.ingest_abi(cap=cap, n=0)
        codec = _abi.ZK_CODEC_SNAPPY_THRIFT if snappy else _abi.ZK_CODEC_THRIFT
        flags = (_abi.ZK_INGEST_STRICT if strict else 0) | (_abi.ZK_INGEST_ONE_THREAD if one_thread else 0)
        flags |= _abi.ZK_INGEST_SPAN_NAMES if span_names else 0
        ab = cols.abi()
        brows = None
        if binary:
            bcap = int(binary_cap) if binary_cap is not None else max(16, 8 * n)
            brows = BinaryAnnotationRows.empty(bcap)
            bn = brows.ingest_abi(cap=bcap, n=0)
            st = self._L.zk_ingest_spans_annotated_binary(self._h, buf.ctypes.data, offsets.ctypes.data, n, codec, flags,
                                                          C.byref(ab), C.byref(nout), C.byref(nrej), None, C.byref(an),
                                                          C.byref(bn))
            brows = brows.take(slice(0, int(bn.n)))
        else:
            st = self._L.zk_ingest_spans_annotated(self._h, buf.ctypes.data, offsets.ctypes.data, n, codec, flags,
                                                   C.byref(ab), C.byref(nout), C.byref(nrej), None, C.byref(an))
        rows = rows.take(slice(0, int(an.n)))
        if st == _abi.ZK_ERR_CAPACITY:
            e = _abi.ZkError(st, self._L.zk_ingest_last_error(self._h).decode() or _abi.status_str(st))
            e.rows = rows
            e.brows = brows
            e.cols = cols.take(slice(0, nout.value))
            raise e
        self._check(st)
        if binary:
            return cols.take(slice(0, nout.value)), int(nrej.value), rows, brows
        return cols.take(slice(0, nout.value)), int(nrej.value), rows

    @property
    def num_services(self) -> int:
        n = C.c_uint32()
        self._check(self._L.zk_ingest_num_services(self._h, C.byref(n)))
        return int(n.value)

    def service_id(self, name: str) -> int:
        b = name.encode()
        i = C.c_uint32()
        self._check(self._L.zk_ingest_service_id(self._h, b, len(b), C.byref(i)))
        return int(i.value)

    def service_name(self, i: int) -> str:
        ln = C.c_uint64()
        self._check(self._L.zk_ingest_service_name(self._h, i, None, 0, C.byref(ln)))
        buf = C.create_string_buffer(max(1, ln.value))
        self._check(self._L.zk_ingest_service_name(self._h, i, buf, ln.value, C.byref(ln)))
        return buf.raw[: ln.value].decode("utf-8", "surrogateescape")

    def service_names(self) -> List[str]:
        return [self.service_name(i) for i in range(self.num_services)]

    @property
    def num_span_names(self) -> int:
        n = C.c_uint32()
        self._check(self._L.zk_ingest_num_span_names(self._h, C.byref(n)))
        return int(n.value)

    def span_name_id(self, name: str) -> int:
        """The span-name dictionary id of `name` (added if new); a record's flags carry id + 1."""
        b = name.encode()
        i = C.c_uint32()
        self._check(self._L.zk_ingest_span_name_id(self._h, b, len(b), C.byref(i)))
        return int(i.value)

    def span_name(self, i: int) -> str:
        ln = C.c_uint64()
        self._check(self._L.zk_ingest_span_name(self._h, i, None, 0, C.byref(ln)))
        buf = C.create_string_buffer(max(1, ln.value))
        self._check(self._L.zk_ingest_span_name(self._h, i, buf, ln.value, C.byref(ln)))
        return buf.raw[: ln.value].decode("utf-8", "surrogateescape")

    def span_names(self) -> List[str]:
        return [self.span_name(i) for i in range(self.num_span_names)]

    def bytes(self, h: int) -> bytes:
        """The bytes behind a key / value hash, with their length (a binary annotation's value may hold NUL
        and bytes that are no UTF-8)."""
        ln = C.c_uint64()
        self._check(self._L.zk_ingest_string(self._h, h, None, 0, C.byref(ln)))
        buf = C.create_string_buffer(max(1, ln.value))
        self._check(self._L.zk_ingest_string(self._h, h, buf, ln.value, C.byref(ln)))
        return buf.raw[: ln.value]

    def string(self, h: int) -> str:
        return self.bytes(h).decode("utf-8", "surrogateescape")


def snappy_uncompress(data: bytes) -> bytes:
    L = _abi.lib()
    src = np.frombuffer(data or b"\0", dtype=np.uint8)
    n = C.c_uint64()
    st = L.zk_snappy_uncompress(src.ctypes.data, len(data), None, 0, C.byref(n))
    if st != _abi.ZK_OK:
        raise _abi.ZkError(st, _abi.status_str(st))
    out = np.zeros(max(1, n.value), np.uint8)
    st = L.zk_snappy_uncompress(src.ctypes.data, len(data), out.ctypes.data, n.value, C.byref(n))
    if st != _abi.ZK_OK:
        raise _abi.ZkError(st, _abi.status_str(st))
    return out[: n.value].tobytes()


def _one_pass(indexed: bool, annotated: bool, binary: bool = False) -> None:
    if binary and not annotated:
        raise ValueError("binary=True needs annotated=True: the binary rows come from the rows pass (no binary-only call)")
    if indexed and annotated:
        raise ValueError("annotated=True with indexed=True: no call runs the index pass and the rows pass together")


class DeviceSpanDecoder:
    """zk_ingest_dev: stored fragments already in HBM -> device columns (one lane per fragment).

    `decode_device(buf, offsets, n)` takes torch tensors (uint8 bytes, int64 offsets[n+1]) on the
    device; `decode(blobs)` uploads a list of bytes objects first (tests, small batches).

    max_span_names > 0 (at most 65535) makes a decoder that also keeps a span-name dictionary in HBM
    (zk_ingest_dev_create_names): the decode calls then take span_names=True and write every
    record's name id (id + 1; 0 for "" and "Unknown") into bits 16..31 of flags. Its ids follow
    hash-table slot order, not the host decoder's first-appearance order: compare through
    span_name(i). With 0 (the default) span_names=True raises ZK_ERR_UNSUPPORTED."""

    def __init__(self, max_services: int = 4096, *, max_span_names: int = 0, device: int = 0,
                 stream: int | None = None, scratch_bytes: int = 0):
        self._L = _abi.lib()
        h = C.c_void_p()
        if max_span_names:
            st = self._L.zk_ingest_dev_create_names(device, stream, max_services, max_span_names, C.byref(h))
        else:
            st = self._L.zk_ingest_dev_create(device, stream, max_services, C.byref(h))
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, _abi.status_str(st))
        self._h = h
        self.device = device
        self.max_services = max_services
        self.max_span_names = max_span_names
        if scratch_bytes:  # the Snappy scratch's first size (zk_ingest_dev_set_scratch); it grows on demand
            st = self._L.zk_ingest_dev_set_scratch(self._h, scratch_bytes)
            if st != _abi.ZK_OK:
                raise _abi.ZkError(st, _abi.status_str(st))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.zk_ingest_dev_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int) -> None:
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_ingest_dev_last_error(self._h).decode() or _abi.status_str(st))

    def decode_device(self, buf, offsets, n: int, *, snappy: bool = True, strict: bool = True, out=None,
                      items: bool = False, item_cap: int | None = None, span_names: bool = False,
                      indexed: bool = False, client_rule: bool = True, index_cap: int | None = None,
                      annotated: bool = False, row_cap: int | None = None, row_strings: bool = True,
                      binary: bool = False, binary_cap: int | None = None):
        """-> (DeviceColumns with .n = records written, rejected), or with items=True
        (cols, rejected, (kv_service, kv_key), (ann_service, ann_value)): the span indexer's items as
        device tensors (int32 service ids of this decoder, int64 hashes = uint64 bit patterns), in no
        particular order within the batch (zk_ingest_dev_spans_items). item_cap: the items per kind
        to allow for (default 2n + 16; a batch with more is decoded again with 4x the room).
        span_names: ZK_INGEST_SPAN_NAMES (a decoder made with max_span_names > 0).
        indexed=True (zk_ingest_dev_spans_indexed) appends the annotation index's entries, an
        annindex.DeviceAnnotationItems in the host decoder's order, to the result: (cols, rejected,
        entries), or after the two item pairs with items=True. client_rule=False emits the entries of
        a client-side span of the service "client" too (ZK_INGEST_NO_CLIENT_RULE). index_cap: the
        entries to allow for (default 8 per fragment, at least 16; a batch with more is decoded again
        with 4x the room).
        annotated=True (zk_ingest_dev_spans_annotated) appends the annotation store's rows, an
        annotstore.DeviceAnnotationRows in the host decoder's order, to the result: (cols, rejected,
        rows), or after the two item pairs with items=True. row_cap: the rows to allow for (default 8
        per fragment, at least 16; a batch with more is decoded again with 4x the room).
        row_strings=False (ZK_INGEST_NO_ROW_STRINGS) leaves the rows' value strings uncaptured: the
        rows are the same, string() does not learn them. annotated and indexed together are a
        ValueError: no C call runs both passes.
        binary=True with annotated=True (zk_ingest_dev_spans_annotated_binary) appends, behind the rows, the
        binary-annotation store's rows, a binannotstore.DeviceBinaryAnnotationRows in the host decoder's
        order, from the same rows pass. binary_cap: the binary rows to allow for (default 8 per fragment, at
        least 16; a batch with more is decoded again with 4x the room). row_strings covers keys and values
        too. binary=True without annotated=True is a ValueError."""
        _one_pass(indexed, annotated, binary)
        L, h = self._L, self._h
        bp, op = buf.data_ptr(), offsets.data_ptr()

        def call(codec, flags, ab, nout, nrej, it, ix=None, an=None, bn=None):
            if bn is not None:
                return L.zk_ingest_dev_spans_annotated_binary(h, bp, op, n, codec, flags, C.byref(ab), C.byref(nout),
                                                              C.byref(nrej), None if it is None else C.byref(it),
                                                              C.byref(an), C.byref(bn))
            if an is not None:
                return L.zk_ingest_dev_spans_annotated(h, bp, op, n, codec, flags, C.byref(ab), C.byref(nout), C.byref(nrej),
                                                       None if it is None else C.byref(it), C.byref(an))
            if ix is not None:
                return L.zk_ingest_dev_spans_indexed(h, bp, op, n, codec, flags, C.byref(ab), C.byref(nout), C.byref(nrej),
                                                     None if it is None else C.byref(it), C.byref(ix))
            if it is None:
                return L.zk_ingest_dev_spans(h, bp, op, n, codec, flags, C.byref(ab), C.byref(nout), C.byref(nrej))
            return L.zk_ingest_dev_spans_items(h, bp, op, n, codec, flags, C.byref(ab), C.byref(nout), C.byref(nrej),
                                               C.byref(it))

        return self._run(call, n, snappy, strict, out, items, item_cap, span_names, indexed, client_rule, index_cap,
                         annotated, row_cap, row_strings, binary, binary_cap)

    def decode_device_many(self, batches, *, snappy: bool = True, strict: bool = True, out=None,
                           items: bool = False, item_cap: int | None = None, span_names: bool = False,
                           indexed: bool = False, client_rule: bool = True, index_cap: int | None = None,
                           annotated: bool = False, row_cap: int | None = None, row_strings: bool = True,
                           binary: bool = False, binary_cap: int | None = None):
        """Several HBM-resident batches [(buf, offsets, n), ...] in ONE decode
        (zk_ingest_dev_spans_multi, zk_ingest_dev_spans_multi_indexed with indexed=True, or
        zk_ingest_dev_spans_multi_annotated with annotated=True): the results of decode_device over
        the batches joined in order, for one set of launches and one host round trip. binary=True:
        zk_ingest_dev_spans_multi_annotated_binary."""
        _one_pass(indexed, annotated, binary)
        L, h = self._L, self._h
        nb = len(batches)
        n = sum(int(b[2]) for b in batches)
        bufs = (C.c_void_p * max(1, nb))(*[b[0].data_ptr() if int(b[2]) else None for b in batches])
        offs = (C.c_void_p * max(1, nb))(*[b[1].data_ptr() if int(b[2]) else None for b in batches])
        ns = (C.c_uint64 * max(1, nb))(*[int(b[2]) for b in batches])

        def call(codec, flags, ab, nout, nrej, it, ix=None, an=None, bn=None):
            if bn is not None:
                return L.zk_ingest_dev_spans_multi_annotated_binary(h, nb, bufs, offs, ns, codec, flags, C.byref(ab), C.byref(nout),
                                                                    C.byref(nrej), None if it is None else C.byref(it),
                                                                    C.byref(an), C.byref(bn))
            if an is not None:
                return L.zk_ingest_dev_spans_multi_annotated(h, nb, bufs, offs, ns, codec, flags, C.byref(ab), C.byref(nout),
                                                             C.byref(nrej), None if it is None else C.byref(it), C.byref(an))
            if ix is not None:
                return L.zk_ingest_dev_spans_multi_indexed(h, nb, bufs, offs, ns, codec, flags, C.byref(ab), C.byref(nout),
                                                           C.byref(nrej), None if it is None else C.byref(it), C.byref(ix))
            return L.zk_ingest_dev_spans_multi(h, nb, bufs, offs, ns, codec, flags, C.byref(ab), C.byref(nout),
                                               C.byref(nrej), None if it is None else C.byref(it))

        return self._run(call, n, snappy, strict, out, items, item_cap, span_names, indexed, client_rule, index_cap,
                         annotated, row_cap, row_strings, binary, binary_cap)

    def _run(self, call, n, snappy, strict, out, items, item_cap, span_names=False, indexed=False, client_rule=True,
             index_cap=None, annotated=False, row_cap=None, row_strings=True, binary=False, binary_cap=None):
        import torch

        from .columns import DeviceColumns

        dev = f"cuda:{self.device}"
        cols = out if out is not None else DeviceColumns(max(1, n), device=dev)
        nout, nrej = C.c_uint64(), C.c_uint64()
        ab = cols.abi(n)
        codec = _abi.ZK_CODEC_SNAPPY_THRIFT if snappy else _abi.ZK_CODEC_THRIFT
        flags = (_abi.ZK_INGEST_STRICT if strict else 0) | (_abi.ZK_INGEST_SPAN_NAMES if span_names else 0)
        if indexed and not client_rule:
            flags |= _abi.ZK_INGEST_NO_CLIENT_RULE
        if annotated and not row_strings:
            flags |= _abi.ZK_INGEST_NO_ROW_STRINGS
        if not items and not indexed and not annotated:
            self._check(call(codec, flags, ab, nout, nrej, None))
            cols.n = int(nout.value)
            return cols, int(nrej.value)
        cap = item_cap if item_cap is not None else 2 * n + 16
        icap = int(index_cap) if index_cap is not None else max(16, 8 * n)
        rcap = int(row_cap) if row_cap is not None else max(16, 8 * n)
        bcap = int(binary_cap) if binary_cap is not None else max(16, 8 * n)
        it = ix = an = bn = None
        while True:
            if items:
                ks = torch.empty(cap, dtype=torch.int32, device=dev)
                kh = torch.empty(cap, dtype=torch.int64, device=dev)
                as_ = torch.empty(cap, dtype=torch.int32, device=dev)
                ah = torch.empty(cap, dtype=torch.int64, device=dev)
                it = _abi.zk_ingest_items(ks.data_ptr(), kh.data_ptr(), cap, 0, as_.data_ptr(), ah.data_ptr(), cap, 0)
            if indexed:
                # (fresh tensors per decode: an index that observed the last ones may still read them)
                ent = [torch.empty(max(1, icap), dtype=torch.int32 if k == 0 else torch.int64, device=dev) for k in range(5)]
                ix = _abi.zk_ingest_index_items(*[t.data_ptr() for t in ent], icap, 0)
                st = call(codec, flags, ab, nout, nrej, it, ix)
            elif annotated:
                # (fresh tensors per decode: a store that observed the last ones may still read them)
                row = [torch.empty(max(1, rcap), dtype=torch.int64 if k < 4 else torch.int32, device=dev) for k in range(7)]
                an = _abi.zk_ingest_annotation_rows(*[t.data_ptr() for t in row], rcap, 0)
                if binary:
                    brow = [torch.empty(max(1, bcap), dtype=torch.int64 if k < 4 else torch.int32, device=dev) for k in range(7)]
                    bn = _abi.zk_ingest_binary_rows(*[t.data_ptr() for t in brow], bcap, 0)
                st = call(codec, flags, ab, nout, nrej, it, None, an, bn)
            else:
                st = call(codec, flags, ab, nout, nrej, it)
            if st == _abi.ZK_ERR_CAPACITY:
                grow_items = items and (it.kv_n == cap or it.ann_n == cap)
                grow_index = indexed and ix.n == icap
                grow_rows = annotated and an.n == rcap
                grow_brows = binary and bn.n == bcap
                if grow_items or grow_index or grow_rows or grow_brows:  # more items / entries / rows than guessed: the batch again
                    bcap = max(16, bcap * 4) if grow_brows else bcap
                    cap = cap * 4 if grow_items else cap
                    icap = max(16, icap * 4) if grow_index else icap
                    rcap = max(16, rcap * 4) if grow_rows else rcap
                    continue
            self._check(st)
            break
        cols.n = int(nout.value)
        res = (cols, int(nrej.value))
        if items:
            res += ((ks[: it.kv_n], kh[: it.kv_n]), (as_[: it.ann_n], ah[: it.ann_n]))
        if indexed:
            from .annindex import DeviceAnnotationItems

            res += (DeviceAnnotationItems(*[t[: ix.n] for t in ent]),)
        if annotated:
            from .annotstore import DeviceAnnotationRows

            res += (DeviceAnnotationRows(*[t[: an.n] for t in row]),)
        if binary:
            from .binannotstore import DeviceBinaryAnnotationRows

            res += (DeviceBinaryAnnotationRows(*[t[: bn.n] for t in brow]),)
        return res

    def index_stats(self) -> dict:
        """{"pass_ms", "slices"} of the last indexed decode's index pass (zk_ingest_dev_index_stats)."""
        ms, sl = C.c_double(), C.c_uint64()
        self._check(self._L.zk_ingest_dev_index_stats(self._h, C.byref(ms), C.byref(sl)))
        return {"pass_ms": float(ms.value), "slices": int(sl.value)}

    def rows_stats(self) -> dict:
        """{"pass_ms", "slices"} of the last annotated decode's rows pass (zk_ingest_dev_rows_stats)."""
        ms, sl = C.c_double(), C.c_uint64()
        self._check(self._L.zk_ingest_dev_rows_stats(self._h, C.byref(ms), C.byref(sl)))
        return {"pass_ms": float(ms.value), "slices": int(sl.value)}

    def string(self, h: int) -> str:
        """The key / value string behind a hash an items batch has seen, or behind the value of a row
        an annotated decode wrote with row_strings=True (zk_ingest_dev_string);
        memoised (a hash keeps the string first captured for it)."""
        h = int(h) & 0xFFFFFFFFFFFFFFFF
        memo = self.__dict__.setdefault("_strings", {})
        if h in memo:
            return memo[h]
        ln = C.c_uint64()
        self._check(self._L.zk_ingest_dev_string(self._h, h, None, 0, C.byref(ln)))
        buf = C.create_string_buffer(max(1, ln.value))
        self._check(self._L.zk_ingest_dev_string(self._h, h, buf, ln.value, C.byref(ln)))
        v = buf.raw[: ln.value].decode("utf-8", "surrogateescape")
        memo[h] = v
        return v

    def bytes(self, h: int) -> bytes:
        """The bytes behind a hash, with their length: string() without the decoding (a binary annotation's
        value may hold NUL and bytes that are no UTF-8)."""
        h = int(h) & 0xFFFFFFFFFFFFFFFF
        ln = C.c_uint64()
        self._check(self._L.zk_ingest_dev_string(self._h, h, None, 0, C.byref(ln)))
        buf = C.create_string_buffer(max(1, ln.value))
        self._check(self._L.zk_ingest_dev_string(self._h, h, buf, ln.value, C.byref(ln)))
        return buf.raw[: ln.value]

    def decode(self, blobs: Sequence[bytes], *, snappy: bool = True, strict: bool = True, items: bool = False,
               span_names: bool = False, indexed: bool = False, client_rule: bool = True,
               index_cap: int | None = None, annotated: bool = False, row_cap: int | None = None,
               row_strings: bool = True, binary: bool = False, binary_cap: int | None = None):
        _one_pass(indexed, annotated, binary)
        import torch

        dev = f"cuda:{self.device}"
        offsets = np.zeros(len(blobs) + 1, np.int64)
        if blobs:
            offsets[1:] = np.cumsum([len(b) for b in blobs])
        raw = np.frombuffer(b"".join(blobs) or b"\0", dtype=np.uint8)
        buf = torch.from_numpy(raw.copy()).to(dev)
        off = torch.from_numpy(offsets).to(dev)
        return self.decode_device(buf, off, len(blobs), snappy=snappy, strict=strict, items=items,
                                  span_names=span_names, indexed=indexed, client_rule=client_rule, index_cap=index_cap,
                                  annotated=annotated, row_cap=row_cap, row_strings=row_strings, binary=binary,
                                  binary_cap=binary_cap)

    @property
    def num_services(self) -> int:
        n = C.c_uint32()
        self._check(self._L.zk_ingest_dev_num_services(self._h, C.byref(n)))
        return int(n.value)

    def service_name(self, i: int) -> str:
        """Memoised: a decoder's service ids never change."""
        memo = self.__dict__.setdefault("_names", {})
        if i in memo:
            return memo[i]
        ln = C.c_uint64()
        self._check(self._L.zk_ingest_dev_service_name(self._h, i, None, 0, C.byref(ln)))
        buf = C.create_string_buffer(max(1, ln.value))
        self._check(self._L.zk_ingest_dev_service_name(self._h, i, buf, ln.value, C.byref(ln)))
        v = buf.raw[: ln.value].decode("utf-8", "surrogateescape")
        memo[i] = v
        return v

    def service_names(self) -> List[str]:
        return [self.service_name(i) for i in range(self.num_services)]

    @property
    def num_span_names(self) -> int:
        n = C.c_uint32()
        self._check(self._L.zk_ingest_dev_num_span_names(self._h, C.byref(n)))
        return int(n.value)

    def span_name(self, i: int) -> str:
        """Memoised: a span name keeps its id for the decoder's life. A record's flags carry id + 1."""
        memo = self.__dict__.setdefault("_span_names", {})
        if i in memo:
            return memo[i]
        ln = C.c_uint64()
        self._check(self._L.zk_ingest_dev_span_name(self._h, i, None, 0, C.byref(ln)))
        buf = C.create_string_buffer(max(1, ln.value))
        self._check(self._L.zk_ingest_dev_span_name(self._h, i, buf, ln.value, C.byref(ln)))
        v = buf.raw[: ln.value].decode("utf-8", "surrogateescape")
        memo[i] = v
        return v

    def span_names(self) -> List[str]:
        return [self.span_name(i) for i in range(self.num_span_names)]
