"""A reader of TBinaryProtocol Spans that shares nothing with the decoders of include/zkingest.h.

Test infrastructure only (pure Python, host only). The host decoder (zk_ingest.cpp read_span) and the
device walks (zk_ingest_dev.hip) read and interpret in one pass; this reader first parses the bytes
into a generic value tree (read_value: what the Thrift wire format says the bytes are, whatever the
field ids mean) and only then interprets the tree as a Span, by the contract of include/zkingest.h
("Wire forms"):

  * a known field is a (field id, wire type) pair; a known id with another type is an unknown field
  * the last occurrence of a scalar field wins; parent_id stays set once seen
  * every field-6 / field-8 list of structs is APPENDED to what earlier lists gave; such a list with
    another element type is an unknown field
  * within an annotation, every host struct marks the host present; the service name is the last
    service_name string of any of them (a second host without one keeps the first's)
  * within an endpoint the last service_name wins; absent or empty means "Unknown service name"
  * bytes after the Span's STOP are ignored
  * a negative string length or container count, a value of an unknown type code and a short read
    make the bytes undecodable (a container of zero elements never reads its element type)
  * validation (thrift.scala) applies to decodable bytes only, in this order: no name; then per
    annotation in order, timestamp <= 0 (an absent timestamp is 0), then a present, empty value
  * an absent annotation value is not invalid

decode(raw) returns ("ok", Span, extras), ("invalid", why) or ("undecodable",). The reader has no
nesting limit: extras["skip_depth"] is the largest number of containers (struct, map, set, list) open
at once inside any one unknown field's value, which is what the decoders' limits count.

The Span is an oracle.spans.Span. Two forms its dataclasses cannot hold are stored as None and
resolved here: an annotation without a value field (Annotation.value None) and a binary annotation
without a key (BinaryAnnotation.key None). Both decoders hash such a string as "" for the indexer
items, and neither is a core annotation: items() maps None to "" after the span-level oracle ran
(validation has already rejected every present-and-empty annotation value, so "" is unambiguous
there). Strings are decoded as the Python wrapper decodes them (UTF-8, surrogateescape)."""
from __future__ import annotations

import struct
from collections import Counter
from typing import List, NamedTuple, Optional, Tuple

from oracle.spans import UNKNOWN_SERVICE_NAME, Annotation, BinaryAnnotation, Endpoint, Span

BOOL, BYTE, DOUBLE, I16, I32, I64, STRING, STRUCT, MAP, SET, LIST = 2, 3, 4, 6, 8, 10, 11, 12, 13, 14, 15
FIXED = {BOOL: ">b", BYTE: ">b", I16: ">h", I32: ">i", I64: ">q"}

UNDECODABLE = "undecodable thrift span"
NO_NAME = "No name set in Span"
NO_TIMESTAMP = "Annotation must have a timestamp"
NO_VALUE = "Annotation must have a value"


class Undecodable(Exception):
    pass


class Struct(NamedTuple):
    fields: list  # [(field id, wire type, value)] in wire order


class Seq(NamedTuple):  # a list or a set
    etype: int
    items: list


class Map(NamedTuple):
    ktype: int
    vtype: int
    items: list  # [(key, value)]


class _Bytes:
    def __init__(self, data: bytes):
        self.data, self.at = data, 0

    def take(self, n: int) -> bytes:
        if n < 0 or self.at + n > len(self.data):
            raise Undecodable("short read")
        self.at += n
        return self.data[self.at - n:self.at]

    def num(self, fmt: str) -> int:
        return struct.unpack(fmt, self.take(struct.calcsize(fmt)))[0]


def read_value(b: _Bytes, t: int):
    """one value of wire type t as a nested Python object"""
    if t in FIXED:
        return b.num(FIXED[t])
    if t == DOUBLE:
        return b.take(8)
    if t == STRING:
        n = b.num(">i")
        if n < 0:
            raise Undecodable("negative string length")
        return b.take(n)
    if t == STRUCT:
        fields = []
        while True:
            ft = b.num(">B")
            if ft == 0:
                return Struct(fields)
            fid = b.num(">h")
            fields.append((fid, ft, read_value(b, ft)))
    if t in (LIST, SET):
        et, n = b.num(">B"), b.num(">i")
        if n < 0:
            raise Undecodable("negative count")
        return Seq(et, [read_value(b, et) for _ in range(n)])
    if t == MAP:
        kt, vt, n = b.num(">B"), b.num(">B"), b.num(">i")
        if n < 0:
            raise Undecodable("negative count")
        items = []
        for _ in range(n):  # (a hostile count ends at the first short read)
            k = read_value(b, kt)
            items.append((k, read_value(b, vt)))
        return Map(kt, vt, items)
    raise Undecodable("type code %d" % t)


def containers(v) -> int:
    """the number of containers open at once at the deepest point of v"""
    if isinstance(v, Struct):
        return 1 + max([containers(x) for _, _, x in v.fields], default=0)
    if isinstance(v, Seq):
        return 1 + max([containers(x) for x in v.items], default=0)
    if isinstance(v, Map):
        return 1 + max([max(containers(k), containers(x)) for k, x in v.items], default=0)
    return 0


def _text(b: bytes) -> str:
    return b.decode("utf-8", "surrogateescape")


class _Interp:
    def __init__(self):
        self.skip_depth = 0
        self.unknown = 0

    def skipped(self, v):
        self.unknown += 1
        self.skip_depth = max(self.skip_depth, containers(v))

    def endpoint(self, s: Struct, name: Optional[bytes]) -> Optional[bytes]:
        """the raw service name after this endpoint struct, given the one before it"""
        for fid, t, v in s.fields:
            if (fid, t) == (3, STRING):
                name = v
            else:
                self.skipped(v)
        return name

    def annotation(self, s: Struct) -> Annotation:
        ts, value, host, name = 0, None, False, None
        for fid, t, v in s.fields:
            if (fid, t) == (1, I64):
                ts = v
            elif (fid, t) == (2, STRING):
                value = v
            elif (fid, t) == (3, STRUCT):
                host, name = True, self.endpoint(v, name)
            else:
                self.skipped(v)
        return Annotation(ts, None if value is None else _text(value), _host(name) if host else None)

    def binary_annotation(self, s: Struct) -> BinaryAnnotation:
        key, host, name = None, False, None
        for fid, t, v in s.fields:
            if (fid, t) == (1, STRING):
                key = v
            elif (fid, t) == (4, STRUCT):
                host, name = True, self.endpoint(v, name)
            else:
                self.skipped(v)
        return BinaryAnnotation(None if key is None else _text(key), b"", "BYTES", _host(name) if host else None)

    def span(self, s: Struct):
        trace_id = span_id = 0
        parent = name = None
        anns: List[Annotation] = []
        bins: List[BinaryAnnotation] = []
        for fid, t, v in s.fields:
            if (fid, t) == (1, I64):
                trace_id = v
            elif (fid, t) == (3, STRING):
                name = v
            elif (fid, t) == (4, I64):
                span_id = v
            elif (fid, t) == (5, I64):
                parent = v
            elif fid in (6, 8) and t == LIST and v.etype == STRUCT:
                if fid == 6:
                    anns += [self.annotation(x) for x in v.items]
                else:
                    bins += [self.binary_annotation(x) for x in v.items]
            else:
                self.skipped(v)
        return trace_id, name, span_id, parent, tuple(anns), tuple(bins)


def _host(name: Optional[bytes]) -> Endpoint:
    # ipv4 and port reach neither the record nor the items
    return Endpoint(0, 0, _text(name) if name else UNKNOWN_SERVICE_NAME)


def decode(raw: bytes):
    b = _Bytes(raw)
    try:
        tree = read_value(b, STRUCT)
    except Undecodable:
        return ("undecodable",)
    it = _Interp()
    trace_id, name, span_id, parent, anns, bins = it.span(tree)
    if name is None:
        return ("invalid", NO_NAME)
    for a in anns:
        if a.timestamp <= 0:
            return ("invalid", NO_TIMESTAMP)
        if a.value == "":
            return ("invalid", NO_VALUE)
    extras = {"trailing": len(raw) - b.at, "unknown_fields": it.unknown, "skip_depth": it.skip_depth}
    return ("ok", Span(trace_id, _text(name), span_id, parent, anns, bins), extras)


def why(result) -> Optional[str]:
    """the decoders' strict-mode message for a result, None for an accepted span"""
    if result[0] == "invalid":
        return result[1]
    return None if result[0] == "ok" else UNDECODABLE


def comparable(span: Span) -> Span:
    """a constructed Span as decode() would return it: what neither record nor items see is dropped"""
    anns = tuple(Annotation(a.timestamp, a.value, None if a.host is None else _host(a.host.service_name.encode()))
                 for a in span.annotations)
    bins = tuple(BinaryAnnotation(b.key, b"", "BYTES", None if b.host is None else _host(b.host.service_name.encode()))
                 for b in span.binary_annotations)
    return Span(span.trace_id, span.name, span.id, span.parent_id, anns, bins)


def items(spans, expected_items) -> Tuple[Counter, Counter]:
    """expected_items (tests/test_ingest.py) of decoded spans, an absent value or key as the empty
    string (an absent and an empty key give the same item, so counts add)"""
    out = []
    for c in expected_items(spans):
        fixed: Counter = Counter()
        for (s, x), n in c.items():
            fixed[(s, "" if x is None else x)] += n
        out.append(fixed)
    return out[0], out[1]
