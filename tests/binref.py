"""Binary annotations for the tests of the binary-annotation rows (zkbinannots.h, zk_ingest_spans_annotated_binary):
a small generator over oracle.spans, an encoder that can write the wire forms tests/thriftenc.py cannot, and the
Python restatement of the rows both decoders must emit.

A fragment is an oracle.spans Span whose binary_annotations hold oracle BinaryAnnotations with a WIDER reading
of their fields, so that every wire form has a model:
  key              str / bytes, or None: no field 1
  value            bytes, or None: no field 2
  annotation_type  a name of thriftenc.ANNOTATION_TYPES, an int (written as the i32 it is, in range or not),
                   None (no field 3), ("i16", v) / ("i64", v) / ("str", b) (field 3 as ANOTHER wire type), or a
                   list of these (several occurrences, in order)
  host             None, an oracle Endpoint (one struct: ipv4, port, and the name unless it is None), or a
                   tuple of HostPart (one struct each, only the given fields written)
and `split`, where a second field-8 list begins (None: one list).
"""
from __future__ import annotations

import random
import struct
from typing import List, NamedTuple, Optional, Sequence

from oracle.spans import UNKNOWN_SERVICE_NAME, Annotation, BinaryAnnotation, Endpoint, Span
from tests import thriftenc as T
from zipkin_amd.ingest import hash_string

M64 = 2 ** 64 - 1


class HostPart(NamedTuple):
    """One host struct of a binary annotation: only the fields that are not None are written."""
    ipv4: Optional[int] = None
    port: Optional[int] = None
    name: Optional[str] = None


class Frag(NamedTuple):
    span: Span
    split: Optional[int] = None  # binary_annotations[split:] go into a second field-8 list


VALUE_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 3000)
HOST_NAMES = ("web", "db", "Cache", "client", "", None, "a-rather-long-service-name-beyond-sixteen-bytes")


# ---- the encoder -------------------------------------------------------------------------------------------
def _host_struct(h) -> bytes:
    if isinstance(h, Endpoint):
        return T.endpoint(h)
    out = b""
    if h.ipv4 is not None:
        out += T._fh(T.T_I32, 1) + struct.pack(">i", ((h.ipv4 + 2 ** 31) % 2 ** 32) - 2 ** 31)
    if h.port is not None:
        out += T._fh(T.T_I16, 2) + struct.pack(">h", ((h.port + 2 ** 15) % 2 ** 16) - 2 ** 15)
    if h.name is not None:
        out += T._fh(T.T_STRING, 3) + T._str(h.name)
    return out + b"\0"


def _type_field(t) -> bytes:
    if t is None:
        return b""
    if isinstance(t, list):
        return b"".join(_type_field(x) for x in t)
    if isinstance(t, str):
        t = T.ANNOTATION_TYPES[t]
    if isinstance(t, int):
        return T._fh(T.T_I32, 3) + struct.pack(">i", t)
    kind, v = t
    if kind == "i16":
        return T._fh(T.T_I16, 3) + struct.pack(">h", v)
    if kind == "i64":
        return T._fh(T.T_I64, 3) + T._i64(v)
    assert kind == "str"
    return T._fh(T.T_STRING, 3) + T._str(v)


def binary_annotation(b: BinaryAnnotation) -> bytes:
    out = b""
    if b.key is not None:
        out += T._fh(T.T_STRING, 1) + T._str(b.key)
    if b.value is not None:
        out += T._fh(T.T_STRING, 2) + T._str(b.value)
    out += _type_field(b.annotation_type)
    hosts = () if b.host is None else (b.host,) if isinstance(b.host, Endpoint) else tuple(b.host)
    for h in hosts:
        out += T._fh(T.T_STRUCT, 4) + _host_struct(h)
    return out + b"\0"


def _blist(bs: Sequence[BinaryAnnotation]) -> bytes:
    return T._fh(T.T_LIST, 8) + struct.pack(">bi", T.T_STRUCT, len(bs)) + b"".join(binary_annotation(b) for b in bs)


def encode(f: Frag) -> bytes:
    s = f.span
    out = T._fh(T.T_I64, 1) + T._i64(s.trace_id) + T._fh(T.T_STRING, 3) + T._str(s.name) + T._fh(T.T_I64, 4) + T._i64(s.id)
    if s.parent_id is not None:
        out += T._fh(T.T_I64, 5) + T._i64(s.parent_id)
    bs = list(s.binary_annotations)
    if f.split is not None:  # the first binary list BEFORE the time annotations, the second behind them
        out += _blist(bs[:f.split])
        bs = bs[f.split:]
    out += T._fh(T.T_LIST, 6) + struct.pack(">bi", T.T_STRUCT, len(s.annotations)) + b"".join(T.annotation(a) for a in s.annotations)
    out += _blist(bs)
    return out + T._fh(T.T_BOOL, 9) + b"\0\0"


def encode_all(frags: Sequence[Frag], snappy: bool = True) -> List[bytes]:
    return [T.snappy(encode(f)) if snappy else encode(f) for f in frags]


# ---- the restatement ---------------------------------------------------------------------------------------
def type_of(t) -> int:
    """The TYPE of a row: the last field 3 that is an i32; absent 0; outside 0..6 -> 7."""
    forms = t if isinstance(t, list) else [t]
    v = 0
    for x in forms:
        if isinstance(x, str):
            v = T.ANNOTATION_TYPES[x]
        elif isinstance(x, int):
            v = x
    return v if 0 <= v <= 6 else 7


def host_of(h):
    """(ipv4 u32, port u16, name) of a binary annotation's host structs folded in order, or None without one."""
    if h is None:
        return None
    parts = (HostPart(h.ipv4, h.port, h.service_name),) if isinstance(h, Endpoint) else tuple(h)
    ipv4 = port = 0
    name = None
    for p in parts:
        if isinstance(p, Endpoint):
            p = HostPart(p.ipv4, p.port, p.service_name)
        ipv4 = ipv4 if p.ipv4 is None else p.ipv4 & 0xFFFFFFFF
        port = port if p.port is None else p.port & 0xFFFF
        name = name if p.name is None else p.name
    return ipv4, port, name or UNKNOWN_SERVICE_NAME


def _bytes(x) -> bytes:
    return b"" if x is None else x.encode() if isinstance(x, str) else bytes(x)


def expected_binary_rows(spans) -> list:
    """One row per binary annotation of every span (Frag or Span), in order: (trace_id, span_id, key hash, value
    hash, ipv4, the host's service NAME or None, bits)."""
    out = []
    for s in spans:
        s = s.span if isinstance(s, Frag) else s
        for b in s.binary_annotations:
            bits, ipv4, name = type_of(b.annotation_type), 0, None
            h = host_of(b.host)
            if h is not None:
                ipv4, port, name = h
                bits |= 8 | (port << 16)
            out.append((s.trace_id & M64, s.id & M64, hash_string(_bytes(b.key)), hash_string(_bytes(b.value)), ipv4, name, bits))
    return out


def named_binary_rows(rows, names: Sequence[str]) -> list:
    """BinaryAnnotationRows with the service id replaced by its name (None without a host), for comparing
    decoders whose dictionaries number the services differently."""
    got = rows.rows()
    assert all(r[5] == 0 and r[4] == 0 and r[6] >> 16 == 0 for r in got if not r[6] & 8)
    assert all((r[6] >> 4) & 0xFFF == 0 for r in got)  # the reserved bits
    return [r[:5] + ((names[r[5]] if r[6] & 8 else None), r[6]) for r in got]


def strings_of(spans) -> dict:
    """hash -> bytes of every key and value."""
    out = {}
    for s in spans:
        s = s.span if isinstance(s, Frag) else s
        for b in s.binary_annotations:
            for x in (_bytes(b.key), _bytes(b.value)):
                out[hash_string(x)] = x
    return out


# ---- the generator -----------------------------------------------------------------------------------------
def _value(n: int, k: int) -> bytes:
    """n bytes that are a function of (n, k): NUL and non-UTF-8 bytes among them from length 7 up."""
    raw = bytes((37 * i + 11 * k + n) & 0xFF for i in range(n))
    return raw[:2] + b"\0\xff\xc3" + raw[5:] if n >= 7 else raw


def shapes(k: int) -> List[BinaryAnnotation]:
    """The catalogue, one list of binary annotations per k (mod its length): every type 0..6 and out-of-range
    ones, absent key / value / type / host, the value lengths, two host structs, field 3 as another wire type."""
    e = Endpoint(0x0A000001 + k % 5, 8000 + k % 3, HOST_NAMES[k % len(HOST_NAMES)] or "")
    n = VALUE_LENGTHS[k % len(VALUE_LENGTHS)]
    cat = [
        [BinaryAnnotation("http.uri", _value(n, k), "String", e)],
        [BinaryAnnotation("t%d" % t, _value(VALUE_LENGTHS[(k + t) % len(VALUE_LENGTHS)], t), t, e if t % 2 else None) for t in range(7)],
        [BinaryAnnotation("oor", b"x", 7, e), BinaryAnnotation("oor", b"x", -1, None), BinaryAnnotation("oor", b"x", 2 ** 31 - 1, e),
         BinaryAnnotation("oor", b"x", -2 ** 31, None)],
        [BinaryAnnotation(None, b"no key", "BYTES", e), BinaryAnnotation("no value", None, "I64", None),
         BinaryAnnotation("no type", b"\x01", None, e), BinaryAnnotation(None, None, None, None)],
        [BinaryAnnotation("two hosts", b"v", "I32", (HostPart(7, 8, "first"), HostPart(name="second"))),
         BinaryAnnotation("two hosts", b"v", "I32", (HostPart(7, 8, "first"), HostPart(ipv4=9))),
         BinaryAnnotation("two hosts", b"v", "I32", (HostPart(-1, -1, "first"), HostPart(port=1))),
         BinaryAnnotation("bare host", b"v", "I16", (HostPart(),)),
         BinaryAnnotation("empty name", b"v", "I16", (HostPart(1, 2, ""),))],
        [BinaryAnnotation("wrong wire type", b"v", ("i16", 6), e), BinaryAnnotation("wrong wire type", b"v", [5, ("i64", 3)], None),
         BinaryAnnotation("wrong wire type", b"v", [("str", b"6"), 4], e), BinaryAnnotation("last wins", b"v", [1, 2, 3], None)],
        [],  # time annotations only
        [BinaryAnnotation("sql.query", _value(n, k + 1), "String", e), BinaryAnnotation("sql.query", _value(n, k + 1), "String", e),
         BinaryAnnotation("", b"", "BOOL", None)],
    ]
    return cat[k % len(cat)]


def gen_frags(seed: int, n: int, traces: int = 0) -> List[Frag]:
    """n fragments: the catalogue's shapes in turn; every third fragment without time annotations, every
    fifth with its binary annotations in two field-8 lists; trace ids 0 and 2^64 - 1 among them."""
    rnd = random.Random(seed)
    traces = traces or max(1, n // 4)
    tids = [0, M64] + [rnd.getrandbits(64) for _ in range(traces)]
    out = []
    for k in range(n):
        tid = tids[k % len(tids)]
        e = Endpoint(rnd.getrandbits(32), rnd.getrandbits(16), rnd.choice(HOST_NAMES[:4]))
        anns = () if k % 3 == 2 else (Annotation(1000 + k, "sr", e), Annotation(1005 + k, "custom %d" % (k % 7), e if k % 2 else None),
                                      Annotation(1010 + k, "ss", e))
        bs = tuple(shapes(k + seed))
        split = len(bs) // 2 if k % 5 == 4 and len(bs) >= 2 else None
        out.append(Frag(Span(tid, "span %d" % (k % 11), rnd.getrandbits(64), rnd.getrandbits(64) if k % 4 else None, anns, bs), split))
    return out


def floors(frags: Sequence[Frag]) -> dict:
    """Counts that keep a case from passing vacuously."""
    rows = expected_binary_rows(frags)
    return {
        "rows": len(rows),
        "per_type": [sum(1 for r in rows if r[6] & 7 == t) for t in range(8)],
        "hostless": sum(1 for r in rows if not r[6] & 8),
        "binary_only": sum(1 for f in frags if f.span.binary_annotations and not f.span.annotations),
        "time_only": sum(1 for f in frags if f.span.annotations and not f.span.binary_annotations),
        "two_lists": sum(1 for f in frags if f.split is not None),
        "unknown_hosts": sum(1 for r in rows if r[5] == UNKNOWN_SERVICE_NAME),
    }
