"""Raw Snappy blocks written element by element from a plan, and a reference decoder of the format.

Test infrastructure only (pure Python, no project imports). The decoders of
include/zkingest.h are otherwise fed what one compressor (libsnappy, through pyarrow) happens to
emit; a plan fixes every element instead, so a test can ask for exactly the copy kind, length,
offset, literal length-field width and header padding it wants to see decoded.

The format (format_description.txt of Snappy): a varint of the uncompressed length (at most 5 bytes,
32 bits), then elements. The low two bits of an element's tag byte give its kind:
  0  literal: length - 1 in the upper six bits if below 60, else tags 60..63 announce 1..4 little-endian
     bytes holding length - 1; the literal's bytes follow
  1  copy, 1-byte offset: length - 4 in bits 2..4 (4..11), offset bits 8..10 in bits 5..7, low 8 bits next
  2  copy, 2-byte offset: length - 1 in the upper six bits (1..64), a little-endian 16-bit offset
  3  copy, 4-byte offset: as 2, with a little-endian 32-bit offset
A copy may overlap its own output (offset < length repeats the last `offset` bytes).

A plan is a Plan(elements, header_bytes): elements are tuples
  (LIT, length, width)     width 0 = the length in the tag, 1..4 = tags 60..63 (wider than needed is legal)
  (COPY1 | COPY2 | COPY4, length, offset)
and header_bytes pads the varint with zero continuation groups (0 = minimal).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Iterable, List, Optional, Sequence, Tuple

LIT, COPY1, COPY2, COPY4 = "lit", "copy1", "copy2", "copy4"
KINDS = (COPY1, COPY2, COPY4)
LEN_RANGE = {COPY1: (4, 11), COPY2: (1, 64), COPY4: (1, 64)}
MAX_OFFSET = {COPY1: 2047, COPY2: 65535, COPY4: 2**32 - 1}


class PlanError(ValueError):
    """The plan does not describe the data (or an element the format cannot express)."""


@dataclass
class Plan:
    elements: List[tuple] = field(default_factory=list)
    header_bytes: int = 0  # 0: the minimal varint; 2..5: padded to that many bytes

    def copies(self) -> List[tuple]:
        return [e for e in self.elements if e[0] != LIT]


# ---- element encoding ---------------------------------------------------------------------------
def header(n: int, nbytes: int = 0) -> bytes:
    """varint of n; nbytes > the minimal size appends continuation groups of zero bits"""
    if not 0 <= n < 2**32:
        raise PlanError("length %d does not fit the header" % n)
    out = []
    v = n
    while True:
        out.append(v & 0x7F)
        v >>= 7
        if not v:
            break
    if nbytes:
        if nbytes < len(out) or nbytes > 5:
            raise PlanError("a %d-byte header cannot hold %d" % (nbytes, n))
        out += [0] * (nbytes - len(out))
    return bytes([b | 0x80 for b in out[:-1]] + [out[-1]])


def min_width(length: int) -> int:
    """the narrowest literal length field that holds `length`"""
    if length <= 60:
        return 0
    w = 1
    while length - 1 >= 1 << (8 * w):
        w += 1
    return w


def element_bytes(el: tuple, data: bytes = b"") -> bytes:
    """One element's bytes (a literal's `data` included). Only what the format can express is checked,
    not whether the element fits any data: encode() does that."""
    kind, length, arg = el
    if kind == LIT:
        w = arg
        if not 0 <= w <= 4 or length < 1 or length > 2**32:
            raise PlanError("literal %r" % (el,))
        if w == 0:
            if length > 60:
                raise PlanError("literal of %d bytes needs a length field" % length)
            return bytes([(length - 1) << 2]) + data
        if length - 1 >= 1 << (8 * w):
            raise PlanError("literal of %d bytes does not fit %d length bytes" % (length, w))
        return bytes([(59 + w) << 2]) + (length - 1).to_bytes(w, "little") + data
    lo, hi = LEN_RANGE[kind]
    if not lo <= length <= hi or not 0 <= arg <= MAX_OFFSET[kind]:
        raise PlanError("copy %r" % (el,))
    if kind == COPY1:
        return bytes([((arg >> 8) << 5) | ((length - 4) << 2) | 1, arg & 0xFF])
    if kind == COPY2:
        return bytes([((length - 1) << 2) | 2]) + arg.to_bytes(2, "little")
    return bytes([((length - 1) << 2) | 3]) + arg.to_bytes(4, "little")


def element_size(el: tuple) -> int:
    kind, length, arg = el
    if kind == LIT:
        return 1 + arg + length
    return {COPY1: 2, COPY2: 3, COPY4: 5}[kind]


def plan_size(raw_len: int, plan: Plan) -> int:
    """the length of encode(raw, plan) without encoding"""
    return len(header(raw_len, plan.header_bytes)) + sum(element_size(e) for e in plan.elements)


def encode(raw: bytes, plan) -> bytes:
    """The stream the plan describes. Raises PlanError unless the elements, decoded in order, give
    exactly `raw`: every copy is checked against the bytes it must reproduce."""
    if not isinstance(plan, Plan):
        plan = Plan(list(plan))
    out = bytearray(header(len(raw), plan.header_bytes))
    o = 0
    for el in plan.elements:
        kind, length, arg = el
        if o + length > len(raw):
            raise PlanError("element %r at %d runs past the data (%d bytes)" % (el, o, len(raw)))
        if kind == LIT:
            out += element_bytes(el, raw[o:o + length])
        else:
            if arg < 1 or arg > o:
                raise PlanError("copy %r at %d reaches before the data" % (el, o))
            for k in range(length):
                if raw[o + k] != raw[o - arg + k]:
                    raise PlanError("copy %r at %d does not reproduce byte %d" % (el, o, o + k))
            out += element_bytes(el)
        o += length
    if o != len(raw):
        raise PlanError("the plan covers %d of %d bytes" % (o, len(raw)))
    return bytes(out)


# ---- plan builders ------------------------------------------------------------------------------
def literals(n: int, width: Optional[int] = None) -> List[tuple]:
    """n bytes as literals of the minimal (or the given) width; none for n == 0"""
    out = []
    while n > 0:
        c = min(n, 2**32)
        out.append((LIT, c, min_width(c) if width is None else width))
        n -= c
    return out


def match_length(raw: bytes, o: int, off: int, limit: int) -> int:
    m = 0
    while m < limit and raw[o + m] == raw[o - off + m]:
        m += 1
    return m


def greedy(raw: bytes, kind: str, offsets: Iterable[int], lengths: Tuple[int, int], start: int = 0,
           stop: Optional[int] = None, header_bytes: int = 0) -> Plan:
    """At every position in [start, stop) take the longest match among `offsets` (the first of equals)
    that `kind` can express within `lengths` = (min, max); literals elsewhere. Copies only of `kind`."""
    offsets = [d for d in offsets if 1 <= d <= MAX_OFFSET[kind]]
    lo = max(lengths[0], LEN_RANGE[kind][0])
    hi = min(lengths[1], LEN_RANGE[kind][1])
    stop = len(raw) if stop is None else stop
    els: List[tuple] = []
    o, pending = 0, 0
    while o < len(raw):
        if o >= stop:  # past the matcher's range: the rest is literal
            pending += len(raw) - o
            break
        best, boff = 0, 0
        if o >= start:
            for d in offsets:
                if d <= o:
                    m = match_length(raw, o, d, min(hi, len(raw) - o))
                    if m > best:
                        best, boff = m, d
        if best >= lo:
            els += literals(pending)
            pending = 0
            els.append((kind, best, boff))
            o += best
        else:
            pending += 1
            o += 1
    els += literals(pending)
    return Plan(els, header_bytes)


def copies_at(raw: bytes, pos: int, copies: Sequence[tuple], header_bytes: int = 0) -> Plan:
    """Literals up to `pos`, then the given copies back to back, the rest as literals."""
    els = literals(pos) + list(copies)
    done = pos + sum(c[1] for c in copies)
    return Plan(els + literals(len(raw) - done), header_bytes)


def literal_at(raw: bytes, pos: int, length: int, width: int) -> Plan:
    """Literals (minimal width) up to `pos`, one literal of `length` with a `width`-byte length field,
    the rest as literals."""
    return Plan(literals(pos) + [(LIT, length, width)] + literals(len(raw) - pos - length))


def run_then_literals(raw_len: int, run_start: int, run_len: int, k: int) -> Plan:
    """Copies first, literals last: a literal up to and including the run's first byte, the run's other
    bytes as offset-1 copies (64 at a time), then k single-byte literals, then the rest as one literal.
    After the run the output is far ahead of the input; the single-byte literals (2 bytes in, 1 out)
    eat into that lead."""
    els = literals(run_start + 1)
    left = run_len - 1
    while left > 0:
        c = min(64, left)
        els.append((COPY2, c, 1))
        left -= c
    els += [(LIT, 1, 0)] * k
    rest = raw_len - run_start - run_len - k
    if rest < 0:
        raise PlanError("%d bytes after the run cannot give %d single-byte literals" % (rest + k, k))
    return Plan(els + literals(rest))


# ---- the reference decoder ----------------------------------------------------------------------
def read_header(stream: bytes) -> Optional[Tuple[int, int]]:
    """(length, header bytes), or None: no terminating byte within 5, or a value past 32 bits"""
    v = 0
    for i in range(5):
        if i >= len(stream):
            return None
        b = stream[i]
        v |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            return (v, i + 1) if v < 2**32 else None
    return None


def decode(stream: bytes, max_fragment: Optional[int] = None, max_expansion: Optional[int] = None) -> Optional[bytes]:
    """The bytes the stream decodes to, or None for anything the format forbids: a bad or over-long
    varint, an element cut short at any byte, offset 0, an offset past the bytes produced so far,
    output past or short of the length in the header. With max_fragment / max_expansion also None
    when the header announces more than max_fragment bytes or more than max_expansion times the
    bytes after the header (the admission rules of include/zkingest.h)."""
    h = read_header(stream)
    if h is None:
        return None
    want, i = h
    n = len(stream)
    if max_fragment is not None and want > max_fragment:
        return None
    if max_expansion is not None and want > (n - i) * max_expansion:
        return None
    out = bytearray()
    while i < n:
        tag = stream[i]
        i += 1
        kind = tag & 3
        if kind == 0:
            length = tag >> 2
            if length >= 60:
                nb = length - 59
                if i + nb > n:
                    return None
                length = 0
                for k in range(nb):
                    length |= stream[i + k] << (8 * k)
                i += nb
            length += 1
            if i + length > n or len(out) + length > want:
                return None
            for k in range(length):
                out.append(stream[i + k])
            i += length
            continue
        if kind == 1:
            if i + 1 > n:
                return None
            length = ((tag >> 2) & 7) + 4
            off = ((tag >> 5) << 8) | stream[i]
            i += 1
        elif kind == 2:
            if i + 2 > n:
                return None
            length = (tag >> 2) + 1
            off = stream[i] | (stream[i + 1] << 8)
            i += 2
        else:
            if i + 4 > n:
                return None
            length = (tag >> 2) + 1
            off = stream[i] | (stream[i + 1] << 8) | (stream[i + 2] << 16) | (stream[i + 3] << 24)
            i += 4
        if off == 0 or off > len(out) or len(out) + length > want:
            return None
        for k in range(length):
            out.append(out[len(out) - off])
    return bytes(out) if len(out) == want else None


def elements_of(stream: bytes) -> List[tuple]:
    """The elements of a VALID stream as plan tuples (for coverage tables): what the bytes say, which
    is what a decoder sees, whatever the builder meant to write."""
    _, i = read_header(stream)
    els = []
    while i < len(stream):
        tag = stream[i]
        kind = tag & 3
        if kind == 0:
            length, w = tag >> 2, 0
            if length >= 60:
                w = length - 59
                length = int.from_bytes(stream[i + 1:i + 1 + w], "little")
            length += 1
            els.append((LIT, length, w))
            i += 1 + w + length
        elif kind == 1:
            els.append((COPY1, ((tag >> 2) & 7) + 4, ((tag >> 5) << 8) | stream[i + 1]))
            i += 2
        elif kind == 2:
            els.append((COPY2, (tag >> 2) + 1, int.from_bytes(stream[i + 1:i + 3], "little")))
            i += 3
        else:
            els.append((COPY4, (tag >> 2) + 1, int.from_bytes(stream[i + 1:i + 5], "little")))
            i += 5
    return els
