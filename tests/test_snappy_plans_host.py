"""Snappy element conformance, host side: hand-planned streams (tests/snappyplan.py) through the
reference decoder, libsnappy and the host decoder of include/zkingest.h.

libsnappy (through pyarrow) writes only short literals, long literals with a 1- or 2-byte length and
copies with 1- or 2-byte offsets at whatever offsets its hash table finds. The case families below
fix every element instead:
  A  every copy kind x length x offset in {1..17, 31, 32, 33, 255, 256, 2047, 2048}, copies ending on the
     Span's last byte, copies right after the header (o == offset)
  B  literal lengths around every width of the length field, minimal and every wider field up to 4 bytes
  C  copies first, literals last: the output's final lead over the input takes every value in 0..128
     (the in-place safety boundary of the device's LDS decoder), at all 16 input alignments
  D  incompressible Spans stepping by 1 across the device's region-size thresholds (640 and 20480 bytes)
  E  the elements of A and B behind 21000 bytes of padding (the device's global-memory decoder), with
     offsets 65535, 65536 and 70000 and a 66000-byte literal under a 3- and a 4-byte length
  F  padded header varints, the densest legal stream (21.3-fold, under the 22-fold admission bound), raw = 0
  G  one valid stream broken in each way the format forbids (rejection), among them a high byte set in a
     3- or 4-byte literal length: in a fragment that fits the LDS decoder those bytes are 0 in every
     valid stream, so only a rejection shows that the decoder reads them
Each valid case is (id, Span, stream, payload): the stream decodes to thriftenc.span(Span), and the
payload string sits where a decoder gives strings back (a non-core annotation value or a
binary-annotation key with a host, the service name, the span name). Ids and timestamps are built from
the payload's repeating unit, so a miscopy changes the record as well as the string. The expectation
(expected_records / expected_items of tests/test_ingest.py) never passes through Snappy code.
tests/test_gpu_snappy_plans.py runs the same cases through the device decoder."""
import functools
import random
import re
import string
from collections import Counter
from pathlib import Path
from typing import NamedTuple, Optional

import pytest

from oracle.spans import Annotation, BinaryAnnotation, Endpoint, Span
from tests import snappyplan as P
from tests import thriftenc as T
from tests.test_ingest import expected_items, expected_records, records
from zipkin_amd import ZkError, _abi
from zipkin_amd.ingest import SpanDecoder, hash_string, snappy_uncompress

ROOT = Path(__file__).resolve().parent.parent


def _abi_const(name: str) -> int:
    """an admission constant of include/zkingest.h: from _abi when exported there, else from the header"""
    v = getattr(_abi, name, None)
    if v is None:
        m = re.search(r"#define\s+%s\s+\(?\s*(\d+)u(?:\s*<<\s*(\d+))?" % name, (ROOT / "include" / "zkingest.h").read_text())
        v = int(m.group(1)) << int(m.group(2) or 0)
    return int(v)


MAX_FRAGMENT = _abi_const("ZK_INGEST_MAX_FRAGMENT")
MAX_EXPANSION = _abi_const("ZK_SNAPPY_MAX_EXPANSION")

ALPHA = string.ascii_letters + string.digits
PLACES = ("ann", "key", "svc", "name")  # where a case's payload string goes
OFFSETS = list(range(1, 18)) + [31, 32, 33, 255, 256, 2047, 2048]
LIT_LENGTHS = [1, 7, 8, 9, 15, 16, 17, 59, 60, 61, 255, 256, 257, 300]
TAIL = "\x00\x00\x02\x00\x09\x00\x00"  # the bytes after the last binary annotation's service name


class Case(NamedTuple):
    id: str
    span: Optional[Span]   # None: the stream is no Span (raw = 0, or malformed)
    stream: bytes
    payload: tuple = ()    # (place, string) when the span carries an observable payload

    @property
    def raw(self) -> bytes:
        return T.span(self.span) if self.span is not None else b""


# ---- spans --------------------------------------------------------------------------------------
def unit_of(rnd: random.Random, period: int) -> str:
    """`period` characters that are no repetition of a shorter string (the minimal period of its
    repetitions is `period`)"""
    while True:
        u = "".join(rnd.choices(ALPHA, k=period))
        if period == 1 or u not in (u + u)[1:-1]:
            return u


def repeat_to(unit: str, n: int) -> str:
    return (unit * (n // len(unit) + 1))[:n]


def make_span(pat: str, payload: str, place: str, *, trace_id=None, front=None, fill=None, back=None,
              extra_keys=(), tail_name=None) -> Span:
    """A Span whose ids, timestamps and endpoint numbers are 8 (4, 2) bytes of `pat` repeated, with
    `payload` at `place`. front: a leading host-less annotation (padding); fill: a leading host-less
    binary annotation value; back: a trailing one; extra_keys: more binary annotations with hosts;
    tail_name: the service name of the last binary annotation's host."""
    p = (pat * 24).encode()

    def num(k, n=8):
        return int.from_bytes(p[k:k + n], "big")

    svc = payload if place == "svc" else "svc-" + pat[:2]
    host = Endpoint(num(0, 4), num(1, 2), svc)
    other = Endpoint(num(2, 4), num(3, 2), "edge-" + pat[:1])
    anns = (Annotation(num(3), front, None),) if front is not None else ()
    anns += (Annotation(num(4), "sr", host),
             Annotation(num(5), payload if place == "ann" else "note-" + pat[:3], other),
             Annotation(num(6), "ss", other))
    bins = (BinaryAnnotation("fill", fill, "BYTES", None),) if fill is not None else ()
    last = other if tail_name is None else Endpoint(num(2, 4), num(3, 2), tail_name)
    bins += tuple(BinaryAnnotation(k, b"w", "String", other) for k in extra_keys)
    bins += (BinaryAnnotation(payload if place == "key" else "key-" + pat[:3], b"v", "String", last),)
    if back is not None:
        bins += (BinaryAnnotation("pad", back, "BYTES", None),)
    return Span(num(0) if trace_id is None else trace_id, payload if place == "name" else "op-" + pat[:2],
                num(1), num(2), anns, bins)


def small_span(tag: str, k: int) -> Span:
    rnd = random.Random("%s-%d" % (tag, k))
    return make_span(unit_of(rnd, 8), "%s.%d:%s" % (tag, k, unit_of(rnd, 8)), PLACES[k % 4])


def small_case(tag: str, k: int) -> Case:
    """a small valid fragment (a good neighbour, a filler): copy-2 elements at offsets 1..16"""
    span = small_span(tag, k)
    raw = T.span(span)
    return Case("%s-%d" % (tag, k), span, P.encode(raw, P.greedy(raw, P.COPY2, range(1, 17), (4, 64))))


# ---- the families -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_a():
    cases, n = [], 0
    for kind in P.KINDS:
        lo, hi = P.LEN_RANGE[kind]
        for off in OFFSETS:
            if off > P.MAX_OFFSET[kind]:
                continue
            for ln in range(lo, hi + 1):
                rnd = random.Random("A-%s-%d-%d" % (kind, ln, off))
                unit = unit_of(rnd, off)
                prefix = "%s.%d.%d:" % (kind[-1], ln, off)
                payload = prefix + repeat_to(unit, off + (2 * ln if off < 255 else ln))
                place = PLACES[n % 4]
                n += 1
                span = make_span(unit, payload, place)
                raw = T.span(span)
                # copies of this kind at this offset only, as long as possible up to ln: the payload's
                # repetitions (the first exactly ln long) and, for small offsets, the ids built from the unit
                plan = P.greedy(raw, kind, [off], (lo, ln))
                cases.append(Case("A-%s-L%d-o%d-%s" % (kind, ln, off, place), span, P.encode(raw, plan), (place, payload)))
        # a copy whose last byte is the Span's last byte: the last service name ends with the 7 bytes
        # that follow it (endpoint STOP, annotation STOP, the debug field, the Span's STOP)
        for ln in range(lo, 8):
            payload = "end.%s.%d" % (kind[-1], ln)
            span = make_span("e%s%dzqxjk" % (kind[-1], ln), payload, "ann", tail_name="last-" + payload + TAIL)
            raw = T.span(span)
            plan = P.copies_at(raw, len(raw) - ln, [(kind, ln, 7)])
            cases.append(Case("A-%s-L%d-o7-end" % (kind, ln), span, P.encode(raw, plan), ("ann", payload)))
        if lo == 1:  # the Span's last two bytes are both 0
            payload = "end1.%s" % kind[-1]
            span = make_span("E%sqzkxjw" % kind[-1], payload, "key")
            raw = T.span(span)
            cases.append(Case("A-%s-L1-o1-end" % kind, span, P.encode(raw, P.copies_at(raw, len(raw) - 1, [(kind, 1, 1)])),
                              ("key", payload)))
        # a copy right after the header's first literal, reaching back to byte 0 (o == offset): the
        # trace id field is 0a 00 01 + id, and the id repeats those three bytes
        for ln in range(lo, 9):
            payload = "head.%s.%d" % (kind[-1], ln)
            span = make_span("h%s%dwvuts" % (kind[-1], ln), payload, "name", trace_id=0x0A00010A00010A00)
            raw = T.span(span)
            plan = P.copies_at(raw, 3, [(kind, ln, 3)])
            cases.append(Case("A-%s-L%d-o3-head" % (kind, ln), span, P.encode(raw, plan), ("name", payload)))
    return cases


def copy_table(cases):
    """what the streams hold, read back from their bytes: {(kind, length, offset)}, the kinds with a copy
    ending on the last byte, and the kinds with a copy at o == offset"""
    seen, at_end, at_head = set(), set(), set()
    for c in cases:
        o, n = 0, len(c.raw)
        for kind, ln, arg in P.elements_of(c.stream):
            if kind != P.LIT:
                seen.add((kind, ln, arg))
                if o + ln == n:
                    at_end.add(kind)
                if o == arg:
                    at_head.add(kind)
            o += ln
    return seen, at_end, at_head


def required_copies(extra=()):
    return {(kind, ln, off) for kind in P.KINDS for off in OFFSETS + [o for k, o in extra if k == kind]
            if off <= P.MAX_OFFSET[kind] for ln in range(P.LEN_RANGE[kind][0], P.LEN_RANGE[kind][1] + 1)}


def literal_pairs():
    return [(ln, w) for ln in LIT_LENGTHS for w in range(P.min_width(ln), 5)]


@functools.lru_cache(maxsize=None)
def family_b():
    cases = []
    for n, (ln, w) in enumerate(literal_pairs()):
        rnd = random.Random("B-%d-%d" % (ln, w))
        prefix = "l.%d.%d:" % (ln, w)
        payload = prefix + "".join(rnd.choices(ALPHA, k=ln))
        place = PLACES[n % 4]
        span = make_span(unit_of(rnd, 8), payload, place)
        raw = T.span(span)
        plan = P.literal_at(raw, raw.index(payload.encode()) + len(prefix), ln, w)
        cases.append(Case("B-L%d-w%d-%s" % (ln, w, place), span, P.encode(raw, plan), (place, payload)))
    # every byte its own literal with a 4-byte length: the stream is 6 times the Span
    span = make_span("b6tesYBq", "every-byte-a-literal", "ann")
    raw = T.span(span)
    cases.append(Case("B-every-byte-w4", span, P.encode(raw, P.Plan([(P.LIT, 1, 4)] * len(raw))), ("ann", "every-byte-a-literal")))
    return cases


C_KEYS = tuple("c-key-%d-%s" % (k, "abcdefghijklmnopqrstuvwxyz"[k:] * 2) for k in range(3))
RUN_BYTE = b"\x07"


def c_span(t: int, run: int) -> Span:
    rnd = random.Random("C-%d" % t)
    place = PLACES[t % 4]
    return make_span(unit_of(rnd, 8), "lead.%d:%s" % (t, unit_of(rnd, 6)), place, fill=RUN_BYTE * run, extra_keys=C_KEYS)


@functools.lru_cache(maxsize=None)
def family_c():
    """One long run by copies, then k single-byte literals, then the rest as one literal; for every final
    lead t = raw - clen in 0..128, k = (37 t + 11) mod 129 (every k in 0..128 once) and the run length
    that gives t. The lead after the run is about t + k: above or below what the in-place decoder
    tolerates (its slack plus alignment terms), whatever that is exactly."""
    cases = []
    for t in range(129):
        k = (37 * t + 11) % 129
        probe = T.span(c_span(t, 16))
        start = probe.index(RUN_BYTE * 16)
        for run in range(16, 1200):
            if run & 0xFF == RUN_BYTE[0]:  # (the length field's last byte would extend the run)
                continue
            n = len(probe) - 16 + run
            plan = P.run_then_literals(n, start, run, k)
            if n - P.plan_size(n, plan) == t:
                break
        else:
            raise AssertionError("no run length gives lead %d with %d literals" % (t, k))
        span = c_span(t, run)
        raw = T.span(span)
        stream = P.encode(raw, plan)
        assert len(raw) - len(stream) == t
        cases.append(Case("C-lead%d-k%d-run%d" % (t, k, run), span, stream, (PLACES[t % 4], span_payload(span, PLACES[t % 4]))))
    return cases


def span_payload(span: Span, place: str) -> str:
    if place == "ann":
        return span.annotations[-2].value
    if place == "key":
        return [b for b in span.binary_annotations if b.host is not None][-1].key
    if place == "svc":
        return next(a.host.service_name for a in span.annotations if a.value == "sr")
    return span.name


@functools.lru_cache(maxsize=None)
def fillers():
    """16 valid all-literal fragments whose stream lengths cover every residue mod 16"""
    out = {}
    for p in range(16):
        span = Span(7, "f", 100 + p, None, (Annotation(5, "sr", Endpoint(1, 1, "filler")),),
                    (BinaryAnnotation("p", b"." * (70 + p), "BYTES", None),))
        raw = T.span(span)
        stream = P.encode(raw, P.Plan(P.literals(len(raw))))
        out[len(stream) % 16] = Case("filler-%d" % p, span, stream)
    assert sorted(out) == list(range(16))
    return out


def aligned(cases):
    """The cases at all 16 alignments of their first byte in the joined batch buffer: each is preceded
    by the filler fragment that makes its offset = a (mod 16), a = 0..15 in turn."""
    out, at = [], 0
    for a in range(16):
        for c in cases:
            f = fillers()[(a - at) % 16]
            out += [f, c]
            at += len(f.stream)
            assert at % 16 == a
            at += len(c.stream)
    return out


D_SIZES = list(range(620 - 48 - 40, 620 + 1)) + list(range(20480 - 48 - 64, 20480 + 16 + 1))


@functools.lru_cache(maxsize=None)
def family_d():
    """Incompressible Spans (a trailing binary-annotation value of random bytes) of exactly the sizes
    around the device's uniform/packed switch (regions of 640 bytes) and its LDS budget (20480)."""
    cases = []
    for n, size in enumerate(D_SIZES):
        rnd = random.Random("D-%d" % size)
        place = PLACES[n % 4]
        pat, payload = unit_of(rnd, 8), "size.%d:%s" % (size, unit_of(rnd, 5))
        base = len(T.span(make_span(pat, payload, place, back=b"")))
        pad = rnd.randbytes(size - base)
        span = make_span(pat, payload, place, back=pad)
        raw = T.span(span)
        assert len(raw) == size
        plan = P.greedy(raw, P.COPY2, range(1, 17), (4, 64), stop=raw.index(pad) if pad else None)
        cases.append(Case("D-raw%d-%s" % (size, place), span, P.encode(raw, plan), (place, payload)))
    return cases


@functools.lru_cache(maxsize=None)
def d_among():
    """every size of family D among 200 small fragments (rounds that mix layouts)"""
    small = [small_case("Dsmall", k) for k in range(200)]
    out = []
    for j, c in enumerate(family_d()):
        out += [small[j % 200], c]
    return out


E_BIG = ((P.COPY2, 65535), (P.COPY4, 65536), (P.COPY4, 70000))
E_LONG = 66000
E_PAD = "".join(random.Random("E-pad").choices(ALPHA, k=21000))


@functools.lru_cache(maxsize=None)
def family_e():
    """Families A and B behind a 21000-byte annotation (the fragment is larger than the device's LDS
    budget: the global-memory decoder). One fragment per (kind, offset) holds the copies of every
    length back to back over one periodic string; one fragment per place holds every literal."""
    cases, n = [], 0
    for kind in P.KINDS:
        lo, hi = P.LEN_RANGE[kind]
        lens = list(range(lo, hi + 1))
        for off in OFFSETS + [o for k, o in E_BIG if k == kind]:
            if off > P.MAX_OFFSET[kind]:
                continue
            rnd = random.Random("E-%s-%d" % (kind, off))
            unit = unit_of(rnd, off)
            prefix = "E%s.%d:" % (kind[-1], off)
            payload = prefix + repeat_to(unit, off + sum(lens))
            place = PLACES[n % 4] if off < 2047 else ("ann", "key")[n % 2]
            n += 1
            span = make_span(unit[:64], payload, place, front=E_PAD)
            raw = T.span(span)
            pos = raw.index(payload.encode()) + len(prefix) + off
            plan = P.copies_at(raw, pos, [(kind, ln, off) for ln in lens])
            cases.append(Case("E-%s-o%d-%s" % (kind, off, place), span, P.encode(raw, plan), (place, payload)))
    pairs = literal_pairs()
    for place in ("ann", "key"):
        rnd = random.Random("E-lit-" + place)
        prefix = "Elit.%s:" % place
        payload = prefix + "".join(rnd.choices(ALPHA, k=sum(ln for ln, _ in pairs)))
        span = make_span(unit_of(rnd, 8), payload, place, front=E_PAD)
        raw = T.span(span)
        pos = raw.index(payload.encode()) + len(prefix)
        els = P.literals(pos) + [(P.LIT, ln, w) for ln, w in pairs]
        els += P.literals(len(raw) - pos - sum(ln for ln, _ in pairs))
        cases.append(Case("E-literals-" + place, span, P.encode(raw, P.Plan(els)), (place, payload)))
    for w in (3, 4):  # a literal that needs the third length byte
        rnd = random.Random("E-long-%d" % w)
        prefix = "Elong.%d:" % w
        payload = prefix + "".join(rnd.choices(ALPHA, k=E_LONG))
        span = make_span(unit_of(rnd, 8), payload, "ann", front=E_PAD)
        raw = T.span(span)
        plan = P.literal_at(raw, raw.index(payload.encode()) + len(prefix), E_LONG, w)
        cases.append(Case("E-long-literal-w%d" % w, span, P.encode(raw, plan), ("ann", payload)))
    return cases


F_RUN = 1_000_000  # (the literals around the run cost ~350 bytes: past 21-fold needs a run of ~450000)


@functools.lru_cache(maxsize=None)
def family_f():
    cases = []
    tiny = Span(0x4142434445464748, "t", 0x4242424242424242, None)  # 51 bytes: a 1-byte minimal header
    normal = small_span("Fhdr", 0)
    for name, span, sizes in (("tiny", tiny, (2, 3, 4, 5)), ("normal", normal, (3, 4, 5))):
        raw = T.span(span)
        assert len(P.header(len(raw))) == sizes[0] - 1
        for hb in sizes:
            plan = P.greedy(raw, P.COPY2, range(1, 17), (4, 64), header_bytes=hb)
            cases.append(Case("F-%s-header%d" % (name, hb), span, P.encode(raw, plan)))
    # the densest legal stream: one literal up to a run's first byte, 64-byte offset-1 copies (3 bytes
    # each: 21.3-fold), and the 13 bytes that close the Span as a last literal
    span = make_span("F0densYQ", "densest-legal-stream", "ann", back=RUN_BYTE * F_RUN)
    raw = T.span(span)
    plan = P.run_then_literals(len(raw), raw.index(RUN_BYTE * F_RUN), F_RUN, 0)
    assert {e for e in plan.copies()[:-1]} == {(P.COPY2, 64, 1)}
    cases.append(Case("F-expansion", span, P.encode(raw, plan), ("ann", "densest-legal-stream")))
    cases.append(Case("F-raw0", None, b"\x00"))  # a valid Snappy stream of nothing: no Span
    return cases


@functools.lru_cache(maxsize=None)
def family_g():
    """[(id, stream)]: valid family-A streams (a copy ending on the last byte; for the literal, a last
    literal with a 2-byte length), each broken in exactly one way."""
    a = {c.id: c for c in family_a()}
    bad = []
    ends = {kind: a["A-%s-L5-o7-end" % kind] for kind in P.KINDS}
    for kind, c in ends.items():
        size = P.element_size((kind, 5, 7))
        for cut in range(1, size):  # the last element cut short at each of its bytes (the tag stays)
            bad.append(("G-%s-cut%d" % (kind, cut), c.stream[:-cut]))
        body = c.stream[:-size]
        o = len(c.raw) - 5
        bad.append(("G-%s-offset0" % kind, body + P.element_bytes((kind, 5, 0))))
        bad.append(("G-%s-offset-o+1" % kind, body + P.element_bytes((kind, 5, o + 1))))
        bad.append(("G-%s-one-too-long" % kind, body + P.element_bytes((kind, 6, 7))))
    c = ends[P.COPY2]
    raw, n = c.raw, len(c.raw)
    lit = P.encode(raw, P.Plan(P.literals(n - 5) + [(P.LIT, 5, 2)]))  # ends with tag 61, 2 length bytes, 5 bytes
    assert P.decode(lit) == raw
    for cut in range(1, 8):
        bad.append(("G-literal-cut%d" % cut, lit[:-cut]))
    bad.append(("G-last-literal-dropped", lit[:-8]))
    # a 3- or 4-byte length field with a high byte set: 2^16 (2^24) bytes more than the stream holds. A
    # decoder that drops the field's high bytes reads a valid 5-byte literal instead.
    for w, at in ((3, 2), (4, 2), (4, 3)):
        s = bytearray(P.encode(raw, P.Plan(P.literals(n - 5) + [(P.LIT, 5, w)])))
        s[len(s) - 5 - w + at] = 1
        bad.append(("G-literal-w%d-high-byte%d" % (w, at), bytes(s)))
    hdr = len(P.header(n))
    for d in (-1, 1):
        bad.append(("G-header%+d" % d, P.header(n + d) + c.stream[hdr:]))
    for bits in (0x10, 0x40, 0x70):  # a 5-byte varint with bit 32, 34, or 32..34 set
        h = bytearray(P.header(n, 5))
        h[4] |= bits
        bad.append(("G-varint-bit32-%02x" % bits, bytes(h) + c.stream[hdr:]))
    h = bytearray(P.header(n, 5))
    h[4] |= 0x80
    bad.append(("G-varint-endless", bytes(h) + c.stream[hdr:]))
    bad.append(("G-varint-cut", b"\x80\x80"))
    bad.append(("G-extra-literal", c.stream + P.element_bytes((P.LIT, 1, 0), b"x")))
    bad.append(("G-extra-copy", c.stream + P.element_bytes((P.COPY2, 1, 1))))
    return bad


@functools.lru_cache(maxsize=None)
def g_batch():
    """every bad stream between two good fragments: [good, bad, good, bad, ..., good] as Cases (a bad
    one has no Span)"""
    bad = family_g()
    out = [small_case("Ggood", 0)]
    for k, (cid, stream) in enumerate(bad):
        out += [Case(cid, None, stream), small_case("Ggood", k + 1)]
    assert len(out) >= 64
    return out


FAMILIES = {"A": family_a, "B": family_b, "C": lambda: aligned(family_c()), "D": d_among, "E": family_e,
            "F": family_f, "G": g_batch}


# ---- what a decoder gave, and what it should give -----------------------------------------------
def view(dec, result, *, items, span_names):
    """a decode call's result by name: records (service and span name as strings), rejected count, the
    item multisets as (service, string)"""
    cols, rej = result[0], result[1]
    cols = cols.to_host() if hasattr(cols, "to_host") else cols
    svc = dec.service_names()
    recs = records(cols)
    ids = cols.name_ids().tolist()
    names = dec.span_names() if span_names else []
    for r, k in zip(recs, ids):
        r["service"] = svc[r.pop("service_id")] if r["flags"] & (_abi.ZK_F_SVC_SERVER | _abi.ZK_F_SVC_CLIENT) else None
        r["flags"] &= 0xFFFF
        assert span_names or k == 0
        r["name"] = names[k - 1] if k else ""
    out = {"records": recs, "rejected": rej}
    if items:
        for key, (s, h) in (("kv", result[2]), ("ann", result[3])):
            if hasattr(s, "cpu"):
                s, h = s.cpu().numpy(), h.cpu().numpy()
            out[key] = Counter((svc[int(a)], dec.string(int(b) & (2**64 - 1))) for a, b in zip(s, h))
    return out


def expected_view(cases, *, items, span_names):
    """the same from the Spans alone (no Snappy, no thrift): cases without a Span are rejected"""
    spans = [c.span for c in cases if c.span is not None]
    want, ids = expected_records(spans)
    names = list(ids)
    for r, s in zip(want, spans):
        r["service"] = names[r.pop("service_id")] if r["flags"] & 12 else None
        r["name"] = s.name if span_names and s.name not in ("", "Unknown") else ""
    out = {"records": want, "rejected": len(cases) - len(spans)}
    if items:
        out["kv"], out["ann"] = expected_items(spans)
    return out


def project(v, *, items, span_names):
    """a view decoded with items and span names, as a decode without them would give it"""
    out = {"records": [dict(r, name=r["name"] if span_names else "") for r in v["records"]], "rejected": v["rejected"]}
    if items:
        out["kv"], out["ann"] = v["kv"], v["ann"]
    return out


def assert_payloads(dec, cases, *, items, span_names):
    """every payload string comes back: by hash, or as a service / span name"""
    svc = set(dec.service_names())
    names = set(dec.span_names()) if span_names else None
    for c in cases:
        if not c.payload:
            continue
        place, s = c.payload
        if place in ("ann", "key"):
            if items:
                assert dec.string(hash_string(s)) == s, c.id
        elif place == "svc":
            assert s in svc, c.id
        elif names is not None:
            assert s in names, c.id


def host_view(cases, snappy=True):
    dec = SpanDecoder()
    blobs = [c.stream if snappy else c.raw for c in cases]
    v = view(dec, dec.decode(blobs, snappy=snappy, strict=False, items=True, span_names=True), items=True, span_names=True)
    return dec, v


# ---- the tests ----------------------------------------------------------------------------------
def test_family_a_holds_every_copy():
    """a builder that fell back to literals would leave holes here"""
    seen, at_end, at_head = copy_table(family_a())
    assert not required_copies() - seen
    assert at_end == set(P.KINDS) and at_head == set(P.KINDS)
    assert len(family_a()) >= len(required_copies())


def test_family_e_holds_every_copy_and_literal():
    seen, _, _ = copy_table(family_e())
    assert not required_copies(E_BIG) - seen
    assert all(len(c.stream) > 21000 for c in family_e())
    lits = {(ln, w) for c in family_e() for k, ln, w in P.elements_of(c.stream) if k == P.LIT}
    assert not (set(literal_pairs()) | {(E_LONG, 3), (E_LONG, 4)}) - lits


def test_family_b_holds_every_literal():
    lits = {(ln, w) for c in family_b() for k, ln, w in P.elements_of(c.stream) if k == P.LIT}
    assert not set(literal_pairs()) - lits
    assert {w for ln, w in literal_pairs()} == {0, 1, 2, 3, 4} and (300, 4) in lits and (1, 4) in lits
    every = family_b()[-1]
    assert len(every.stream) > 5.9 * len(every.raw)


def test_family_c_sweeps_the_lead_at_every_alignment():
    cases = family_c()
    assert [len(c.raw) - len(c.stream) for c in cases] == list(range(129))
    assert sorted(int(c.id.split("-k")[1].split("-")[0]) for c in cases) == list(range(129))
    batch = aligned(cases)
    at, seen = 0, set()
    for c in batch:
        if c.id.startswith("C-"):
            seen.add((c.id, at % 16))
        at += len(c.stream)
    assert len(seen) == 129 * 16


def test_family_d_and_f_shapes():
    assert [len(c.raw) for c in family_d()] == D_SIZES
    assert all(len(c.stream) >= len(c.raw) - 64 for c in family_d())  # incompressible
    f = {c.id: c for c in family_f()}
    dense = f["F-expansion"]
    ratio = len(dense.raw) / (len(dense.stream) - len(P.header(len(dense.raw))))
    assert 21 < ratio < MAX_EXPANSION
    for hb in (2, 3, 4, 5):
        assert P.read_header(f["F-tiny-header%d" % hb].stream) == (51, hb)


@pytest.mark.parametrize("fam", ["A", "B", "C", "D", "E", "F"])
def test_valid_streams_decode_to_the_span_bytes(fam):
    """reference decoder == thrift bytes == libsnappy == zk_snappy_uncompress, for every valid stream.
    The project's two admission rules reject none of them (decode is called with and without)."""
    import pyarrow as pa

    codec = pa.Codec("snappy")
    cases = {"C": family_c, "D": family_d}.get(fam, FAMILIES[fam])()
    for c in cases:
        raw = c.raw
        assert P.decode(c.stream) == raw, c.id
        assert P.decode(c.stream, MAX_FRAGMENT, MAX_EXPANSION) == raw, c.id
        assert codec.decompress(c.stream, decompressed_size=len(raw), asbytes=True) == raw, c.id
        assert snappy_uncompress(c.stream) == raw, c.id


def test_malformed_streams_are_rejected_by_every_decoder():
    import pyarrow as pa

    codec = pa.Codec("snappy")
    base = len(family_a()[0].raw)
    for cid, stream in family_g():
        assert P.decode(stream) is None, cid
        assert P.decode(stream, MAX_FRAGMENT, MAX_EXPANSION) is None, cid
        h = P.read_header(stream)
        with pytest.raises(Exception):  # (pyarrow's error type for corrupt input)
            codec.decompress(stream, decompressed_size=h[0] if h else base, asbytes=True)
        with pytest.raises(ZkError) as e:
            snappy_uncompress(stream)
        assert e.value.status == _abi.ZK_ERR_INVALID_SPAN, cid


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_host_decoder(fam):
    """the host decoder on the streams == on the uncompressed thrift == the span-level expectation"""
    cases = FAMILIES[fam]()
    dec, got = host_view(cases)
    _, plain = host_view(cases, snappy=False)
    want = expected_view(cases, items=True, span_names=True)
    assert got["rejected"] == plain["rejected"] == want["rejected"]
    if fam == "G":
        assert got["rejected"] == len(family_g()) == sum(P.decode(c.stream) is None for c in cases)
    for k in ("records", "kv", "ann"):
        assert got[k] == plain[k], k
        assert got[k] == want[k], k
    assert_payloads(dec, cases, items=True, span_names=True)


def test_host_decoder_family_d_alone():
    """every size of family D as a batch of its own"""
    for c in family_d():
        dec, got = host_view([c])
        assert got == expected_view([c], items=True, span_names=True), c.id
        assert_payloads(dec, [c], items=True, span_names=True)


def strict_batches():
    """[(id, index of the first bad fragment, blobs)] for three of the malformed streams: good fragments,
    the bad one (in the first wave of 64, on a wave's first lane, in a third wave), a good one, and a
    second bad one that must not be the one named"""
    good = [small_case("Ggood", k).stream for k in range(131)]
    bad = family_g()
    return [(bad[j][0], at, good[:at] + [bad[j][1], good[at], bad[j + 1][1]]) for j, at in ((0, 1), (9, 64), (18, 130))]


def test_host_decoder_strict_names_the_first_bad_fragment():
    for cid, at, blobs in strict_batches():
        with pytest.raises(ZkError) as e:
            SpanDecoder().decode(blobs, strict=True)
        assert e.value.status == _abi.ZK_ERR_INVALID_SPAN and "span %d:" % at in e.value.message, (cid, e.value.message)
