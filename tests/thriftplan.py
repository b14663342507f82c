"""Thrift wire forms of a Span that Scrooge never writes, planned field by field.

Test infrastructure only. tests/thriftenc.py writes the one canonical layout; every decoder of
include/zkingest.h must also read any other legal TBinaryProtocol encoding of the same struct, skip
what it does not know, and reject what is no encoding at all -- all of them alike (the device has a
window-matched fast path for the canonical layout, a generic walk over LDS, the same walk over
global memory and three builds of each). The families below hold the forms; tests/thriftref.py says
what each means.

A Case is (id, raw thrift bytes, a Snappy stream of them, want, depth):
  want   a Span: the case was built from it and must decode to it; a rejection message of
         thriftref: it must be rejected with that class; None: the reference reader alone decides
  depth  (containers open at once inside one skipped value, leaf kind) for the nesting cases of
         family K, whose accept/reject the decoders' limits decide (host_accepts / device_accepts)

Families (FAMILIES: name -> function returning the case list; all deterministic):
  S1, S2  single-byte edits of the canonical base spans B1 and B2: at every byte each of SUBST that
          differs, every truncation, every single-byte deletion, every insertion of 00 and of 0C
  Z       the truncations of B1, B2 and B3, each with a fragment of zero bytes behind it
  A       canonical spans whose six string lengths sweep 0..8 (names also 15..17): full grids on
          every pair, a seeded sample of all six, parent_id present and absent -- every window of
          the device's fast path at every address residue mod 4, and the empty-string forms
  O       field order, absence, duplication, known ids with other wire types, odd field ids, debug
          bytes, bytes after the STOP
  K       unknown fields of every wire type at every struct level; malformed ones
  KD      the nesting cases (kept apart: the one documented divergence between host and device)
  G       a cross-section of O and K past the device's LDS budget (an unknown 21000-byte string
          field in front), among small canonical fragments
  GD      nesting cases around both limits, the same way
"""
from __future__ import annotations

import functools
import itertools
import random
import struct
from dataclasses import replace
from typing import List, NamedTuple, Optional, Tuple

from oracle.spans import UNKNOWN_SERVICE_NAME, Annotation, BinaryAnnotation, Endpoint, Span
from tests import thriftenc as T
from tests import thriftref as R

BOOL, BYTE, DOUBLE, I16, I32, I64, STRING, STRUCT, MAP, SET, LIST = 2, 3, 4, 6, 8, 10, 11, 12, 13, 14, 15
STOP = b"\x00"


class Case(NamedTuple):
    id: str
    raw: bytes
    stream: bytes
    want: object = None     # Span | rejection message | None
    depth: Optional[Tuple[int, str]] = None


def case(cid: str, raw: bytes, want=None, depth=None) -> Case:
    return Case(cid, raw, T.snappy(raw), want, depth)


# ---- wire elements ------------------------------------------------------------------------------
def fh(t: int, fid: int) -> bytes:
    return struct.pack(">Bh", t, fid)


def i16(v): return struct.pack(">h", v)
def i32(v): return struct.pack(">i", v)
def i64(v): return struct.pack(">q", v)


def s(b) -> bytes:
    b = b.encode() if isinstance(b, str) else bytes(b)
    return i32(len(b)) + b


def stru(fields) -> bytes:
    return b"".join(fields) + STOP


def seq(et: int, items, count=None) -> bytes:
    items = list(items)
    return struct.pack(">Bi", et, len(items) if count is None else count) + b"".join(items)


def mp(kt: int, vt: int, pairs, count=None) -> bytes:
    pairs = list(pairs)
    return struct.pack(">BBi", kt, vt, len(pairs) if count is None else count) + b"".join(k + v for k, v in pairs)


def ep_fields(e: Endpoint) -> List[bytes]:
    return [fh(I32, 1) + i32(e.ipv4), fh(I16, 2) + i16(e.port), fh(STRING, 3) + s(e.service_name)]


def ann_fields(a: Annotation) -> List[bytes]:
    """[timestamp, value, host, duration]; an absent one is b"" """
    return [fh(I64, 1) + i64(a.timestamp),
            fh(STRING, 2) + s(a.value) if a.value is not None else b"",
            fh(STRUCT, 3) + stru(ep_fields(a.host)) if a.host is not None else b"",
            fh(I32, 4) + i32(a.duration) if a.duration is not None else b""]


def bann_fields(b: BinaryAnnotation) -> List[bytes]:
    return [fh(STRING, 1) + s(b.key), fh(STRING, 2) + s(b.value), fh(I32, 3) + i32(T.ANNOTATION_TYPES[b.annotation_type]),
            fh(STRUCT, 4) + stru(ep_fields(b.host)) if b.host is not None else b""]


def ann_list(anns, fid=6) -> bytes:
    return fh(LIST, fid) + seq(STRUCT, [stru(ann_fields(a)) for a in anns])


def bann_list(bins, fid=8) -> bytes:
    return fh(LIST, fid) + seq(STRUCT, [stru(bann_fields(b)) for b in bins])


def span_fields(sp: Span) -> dict:
    """the canonical fields by id (5 only with a parent)"""
    f = {1: fh(I64, 1) + i64(sp.trace_id), 3: fh(STRING, 3) + s(sp.name), 4: fh(I64, 4) + i64(sp.id)}
    if sp.parent_id is not None:
        f[5] = fh(I64, 5) + i64(sp.parent_id)
    f[6] = ann_list(sp.annotations)
    f[8] = bann_list(sp.binary_annotations)
    f[9] = fh(BOOL, 9) + (b"\x01" if sp.debug else b"\x00")
    return f


# ---- base spans ---------------------------------------------------------------------------------
H1 = Endpoint(0x0A010203, 8080, "front-b1")
H2 = Endpoint(0x0A010204, 9411, "store-b1")
B1 = Span(0x1122334455667788, "get-b1", 0x2131415161718191, 0x0102030405060708,
          (Annotation(0x0005A0B0C0D0E0F1, "sr", H1), Annotation(0x0005A0B0C0D0E1F2, "custom-b1", H2),
           Annotation(0x0005A0B0C0D0E2F3, "ss", None)),
          (BinaryAnnotation("http.uri", b"/b1", "String", H1), BinaryAnnotation("nohost", b"\x07\x09", "BYTES", None)),
          debug=True)
HC = Endpoint(0x7F000001, 80, "client-b2")
B2 = Span(0x0F1E2D3C4B5A6978, "call-b2", 0x1213141516171819, None,
          (Annotation(0x0005A0B0C0D0F0A1, "cs", HC), Annotation(0x0005A0B0C0D0F1A2, "cr", HC)))
B3 = Span(0x3141592653589793, "idle-b3", 0x2718281828459045, None, (),
          (BinaryAnnotation("only.key", b"v3", "String", Endpoint(1, 2, "lonely-b3")),))
RAW_B1 = T.span(B1)
RAW_B2 = T.span(B2, write_debug=False, binary_annotations_field=False)
RAW_B3 = T.span(B3)
assert RAW_B1 == stru(span_fields(B1).values())  # the two encoders agree on the canonical layout

# ---- family S -----------------------------------------------------------------------------------
SUBST = (lambda o: 0x00, lambda o: 0x01, lambda o: o ^ 1, lambda o: (o + 1) & 0xFF, lambda o: 0x0B, lambda o: 0x0C,
         lambda o: 0x0F, lambda o: 0x7F, lambda o: 0x80, lambda o: 0xFF)


def single_byte_edits(tag: str, raw: bytes) -> List[Case]:
    out = []
    for at, orig in enumerate(raw):
        for v in sorted({f(orig) for f in SUBST} - {orig}):
            out.append(case("%s-sub%d-%02x" % (tag, at, v), raw[:at] + bytes([v]) + raw[at + 1:]))
    for n in range(len(raw)):
        out.append(case("%s-trunc%d" % (tag, n), raw[:n]))
    for at in range(len(raw)):
        out.append(case("%s-del%d" % (tag, at), raw[:at] + raw[at + 1:]))
    for at in range(len(raw) + 1):
        for v in (0x00, 0x0C):
            out.append(case("%s-ins%d-%02x" % (tag, at, v), raw[:at] + bytes([v]) + raw[at:]))
    return out


@functools.lru_cache(maxsize=None)
def family_s1():
    return single_byte_edits("S1", RAW_B1)


@functools.lru_cache(maxsize=None)
def family_s2():
    return single_byte_edits("S2", RAW_B2)


@functools.lru_cache(maxsize=None)
def family_z():
    """every truncation of B1, B2 and B3 with zero bytes behind it in the batch buffer: each is followed
    by a fragment of 4..7 zero bytes (a STOP and ignored bytes: no name), four times over so that the
    truncation's end falls at different places of its last 16-byte block. A window that reads past the
    fragment's end then reads STOP bytes, not the next fragment's 0A 00 01."""
    out = []
    for rep, pad in enumerate((4, 5, 6, 7)):
        for tag, raw in (("B1", RAW_B1), ("B2", RAW_B2), ("B3", RAW_B3)):
            for n in range(len(raw)):
                out.append(case("Z%d-%s-trunc%d" % (rep, tag, n), raw[:n]))
                out.append(case("Z%d-%s-zeros%d" % (rep, tag, n), b"\x00" * pad, R.NO_NAME))
    return out


# ---- family A -----------------------------------------------------------------------------------
A_DIMS = ("name", "aval", "ahost", "bkey", "bval", "bhost")
SHORT = tuple(range(9))
NAMES = SHORT + (15, 16, 17)
A_RANGE = {"name": NAMES, "aval": SHORT, "ahost": NAMES, "bkey": SHORT, "bval": SHORT, "bhost": NAMES}
A_DEFAULT = {"name": 5, "aval": 6, "ahost": 3, "bkey": 2, "bval": 1, "bhost": 7}
A_SAMPLE = 600


def text(tag: str, n: int) -> str:
    """n characters that spell no core annotation and not "Unknown" """
    return (tag + "qzjxvkwy" * 3)[:n]


def a_span(lens: dict, parent: bool, k: int) -> Span:
    ha = Endpoint(0x0A000001 + k, 1000 + k % 50000, text("H", lens["ahost"]))
    hb = Endpoint(0x0A800001 + k, 2000 + k % 50000, text("B", lens["bhost"]))
    t0 = 0x0005A00000000000 + 1000 * k
    return Span(0x5100000000000000 + k, text("N", lens["name"]), 0x5200000000000000 + k,
                0x5300000000000000 + k if parent else None,
                (Annotation(t0 + 1, "sr", ha), Annotation(t0 + 2, text("V", lens["aval"]), ha), Annotation(t0 + 3, "ss", None)),
                (BinaryAnnotation(text("K", lens["bkey"]), text("W", lens["bval"]).encode(), "String", hb),
                 BinaryAnnotation(text("k", lens["bkey"]), b"x", "BYTES", None)))


def a_want(sp: Span):
    return R.NO_VALUE if any(a.value == "" for a in sp.annotations) else sp


@functools.lru_cache(maxsize=None)
def family_a():
    out, k = [], 0
    for d0, d1 in itertools.combinations(A_DIMS, 2):
        for v0 in A_RANGE[d0]:
            for v1 in A_RANGE[d1]:
                lens = dict(A_DEFAULT, **{d0: v0, d1: v1})
                sp = a_span(lens, bool(k & 1), k)
                out.append(case("A-%s%d-%s%d-p%d" % (d0, v0, d1, v1, k & 1), T.span(sp), a_want(sp)))
                k += 1
    rnd = random.Random("family-A")
    for j in range(A_SAMPLE):
        lens = {d: rnd.choice(A_RANGE[d]) for d in A_DIMS}
        sp = a_span(lens, bool(rnd.getrandbits(1)), k)
        out.append(case("A-sample%d-%s" % (j, ".".join(str(lens[d]) for d in A_DIMS)), T.span(sp), a_want(sp)))
        k += 1
    return out


def fast_windows(raw: bytes) -> dict:
    """{window name: [byte offsets]} of a CANONICAL span: where the device's fast path places its
    windows (zk_ingest_dev.hip parse_record_fast: w1, w2, then per annotation c, h and -- with a host
    -- z; d; per binary annotation k1, k2, k3 and z; f). Walked with the layout's fixed widths only."""
    be32 = lambda at: struct.unpack(">i", raw[at:at + 4])[0]  # noqa: E731
    w = {k: [] for k in ("w1", "w2", "c", "h", "za", "d", "k1", "k2", "k3", "zb", "f")}
    p = 0
    w["w1"].append(p)
    p += 18 + be32(14)
    w["w2"].append(p)
    parent = raw[p + 11:p + 14] == fh(I64, 5)
    na = be32(p + (26 if parent else 15))
    p += 30 if parent else 19
    for _ in range(na):
        w["c"].append(p)
        p += 18 + be32(p + 14)
        w["h"].append(p)
        if raw[p] == 0:
            p += 1
        else:
            p += 22 + be32(p + 18)
            w["za"].append(p)
            p += 2
    w["d"].append(p)
    nb = 0
    if raw[p:p + 3] == fh(LIST, 8):
        nb = be32(p + 4)
        p += 8
    for _ in range(nb):
        w["k1"].append(p)
        p += 7 + be32(p + 3)
        w["k2"].append(p)
        p += 7 + be32(p + 3)
        w["k3"].append(p)
        if raw[p + 7] == 0:
            p += 8
        else:
            p += 29 + be32(p + 25)
            w["zb"].append(p)
            p += 2
    w["f"].append(p)
    assert raw[p:] in (STOP, fh(BOOL, 9) + b"\x00" + STOP, fh(BOOL, 9) + b"\x01" + STOP), "not the canonical layout"
    return w


# ---- family O -----------------------------------------------------------------------------------
HO = Endpoint(0x0A020301, 7001, "svc-o")
HP = Endpoint(0x0A020302, 7002, "peer-o")
OA = Annotation(0x0005B00000000111, "note-o", HP, duration=9)      # all four fields
OB = BinaryAnnotation("key-o", b"val-o", "String", HP)               # all four fields
O1 = Span(0x6100000000000001, "order-o", 0x6200000000000002, 0x6300000000000003,
          (Annotation(0x0005B00000000100, "sr", HO), OA, Annotation(0x0005B00000000122, "ss", HO)),
          (OB, BinaryAnnotation("bare-o", b"", "BYTES", None)), debug=False)
O_SPAN_PERMS = 500


def o_raw(sp: Span = O1, *, ann1: Optional[bytes] = None, bann0: Optional[bytes] = None, fields=None, order=None,
          extra=()) -> bytes:
    """O1 with annotation 1 / binary annotation 0 replaced by the given struct bytes, span fields
    replaced by id (`fields`: {id: bytes}), written in `order` (ids; default canonical), `extra`
    appended before the STOP"""
    f = span_fields(sp)
    if ann1 is not None:
        a = [stru(ann_fields(x)) for x in sp.annotations]
        a[1] = ann1
        f[6] = fh(LIST, 6) + seq(STRUCT, a)
    if bann0 is not None:
        b = [stru(bann_fields(x)) for x in sp.binary_annotations]
        b[0] = bann0
        f[8] = fh(LIST, 8) + seq(STRUCT, b)
    f.update(fields or {})
    return stru([f[k] for k in (order or sorted(f))] + list(extra))


def with_ann1(a: Optional[Annotation]) -> Span:
    anns = list(O1.annotations)
    anns[1] = a
    return replace(O1, annotations=tuple(anns))


def with_bann0(b: BinaryAnnotation) -> Span:
    return replace(O1, binary_annotations=(b,) + O1.binary_annotations[1:])


def host_named(name: Optional[str]) -> Endpoint:
    return Endpoint(HP.ipv4, HP.port, name if name else UNKNOWN_SERVICE_NAME)


def subsets(n: int):
    return itertools.product((True, False), repeat=n)


@functools.lru_cache(maxsize=None)
def family_o():
    out = []
    # -- order
    for p in itertools.permutations(range(4)):
        f = ann_fields(OA)
        out.append(case("O-ann-order%s" % "".join(map(str, p)), o_raw(ann1=stru(f[k] for k in p)), O1))
        f = bann_fields(OB)
        out.append(case("O-bann-order%s" % "".join(map(str, p)), o_raw(bann0=stru(f[k] for k in p)), O1))
    for p in itertools.permutations(range(3)):
        e = ep_fields(HP)
        host = fh(STRUCT, 3) + stru(e[k] for k in p)
        f = ann_fields(OA)
        out.append(case("O-ep-order%s" % "".join(map(str, p)), o_raw(ann1=stru([f[0], f[1], host, f[3]])), O1))
        host = fh(STRUCT, 4) + stru(e[k] for k in p)
        f = bann_fields(OB)
        out.append(case("O-bep-order%s" % "".join(map(str, p)), o_raw(bann0=stru(f[:3] + [host])), O1))
    ids = sorted(span_fields(B1))
    for r in range(1, len(ids)):
        out.append(case("O-span-rot%d" % r, o_raw(B1, order=ids[r:] + ids[:r]), B1))
    rnd = random.Random("family-O")
    seen = {tuple(ids)}
    while len(seen) <= O_SPAN_PERMS:
        p = tuple(rnd.sample(ids, len(ids)))
        if p not in seen:
            seen.add(p)
            out.append(case("O-span-order%s" % "".join(map(str, p)), o_raw(B1, order=list(p)), B1))
    # -- absence
    for ip, port, name in subsets(3):
        e = ep_fields(HP)
        host = fh(STRUCT, 3) + stru([e[0] if ip else b"", e[1] if port else b"", e[2] if name else b""])
        f = ann_fields(OA)
        want = with_ann1(replace(OA, host=host_named(HP.service_name if name else None)))
        out.append(case("O-ep-has-%d%d%d" % (ip, port, name), o_raw(ann1=stru([f[0], f[1], host, f[3]])), want))
        host = fh(STRUCT, 4) + host[3:]
        want = with_bann0(replace(OB, host=host_named(HP.service_name if name else None)))
        out.append(case("O-bep-has-%d%d%d" % (ip, port, name), o_raw(bann0=stru(bann_fields(OB)[:3] + [host])), want))
    for ts, value, host in subsets(3):
        f = ann_fields(OA)
        raw = o_raw(ann1=stru([f[0] if ts else b"", f[1] if value else b"", f[2] if host else b"", f[3]]))
        want = with_ann1(Annotation(OA.timestamp, OA.value if value else None, OA.host if host else None))
        out.append(case("O-ann-has-%d%d%d" % (ts, value, host), raw, want if ts else R.NO_TIMESTAMP))
    for has in subsets(5):
        keep = dict(zip((1, 3, 4, 6, 8), has))
        f = span_fields(O1)
        raw = stru(f[k] for k in sorted(f) if keep.get(k, True))
        want = Span(O1.trace_id if keep[1] else 0, O1.name, O1.id if keep[4] else 0, O1.parent_id,
                    O1.annotations if keep[6] else (), O1.binary_annotations if keep[8] else ())
        out.append(case("O-span-has-%s" % "".join(str(int(h)) for h in has), raw, want if keep[3] else R.NO_NAME))
    for key, value, typ, host in subsets(4):
        f = bann_fields(OB)
        raw = o_raw(bann0=stru(x for x, h in zip(f, (key, value, typ, host)) if h))
        want = with_bann0(BinaryAnnotation(OB.key if key else None, b"", "BYTES", OB.host if host else None))
        out.append(case("O-bann-has-%d%d%d%d" % (key, value, typ, host), raw, want))
    # -- duplication
    f = span_fields(O1)
    for fid, attr in ((1, "trace_id"), (4, "id"), (5, "parent_id")):
        other = fh(I64, fid) + i64(0x6F00000000000000 + fid)
        want = replace(O1, **{attr: 0x6F00000000000000 + fid})
        out.append(case("O-dup-%s-adjacent" % attr, stru(f[k] + (other if k == fid else b"") for k in sorted(f)), want))
        out.append(case("O-dup-%s-last" % attr, o_raw(extra=[other]), want))
        out.append(case("O-dup-%s-first" % attr, stru([other] + [f[k] for k in sorted(f)]), O1))
    out.append(case("O-dup-name", o_raw(extra=[fh(STRING, 3) + s("second-name")]), replace(O1, name="second-name")))
    la = (Annotation(0x0005B00000000200, "sr", HO), Annotation(0x0005B00000000250, "dup-o", HO))
    lb = (Annotation(0x0005B00000000240, "dup-o", HP), Annotation(0x0005B00000000260, "ss", HO),
          Annotation(0x0005B00000000270, "late-o", HP))
    want = replace(O1, annotations=la + lb)
    out.append(case("O-two-lists6-adjacent", o_raw(fields={6: ann_list(la) + ann_list(lb)}), want))
    out.append(case("O-two-lists6-apart", o_raw(fields={6: ann_list(la)}, extra=[ann_list(lb)]), want))
    out.append(case("O-two-lists6-first-empty", o_raw(fields={6: ann_list(()) + ann_list(lb)}), replace(O1, annotations=lb)))
    out.append(case("O-two-lists6-second-empty", o_raw(fields={6: ann_list(la) + ann_list(())}), replace(O1, annotations=la)))
    ka = (BinaryAnnotation("k-a", b"1", "String", HO), BinaryAnnotation("k-b", b"2", "String", None))
    kb = (BinaryAnnotation("k-a", b"3", "String", HP), BinaryAnnotation("k-c", b"4", "String", HO))
    want = replace(O1, binary_annotations=ka + kb)
    out.append(case("O-two-lists8-adjacent", o_raw(fields={8: bann_list(ka) + bann_list(kb)}), want))
    out.append(case("O-two-lists8-apart", o_raw(fields={8: bann_list(ka)}, extra=[bann_list(kb)]), want))
    out.append(case("O-list8-before-list6", o_raw(order=[1, 3, 4, 5, 8, 6, 9]), O1))
    f = ann_fields(OA)
    own = fh(STRUCT, 3) + stru(ep_fields(Endpoint(1, 2, "second-host")))
    bare = fh(STRUCT, 3) + stru(ep_fields(HP)[:2])
    empty = fh(STRUCT, 3) + stru(ep_fields(Endpoint(1, 2, "")))
    out.append(case("O-two-hosts-own-name", o_raw(ann1=stru([f[0], f[1], f[2], own, f[3]])),
                    with_ann1(replace(OA, host=host_named("second-host")))))
    out.append(case("O-two-hosts-second-bare", o_raw(ann1=stru([f[0], f[1], f[2], bare, f[3]])), O1))
    out.append(case("O-two-hosts-first-bare", o_raw(ann1=stru([f[0], bare, f[1], f[2]])), O1))
    out.append(case("O-two-hosts-second-empty-name", o_raw(ann1=stru([f[0], f[1], f[2], empty])),
                    with_ann1(replace(OA, host=host_named(None)))))
    out.append(case("O-two-hosts-only-bare", o_raw(ann1=stru([f[0], f[1], bare, bare])),
                    with_ann1(replace(OA, host=host_named(None)))))
    bf = bann_fields(OB)
    out.append(case("O-bann-two-hosts-own-name", o_raw(bann0=stru(bf + [fh(STRUCT, 4) + own[3:]])),
                    with_bann0(replace(OB, host=host_named("second-host")))))
    out.append(case("O-bann-two-hosts-second-bare", o_raw(bann0=stru(bf + [fh(STRUCT, 4) + bare[3:]])), O1))
    out.append(case("O-bann-two-keys", o_raw(bann0=stru(bf + [fh(STRING, 1) + s("key-2")])), with_bann0(replace(OB, key="key-2"))))
    out.append(case("O-two-values", o_raw(ann1=stru(f + [fh(STRING, 2) + s("value-2")])), with_ann1(replace(OA, value="value-2"))))
    out.append(case("O-two-values-second-empty", o_raw(ann1=stru(f + [fh(STRING, 2) + s("")])), R.NO_VALUE))
    out.append(case("O-two-values-first-empty", o_raw(ann1=stru([f[0], fh(STRING, 2) + s(""), f[1], f[2]])), O1))
    out.append(case("O-two-values-second-core", o_raw(ann1=stru(f + [fh(STRING, 2) + s("cs")])), with_ann1(replace(OA, value="cs"))))
    out.append(case("O-two-timestamps", o_raw(ann1=stru(f + [fh(I64, 1) + i64(0x0005B00000000099)])),
                    with_ann1(replace(OA, timestamp=0x0005B00000000099))))
    out.append(case("O-two-timestamps-second-zero", o_raw(ann1=stru(f + [fh(I64, 1) + i64(0)])), R.NO_TIMESTAMP))
    out.append(case("O-two-timestamps-first-zero", o_raw(ann1=stru([fh(I64, 1) + i64(0)] + f)), O1))
    e = ep_fields(HP)
    for tag, second in (("other", "renamed-o"), ("empty", "")):
        host = fh(STRUCT, 3) + stru(e + [fh(STRING, 3) + s(second)])
        out.append(case("O-two-service-names-%s" % tag, o_raw(ann1=stru([f[0], f[1], host])),
                        with_ann1(replace(OA, host=host_named(second)))))
        host = fh(STRUCT, 4) + host[3:]
        out.append(case("O-bann-two-service-names-%s" % tag, o_raw(bann0=stru(bf[:3] + [host])),
                        with_bann0(replace(OB, host=host_named(second)))))
    # -- known ids, other wire types
    anns = [stru(ann_fields(a)) for a in O1.annotations]
    bins = [stru(bann_fields(b)) for b in O1.binary_annotations]
    no6, no8 = replace(O1, annotations=()), replace(O1, binary_annotations=())
    out += [
        case("O-type-1-i32", o_raw(fields={1: fh(I32, 1) + i32(77)}), replace(O1, trace_id=0)),
        case("O-type-3-i64", o_raw(fields={3: fh(I64, 3) + i64(77)}), R.NO_NAME),
        case("O-type-3-i64-then-string", o_raw(fields={3: fh(I64, 3) + i64(77)}, extra=[fh(STRING, 3) + s("late-name")]),
             replace(O1, name="late-name")),
        case("O-type-5-i32", o_raw(fields={5: fh(I32, 5) + i32(77)}), replace(O1, parent_id=None)),
        case("O-type-5-i32-after-i64", o_raw(extra=[fh(I32, 5) + i32(77)]), O1),
        case("O-type-6-set", o_raw(fields={6: fh(SET, 6) + seq(STRUCT, anns)}), no6),
        case("O-type-6-map", o_raw(fields={6: fh(MAP, 6) + mp(STRING, STRUCT, [(s("k%d" % k), a) for k, a in enumerate(anns)])}), no6),
        case("O-type-6-struct", o_raw(fields={6: fh(STRUCT, 6) + anns[0]}), no6),
        case("O-type-8-set", o_raw(fields={8: fh(SET, 8) + seq(STRUCT, bins)}), no8),
        case("O-type-ann1-i32", o_raw(ann1=stru([fh(I32, 1) + i32(5)] + f[1:])), R.NO_TIMESTAMP),
        case("O-type-ann2-i64", o_raw(ann1=stru([f[0], fh(I64, 2) + i64(5), f[2]])), with_ann1(replace(OA, value=None))),
        case("O-type-ann3-string", o_raw(ann1=stru([f[0], f[1], fh(STRING, 3) + s("not-a-host")])), with_ann1(replace(OA, host=None))),
        case("O-type-ep3-i32", o_raw(ann1=stru([f[0], f[1], fh(STRUCT, 3) + stru(e[:2] + [fh(I32, 3) + i32(5)])])),
             with_ann1(replace(OA, host=host_named(None)))),
        case("O-type-bann1-i32", o_raw(bann0=stru([fh(I32, 1) + i32(5)] + bf[1:])), with_bann0(replace(OB, key=None))),
        case("O-type-bann4-string", o_raw(bann0=stru(bf[:3] + [fh(STRING, 4) + s("not-a-host")])), with_bann0(replace(OB, host=None))),
        case("O-type-bep3-i32", o_raw(bann0=stru(bf[:3] + [fh(STRUCT, 4) + stru(e[:2] + [fh(I32, 3) + i32(5)])])),
             with_bann0(replace(OB, host=host_named(None)))),
    ]
    for fid, whole in ((6, no6), (8, no8)):
        for name, et, items in (("i64", I64, [i64(1), i64(2)]), ("string", STRING, [s("sr"), s(""), s("x" * 40)]),
                                ("bool", BOOL, [b"\x01", b"\x00", b"\x02"])):
            out.append(case("O-list%d-of-%s" % (fid, name), o_raw(fields={fid: fh(LIST, fid) + seq(et, items)}), whole))
            both = fh(LIST, fid) + seq(et, items) + span_fields(O1)[fid]  # the list of structs after it still counts
            out.append(case("O-list%d-of-%s-then-structs" % (fid, name), o_raw(fields={fid: both}), O1))
    # -- odd field ids, debug bytes, bytes after the STOP
    for fid in (0, -1, 32767, -32768):
        junk = fh(I32, fid) + i32(0x0C0B0A09)
        out.append(case("O-field-id%d-span" % fid, o_raw(extra=[junk]), O1))
        out.append(case("O-field-id%d-span-first" % fid, stru([junk] + list(span_fields(O1).values())), O1))
        out.append(case("O-field-id%d-ann" % fid, o_raw(ann1=stru([junk] + f)), O1))
        out.append(case("O-field-id%d-ep" % fid, o_raw(ann1=stru([f[0], f[1], fh(STRUCT, 3) + stru([junk] + e)])), O1))
        out.append(case("O-field-id%d-bann" % fid, o_raw(bann0=stru(bf[:2] + [junk] + bf[2:])), O1))
    for v in (2, 0xFF):
        out.append(case("O-debug-%02x" % v, RAW_B1[:-2] + bytes([v]) + STOP, B1))
        out.append(case("O-debug-%02x-o1" % v, o_raw(fields={9: fh(BOOL, 9) + bytes([v])}), O1))
    out.append(case("O-debug-as-byte", o_raw(fields={9: fh(BYTE, 9) + b"\x01"}), O1))
    out.append(case("O-debug-twice", o_raw(extra=[fh(BOOL, 9) + b"\x01"]), O1))
    for k, tail in enumerate((STOP, b"\x0c\x00\x01", RAW_B2, b"\xff" * 7, fh(STRING, 3) + s("after-the-stop"), b"\x0b")):
        out.append(case("O-trailing%d-b1" % k, RAW_B1 + tail, B1))
        out.append(case("O-trailing%d-b2" % k, RAW_B2 + tail, B2))
        out.append(case("O-trailing%d-o1" % k, o_raw(order=[3, 1, 4, 5, 6, 8, 9]) + tail, O1))
    out += [case("O-b1", RAW_B1, B1), case("O-b2", RAW_B2, B2), case("O-b3", RAW_B3, B3), case("O-o1", o_raw(), O1)]
    return out


# ---- family K -----------------------------------------------------------------------------------
LEVELS = ("span", "ann", "ep", "bann", "bep")


def k_raw(level: str, field: bytes, first: bool = False) -> bytes:
    """O1 with the field bytes added to one struct: the span, annotation 1, its endpoint, binary
    annotation 0, or its endpoint; before the struct's other fields or after them"""
    put = (lambda fs: [field] + list(fs)) if first else (lambda fs: list(fs) + [field])
    if level == "span":
        return stru(put(span_fields(O1).values()))
    f, bf, e = ann_fields(OA), bann_fields(OB), ep_fields(HP)
    if level == "ann":
        return o_raw(ann1=stru(put(f)))
    if level == "ep":
        return o_raw(ann1=stru([f[0], f[1], fh(STRUCT, 3) + stru(put(e)), f[3]]))
    if level == "bann":
        return o_raw(bann0=stru(put(bf)))
    return o_raw(bann0=stru(bf[:3] + [fh(STRUCT, 4) + stru(put(e))]))


FLAT_STRUCT = stru([fh(I32, 1) + i32(7), fh(STRING, 2) + s("in-a-struct"), fh(BOOL, 3) + b"\x01"])
K_VALID = (
    ("bool", BOOL, b"\x01"), ("byte", BYTE, b"\x80"), ("double", DOUBLE, struct.pack(">d", 2.5)), ("i16", I16, i16(-2)),
    ("i32", I32, i32(0x0B0C0D0F)), ("i64", I64, i64(-3)), ("string0", STRING, s("")), ("string1", STRING, s("z")),
    ("string300", STRING, s("0123456789" * 30)),
    ("struct", STRUCT, FLAT_STRUCT), ("empty-struct", STRUCT, STOP),
    ("list", LIST, seq(I32, [i32(1), i32(2), i32(3)])), ("set", SET, seq(STRING, [s("a"), s(""), s("ccc")])),
    ("list0", LIST, seq(STRUCT, [])), ("map", MAP, mp(STRING, I32, [(s("a"), i32(1)), (s("bb"), i32(2))])),
    ("map-of-structs", MAP, mp(I16, STRUCT, [(i16(1), FLAT_STRUCT), (i16(2), STOP)])),
    ("map0-odd-types", MAP, mp(0x7F, 0x63, [])), ("map0-zero-types", MAP, mp(0, 0, [])),
    ("list0-odd-type", LIST, seq(0x10, [])), ("set0-odd-type", SET, seq(1, [])),
    ("list-of-structs", LIST, seq(STRUCT, [FLAT_STRUCT, STOP, stru([fh(STRUCT, 9) + FLAT_STRUCT])])),
    ("list-of-maps-of-structs", LIST, seq(MAP, [mp(STRING, STRUCT, [(s("k"), FLAT_STRUCT), (s("l"), STOP)]),
                                                 mp(STRING, STRUCT, [])])),
    ("struct-of-lists", STRUCT, stru([fh(LIST, 1) + seq(I64, [i64(1), i64(2)]), fh(LIST, 2) + seq(STRING, [s("x")]),
                                      fh(SET, 3) + seq(LIST, [seq(BYTE, [b"\x01"])])])),
    ("list-of-lists", LIST, seq(LIST, [seq(I16, [i16(1)]), seq(I16, [])])),
)
K_BAD = (
    ("list-count-1", LIST, seq(I32, [], count=-1)), ("set-count-1", SET, seq(I32, [], count=-1)),
    ("map-count-1", MAP, mp(I32, I32, [], count=-1)), ("list-count-min", LIST, seq(BYTE, [], count=-2**31)),
    ("map-count-2p29+1", MAP, mp(BYTE, BYTE, [(b"\x01", b"\x02")], count=2**29 + 1)),
    ("map-count-2p30", MAP, mp(BYTE, BYTE, [(b"\x01", b"\x02")], count=2**30)),
    ("list-count-2p31-1", LIST, seq(I64, [i64(1)], count=2**31 - 1)),
    ("string-len-1", STRING, i32(-1)), ("string-len-min", STRING, i32(-2**31)),
    ("list-of-type16", LIST, seq(16, [b"\x00"])), ("map-key-type1", MAP, mp(1, I32, [(b"\x00", i32(1))])),
    ("struct-field-type5", STRUCT, stru([fh(5, 1) + b"\x00"])),
) + tuple(("type%d" % t, t, b"\x00" * 8) for t in (1, 5, 7, 9, 16))
REST = 0x7FFFFF01  # a string length to be replaced by what remains of the fragment


def patch_rest(raw: bytes, plus: int) -> bytes:
    at = raw.index(i32(REST))
    return raw[:at] + i32(len(raw) - at - 4 + plus) + raw[at + 4:]


@functools.lru_cache(maxsize=None)
def family_k():
    out = []
    for level in LEVELS:
        for first in (False, True):
            where = "%s-%s" % (level, "first" if first else "last")
            for name, t, body in K_VALID:
                out.append(case("K-%s-%s" % (name, where), k_raw(level, fh(t, 20) + body, first), O1))
            for name, t, body in K_BAD:
                out.append(case("K-bad-%s-%s" % (name, where), k_raw(level, fh(t, 20) + body, first), R.UNDECODABLE))
            for plus in (0, 1):  # to the fragment's last byte (no STOP left), and one past it
                raw = patch_rest(k_raw(level, fh(STRING, 20) + i32(REST), first), plus)
                out.append(case("K-bad-string-rest+%d-%s" % (plus, where), raw, R.UNDECODABLE))
    # a large count over an empty element list costs nothing to walk: a list of 2^31-1 zero-field structs
    # would, so only counts whose first element already fails are planned
    return out


# -- nesting
DEPTHS = (1, 15, 16, 17, 64, 65, 66)
DEVICE_SKIP_DEPTH = 16  # zk_ingest_dev.hip DRdT::skip: a 17th container opening inside one skipped value fails
HOST_SKIP_DEPTH = 64    # zk_ingest.cpp Rd::skip(t, depth): any value, container or not, with depth > 64 fails;
#                         a value's depth is the number of containers open around it inside the skipped value


def nest(kinds: str, leaf) -> Tuple[int, bytes]:
    """(wire type, bytes) of containers nested as `kinds` says, outermost first ('s' struct, 'l' list,
    'e' set, 'm' map); leaf: (type, bytes) inside the innermost, or None to leave that one empty"""
    if not kinds:
        return leaf
    inner = nest(kinds[1:], leaf) if kinds[1:] or leaf else None
    k = kinds[0]
    if k == "s":
        return STRUCT, stru([fh(inner[0], 1) + inner[1]] if inner else [])
    if k in "le":
        return (LIST if k == "l" else SET), seq(inner[0] if inner else I32, [inner[1]] if inner else [])
    return MAP, mp(I32, inner[0] if inner else I32, [(i32(5), inner[1])] if inner else [])


def host_accepts(depth: int, leaf: str) -> bool:
    """Rd::skip: the innermost container sits at depth - 1, a scalar inside it at depth"""
    return (depth if leaf == "scalar" else depth - 1) <= HOST_SKIP_DEPTH


def device_accepts(depth: int, leaf: str) -> bool:
    return depth <= DEVICE_SKIP_DEPTH


K_SHAPES = {"struct": "s", "mixed-s": "slm", "mixed-l": "lsm", "mixed-ls": "lssm", "mixed-m": "mesl"}


@functools.lru_cache(maxsize=None)
def family_kd():
    out = []
    for level in LEVELS:
        for shape, cycle in K_SHAPES.items():
            for d in DEPTHS:
                for leaf_name, leaf in (("empty", None), ("scalar", (I32, i32(42)))):
                    t, body = nest((cycle * d)[:d], leaf)
                    out.append(case("KD-%s-%s-depth%d-%s" % (level, shape, d, leaf_name), k_raw(level, fh(t, 20) + body),
                                    O1, (d, leaf_name)))
    # field 6 / 8 as a list of maps (skipped element by element, the list being the first container),
    # in front of the field's list of structs
    for fid in (6, 8):
        for d in DEPTHS[1:]:
            for leaf_name, leaf in (("empty", None), ("scalar", (I32, i32(42)))):
                t, body = nest(("lmsl" * d)[:d], leaf)
                assert t == LIST and body[0] == MAP
                out.append(case("KD-list%d-of-maps-depth%d-%s" % (fid, d, leaf_name),
                                o_raw(fields={fid: fh(LIST, fid) + body + span_fields(O1)[fid]}), O1, (d, leaf_name)))
    return out


# ---- family G -----------------------------------------------------------------------------------
G_PAD = random.Random("family-G").randbytes(21000)
G_BUDGET = 20480  # the device's LDS bytes per wave (zk_ingest_dev.hip kLdsBudget)
G_STRIDE = {"O": 11, "K": 7}


def small(k: int) -> Case:
    sp = a_span({d: 3 + (k + j) % 5 for j, d in enumerate(A_DIMS)}, bool(k & 1), 100000 + k)
    return case("G-small%d" % k, T.span(sp), sp)


def behind_the_pad(picked) -> List[Case]:
    pad = fh(STRING, 31) + s(G_PAD)
    out = []
    for k, c in enumerate(picked):
        out += [small(2 * k), small(2 * k + 1), case("G-" + c.id, pad + c.raw, c.want, c.depth)]
    return out


@functools.lru_cache(maxsize=None)
def family_g():
    """every G_STRIDE-th case of O and K behind an unknown 21000-byte string field (random bytes: the
    Snappy stream stays past the budget too), two small canonical fragments between each two"""
    return behind_the_pad([c for fam, cases in (("O", family_o()), ("K", family_k())) for c in cases[3::G_STRIDE[fam]]])


@functools.lru_cache(maxsize=None)
def family_gd():
    """nesting cases around both limits the same way (apart from G, as KD is from K)"""
    return behind_the_pad([c for c in family_kd() if c.id.startswith(("KD-span-", "KD-bann-")) and c.depth[0] in (16, 17, 65, 66)
                           and ("-struct-" in c.id or "-mixed-l-" in c.id)])


FAMILIES = {"S1": family_s1, "S2": family_s2, "Z": family_z, "A": family_a, "O": family_o, "K": family_k, "KD": family_kd, "G": family_g,
            "GD": family_gd}
DEPTH_FAMILIES = ("KD", "GD")
