"""The span store by trace id (include/zkspans.h): tracesExist, getSpansByTraceIds and trace summaries
from whole records in HBM.

TraceSpanStore keeps every observed 48-B fragment, grouped by a hash of its trace id, and hands the
fragments of asked traces back (SpanStore.tracesExist / getSpansByTraceIds). Trace and TraceSummary restate
the reference's Trace.scala and TraceSummary.scala at record granularity on the host, so that the ids a
TraceNameIndex, TraceAnnotationIndex or TraceDurationIndex returns become the query service's
getTraceSummariesByIds without another store.

A trace's fragments travel as a list of ROWS, tuples (trace_id, span_id, parent_id, first_ts, last_ts,
service_id, flags) of Python ints, in the header's canonical order.

With a TraceAnnotationStore (annotstore.py) beside it, a Trace also carries every span's annotations, and the
query service's adjusters and timelines are built over them on the host: TimeSkewAdjuster
(TimeSkewAdjuster.scala), TraceTimeline (TraceTimeline.scala), adjust= and annotations= on the by-id calls, and
getTraceTimelinesByIds.
"""
from __future__ import annotations

import ctypes as C
import gc
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import _abi
from .annotstore import (KIND_CR, KIND_CS, KIND_NAMES, KIND_SR, KIND_SS, LOOPBACK_IPV4, Annotation, AnnotationRow, Endpoint,
                         annotation_key)
from .binannotstore import BinaryAnnotation, BinaryAnnotationRow, binary_annotation_key
from .columns import COLUMNS, ENTRY_COLUMNS, SUMMARY_HEAD, DeviceColumns  # noqa: F401  (zk_sp_summary's head and entries)

INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
_M64 = 2 ** 64 - 1

Row = Tuple[int, int, int, int, int, int, int]

# zk_sp_trace, the 48-byte head of one asked id, and zk_sp_span, one merged span (48 bytes)
TRACE_HEAD = np.dtype([("trace_id", np.uint64), ("start", np.int64), ("end", np.int64), ("root_most", np.uint64),
                       ("fragments", np.uint32), ("spans", np.uint32), ("services", np.uint32), ("state", np.uint32)])
TRACE_SPAN = np.dtype([("span_id", np.uint64), ("parent_id", np.uint64), ("first", np.int64), ("last", np.int64),
                       ("name", np.uint32), ("depth", np.uint32), ("services", np.uint32), ("bits", np.uint32)])


def _wrap64(x: int) -> int:
    """x as the JVM's Long holds it (two's complement, 64 bits)."""
    x &= _M64
    return x - 2 ** 64 if x >= 2 ** 63 else x


def _to_int(x: int) -> int:
    """Long.toInt: the low 32 bits as a signed value."""
    x &= 0xFFFFFFFF
    return x - 2 ** 32 if x >= 2 ** 31 else x


def canonical_key(row: Row) -> tuple:
    """The canonical order inside a trace: (span_id, parent_id, first_ts, last_ts, service_id, flags)."""
    return row[1:]


class Span(NamedTuple):
    """One merged span of a Trace. parent, first, last: None when no fragment has one. name: the span-name
    id (0: none), or with a span_names dictionary the name (None: none). services: ascending service ids,
    or with a services dictionary the lower-cased names in the ids' order."""
    trace_id: int
    id: int
    parent: Optional[int]
    name: Union[int, str, None]
    first: Optional[int]
    last: Optional[int]
    services: tuple


class AnnotatedSpan(Span):
    """A Span of a Trace that was given annotation rows: the same seven fields (it compares as a Span), and
    `annotations`, the span's list of Annotation (canonical order as stored; list order after an adjuster)."""

    annotations: List[Annotation]


class SpanTimestamp(NamedTuple):
    """The reference's SpanTimestamp(name, startTimestamp, endTimestamp); name is the service."""
    name: Union[int, str]
    start_timestamp: int
    end_timestamp: int

    @property
    def duration(self) -> int:
        return _wrap64(self.end_timestamp - self.start_timestamp)


class Timespan(NamedTuple):
    start: int
    end: int


class Trace:
    """Trace.scala over one trace's rows (in any order; they are put into canonical order first, so every
    answer is a function of the multiset of rows).

    spans: the fragments merged by span id. A span is timed when any of its fragments is
    (ZK_F_HAS_ANNOTATIONS); first = the minimum first_ts and last = the maximum last_ts over its TIMED
    fragments; parent = the parent_id of the first fragment (canonical order) with ZK_F_HAS_PARENT; the
    name id = the first non-zero one in canonical order; services = the ascending set of service_id over
    the fragments with ZK_F_SVC_CLIENT | ZK_F_SVC_SERVER. Spans are sorted by first, an untimed span as
    INT64_MAX (Trace.scala:38-43); ties go by span id ascending as unsigned (the reference's tie order is
    a HashMap's: a stated choice).

    annotations: the trace's annotation rows (annotstore.AnnotationRow, any order; rows of a span id the
    trace has no record of are ignored). Every span is then an AnnotatedSpan that carries its annotations as
    a list in canonical order, `annotations` maps span id -> that list, and the first and last of a span
    that has annotation rows are the minimum and maximum ts of those rows; a span without rows keeps its
    record times. Services, parent and name stay the records' rules. Without it `annotations` is None and
    nothing changes.

    binary: the trace's binary-annotation rows (binannotstore.BinaryAnnotationRow, any order), attached by
    span id after the trace is built (attach_binary): `binary_annotations` then maps span id -> the span's
    BinaryAnnotations in canonical order, for every span of the trace; rows of a span id the trace has no
    span of are ignored. Without it `binary_annotations` is None and getBinaryAnnotations() is []."""

    binary_annotations: Optional[Dict[int, List[BinaryAnnotation]]] = None

    def __init__(self, rows: Sequence[Row], services: Optional[Sequence[str]] = None,
                 span_names: Optional[Sequence[str]] = None, annotations: Optional[Sequence[AnnotationRow]] = None,
                 binary: Optional[Sequence[BinaryAnnotationRow]] = None):
        self.rows: List[Row] = sorted((tuple(int(v) for v in r) for r in rows), key=canonical_key)
        self._services = None if services is None else list(services)
        self._span_names = None if span_names is None else list(span_names)
        self.annotations: Optional[Dict[int, List[Annotation]]] = None
        self.spans: List[Span] = self._merge()
        self._given = None
        if annotations is not None:
            by_span: Dict[int, List[Annotation]] = {}
            for r in sorted((tuple(int(v) for v in r) for r in annotations), key=annotation_key):
                by_span.setdefault(r[1], []).append(Annotation.of_row(r))
            self._annotate({s.id: by_span.get(s.id, []) for s in self.spans})
        if binary is not None:
            self.attach_binary(binary)

    def attach_binary(self, rows: Sequence[BinaryAnnotationRow]) -> "Trace":
        """Attach the trace's binary-annotation rows by span id: every span of the trace as it stands gets its
        rows in canonical order ([] without any); rows of other span ids are ignored. Returns self."""
        by_span: Dict[int, List[BinaryAnnotation]] = {s.id: [] for s in self.spans}
        for r in sorted((tuple(int(v) for v in r) for r in rows), key=binary_annotation_key):
            if r[1] in by_span:
                by_span[r[1]].append(BinaryAnnotation.of_row(r))
        self.binary_annotations = by_span
        return self

    def getBinaryAnnotations(self) -> List[BinaryAnnotation]:
        """Trace.getBinaryAnnotations (Trace.scala:161-165): the binary annotations of all spans, the spans
        in the trace's span order, each span's in canonical order. [] without attached rows."""
        given = self.binary_annotations or {}
        return [b for s in self.spans for b in given.get(s.id, ())]

    def getBinaryAnnotationsByKey(self, key) -> List[BinaryAnnotation]:
        """Trace.getBinaryAnnotationsByKey (Trace.scala:167-171): those whose key is `key` (the key's hash, as
        the rows carry it), in getBinaryAnnotations' order."""
        return [b for b in self.getBinaryAnnotations() if b.key == key]

    def _annotate(self, anns: Dict[int, List[Annotation]]) -> None:
        """Every span of anns (the others are dropped) as an AnnotatedSpan with its list, the times of a
        span with annotations from them, and the spans in span order again."""
        spans = []
        for s in self.spans:
            if s.id not in anns:
                continue
            a = anns[s.id]
            first, last = (min(x.ts for x in a), max(x.ts for x in a)) if a else (s.first, s.last)
            n = AnnotatedSpan(s.trace_id, s.id, s.parent, s.name, first, last, s.services)
            n.annotations = a
            spans.append(n)
        spans.sort(key=lambda s: (INT64_MAX if s.first is None else s.first, s.id))
        self.spans = spans
        self.annotations = {s.id: s.annotations for s in spans}

    def with_annotations(self, anns: Dict[int, List[Annotation]]) -> "Trace":
        """A Trace of this one's spans that anns names, each with the list anns gives it (an adjuster's
        result): the trace rebuilt from them, so span times and span order follow the new lists."""
        t = Trace.__new__(Trace)
        t.rows = None if self.rows is None else [r for r in self.rows if r[1] in anns]
        t._services, t._span_names, t._given = self._services, self._span_names, None
        t.spans = list(self.spans)
        t._annotate(anns)
        if self.binary_annotations is not None:  # (a pruned span's binary annotations leave with it)
            t.binary_annotations = {s.id: self.binary_annotations.get(s.id, []) for s in t.spans}
        return t

    @classmethod
    def of_merged(cls, spans: Sequence[Span], root_most: Optional[int], depths: Optional[Dict[int, int]]) -> "Trace":
        """A Trace from spans that are merged and in span order already (zk_sp_traces' answer), with the
        root-most span's id and the span depths that came with them: rows is None, and getRootMostSpan and
        toSpanDepths hand back what was given."""
        t = cls.__new__(cls)
        t.rows, t._services, t._span_names, t.annotations = None, None, None, None
        t.spans = list(spans)
        t._given = (root_most, depths)
        return t

    def _service(self, i: int):
        if self._services is None:
            return i
        if i >= len(self._services):
            raise ValueError("a service id beyond the services dictionary")
        return self._services[i].lower()

    def _name(self, i: int):
        if self._span_names is None:
            return i
        if i == 0:
            return None
        if i > len(self._span_names):
            raise ValueError("a name id beyond the span_names dictionary")
        return self._span_names[i - 1]

    def _merge(self) -> List[Span]:
        acc: Dict[int, list] = {}
        for tid, sid, pid, first, last, svc, fl in self.rows:
            a = acc.setdefault(sid, [tid, None, 0, None, None, set()])
            if fl & _abi.ZK_F_HAS_PARENT and a[1] is None:
                a[1] = pid
            if a[2] == 0:
                a[2] = (fl >> _abi.ZK_F_NAME_SHIFT) & _abi.ZK_F_NAME_MASK
            if fl & _abi.ZK_F_HAS_ANNOTATIONS:
                a[3] = first if a[3] is None else min(a[3], first)
                a[4] = last if a[4] is None else max(a[4], last)
            if fl & (_abi.ZK_F_SVC_CLIENT | _abi.ZK_F_SVC_SERVER):
                a[5].add(svc)
        spans = [Span(a[0], sid, a[1], self._name(a[2]), a[3], a[4], tuple(self._service(s) for s in sorted(a[5])))
                 for sid, a in acc.items()]
        spans.sort(key=lambda s: (INT64_MAX if s.first is None else s.first, s.id))
        return spans

    @property
    def id(self) -> Optional[int]:
        return self.spans[0].trace_id if self.spans else None

    def getRootSpan(self) -> Optional[Span]:
        """The first span without a parent."""
        return next((s for s in self.spans if s.parent is None), None)

    def getSpanById(self, span_id: int) -> Optional[Span]:
        return next((s for s in self.spans if s.id == span_id), None)

    def getIdToSpanMap(self) -> Dict[int, Span]:
        return {s.id: s for s in self.spans}

    def getRootMostSpan(self) -> Optional[Span]:
        """The root span, else (Trace.scala:70-85) from the first span upwards through the parents the
        trace holds, to the last one found. A parent chain that closes on itself ends where it would
        repeat (the reference does not terminate on one)."""
        if self._given is not None:
            return None if not self.spans else self.getSpanById(self._given[0])
        root = self.getRootSpan()
        if root is not None or not self.spans:
            return root
        by_id = self.getIdToSpanMap()
        s, seen = self.spans[0], set()
        while s.parent is not None and s.parent in by_id and s.id not in seen:
            seen.add(s.id)
            s = by_id[s.parent]
        return s

    def getRootSpans(self) -> List[Span]:
        """Trace.scala:77-78: the spans whose parent is none or not a span of this trace, in span order."""
        by_id = self.getIdToSpanMap()
        return [s for s in self.spans if s.parent is None or s.parent not in by_id]

    def getIdToChildrenMap(self) -> Dict[int, List[Span]]:
        """parent id -> its child spans, in span order."""
        out: Dict[int, List[Span]] = {}
        for s in self.spans:
            if s.parent is not None:
                out.setdefault(s.parent, []).append(s)
        return out

    def toSpanDepths(self) -> Optional[Dict[int, int]]:
        """span id -> depth in the tree under the root-most span, which is at depth 1; None for a trace
        without spans. A span reached twice keeps its first depth."""
        if self._given is not None:
            return self._given[1]
        root = self.getRootMostSpan()
        if root is None:
            return None
        children = self.getIdToChildrenMap()
        depths, level, d = {}, [root], 1
        while level:
            nxt = []
            for s in level:
                if s.id in depths:
                    continue
                depths[s.id] = d
                nxt += children.get(s.id, [])
            level, d = nxt, d + 1
        return depths

    def getStartAndEndTimestamp(self) -> Optional[Timespan]:
        """(min first, max last) over the timed fragments; None when no fragment is timed."""
        timed = [s for s in self.spans if s.first is not None]
        if not timed:
            return None
        return Timespan(min(s.first for s in timed), max(s.last for s in timed))

    @property
    def duration(self) -> int:
        """end - start as the reference's wrapping Long subtraction; 0 for a trace without times."""
        t = self.getStartAndEndTimestamp()
        return 0 if t is None else _wrap64(t.end - t.start)

    @property
    def services(self) -> set:
        return {v for s in self.spans for v in s.services}

    def serviceCounts(self) -> Dict[Union[int, str], int]:
        """service -> the number of merged spans that name it."""
        out: Dict[Union[int, str], int] = {}
        for s in self.spans:
            for v in set(s.services):
                out[v] = out.get(v, 0) + 1
        return out

    def spanTimestamps(self) -> List[SpanTimestamp]:
        """(service, first, last) for each timed span, in span order, and for each of the span's
        services, ascending by id."""
        return [SpanTimestamp(v, s.first, s.last) for s in self.spans if s.first is not None for v in s.services]


class TraceSummary(NamedTuple):
    """The reference's TraceSummary. duration_micro = (end - start) wrapped to 64 bits and truncated to a
    signed 32-bit value (its .toInt). endpoints is always []: a record carries no ip or port."""
    trace_id: int
    start: int
    end: int
    duration_micro: int
    span_timestamps: List[SpanTimestamp]
    endpoints: list

    @staticmethod
    def of(trace: Trace) -> Optional["TraceSummary"]:
        """TraceSummary.apply: None for a trace without spans or without a timed fragment."""
        t = trace.getStartAndEndTimestamp()
        if trace.id is None or t is None:
            return None
        return TraceSummary(trace.id, t.start, t.end, _to_int(_wrap64(t.end - t.start)), trace.spanTimestamps(), [])


def _jvm_half(x: int) -> int:
    """x / 2 as the JVM divides a Long: truncated toward zero."""
    q = abs(x) >> 1
    return -q if x < 0 else q


class TimeSkewAdjuster:
    """TimeSkewAdjuster.scala over a Trace that carries annotations: the clock skew between a span's client
    and server side is taken out of the server's annotations, from the root down. All arithmetic is the
    JVM's (Long wraps, / 2 truncates toward zero).

    Where the reference depends on arrival or hash order, these are STATED CHOICES: the children of a span
    are the spans whose parent is its id, in span order; "first with a value" (getAnnotation) is the first in
    the span's list and "last with a value" (getAnnotationsAsMap) the last; the list is in canonical order,
    which breaks the ties of equal timestamps. Injected annotations carry the hashes of "sr" and "ss"."""

    NAME = "TIME_SKEW"

    @staticmethod
    def skew(cs: int, cr: int, sr: int, ss: int, endpoint: Optional[Endpoint]) -> Optional[Tuple[Endpoint, int]]:
        cd, sd = _wrap64(cr - cs), _wrap64(ss - sr)
        if sd > cd or (cs < sr and cr > ss):  # the server side is longer: invalid; or already inside: no skew
            return None
        latency = _jvm_half(_wrap64(cd - sd))
        skew = _wrap64(_wrap64(sr - latency) - cs)
        if skew == 0 or endpoint is None:
            return None
        return endpoint, skew

    @staticmethod
    def _shift(anns: List[Annotation], endpoint: Endpoint, skew: int) -> None:
        if skew == 0:
            return
        for i, a in enumerate(anns):
            if a.host is not None and (a.host.ipv4 == endpoint.ipv4 or
                                       (a.kind in (KIND_CS, KIND_CR) and a.host.ipv4 == LOOPBACK_IPV4)):
                anns[i] = a._replace(ts=_wrap64(a.ts - skew))

    @staticmethod
    def _first(anns: List[Annotation], kinds: tuple) -> Optional[Annotation]:
        return next((a for a in anns if a.kind in kinds), None)

    @classmethod
    def adjust(cls, trace: Trace) -> Trace:
        """The trace with the skews taken out. Root: the first span in span order without a parent; without
        one the trace is returned as it is, with one the result holds only the spans under it (the reference
        rebuilds the trace from the root's tree). The walk is iterative: a chain of any length is fine."""
        from .ingest import hash_string

        root = trace.getRootSpan()
        if root is None:
            return trace
        given = trace.annotations or {}
        anns: Dict[int, List[Annotation]] = {s.id: list(given.get(s.id, ())) for s in trace.spans}
        children = trace.getIdToChildrenMap()
        h_sr, h_ss = hash_string("sr"), hash_string("ss")
        out: Dict[int, List[Annotation]] = {}
        stack: List[Tuple[int, Optional[Tuple[Endpoint, int]]]] = [(root.id, None)]
        while stack:
            sid, prev = stack.pop()
            if sid in out:
                continue
            a = out[sid] = anns[sid]
            kids = children.get(sid, [])
            if prev is not None:  # 1. the skew handed down by the parent
                cls._shift(a, *prev)
            count = [0] * 8
            for x in a:
                count[x.kind] += 1
            if max(count[KIND_CS:KIND_SS + 1]) <= 1 and count[KIND_CS] and count[KIND_CR] and \
                    not (count[KIND_SR] and count[KIND_SS]) and kids:  # 2. a client-only span with children
                lead = cls._first(anns[kids[0].id], (KIND_CS, KIND_CR))
                endpoint = None if lead is None else lead.host
                cs, cr = cls._first(a, (KIND_CS,)), cls._first(a, (KIND_CR,))
                a.append(Annotation(cs.ts, h_sr, KIND_SR, endpoint))
                a.append(Annotation(cr.ts, h_ss, KIND_SS, endpoint))
                for k in kids:
                    ka = anns[k.id]
                    kcs, kcr = cls._first(ka, (KIND_CS,)), cls._first(ka, (KIND_CR,))
                    if kcs is not None and kcr is not None:
                        sk = cls.skew(cs.ts, cr.ts, kcs.ts, kcr.ts, endpoint)
                        if sk is not None:
                            cls._shift(ka, *sk)
            last = {x.kind: x for x in a if KIND_CS <= x.kind <= KIND_SS}  # 3. the span's own skew
            own = None
            if len(last) == 4:
                own = cls.skew(last[KIND_CS].ts, last[KIND_CR].ts, last[KIND_SR].ts, last[KIND_SS].ts, last[KIND_SR].host)
                if own is not None:
                    cls._shift(a, *own)
            stack.extend((k.id, own) for k in reversed(kids))
        return trace.with_annotations(out)


ADJUSTERS = {"NOTHING": lambda trace: trace, "TIME_SKEW": TimeSkewAdjuster.adjust}


def apply_adjusters(trace: Trace, adjust: Sequence[str]) -> Trace:
    """The adjusters folded over the trace in order, as QueryService folds its own."""
    for name in adjust:
        trace = ADJUSTERS[name](trace)
    return trace


class TimelineAnnotation(NamedTuple):
    """The reference's TimelineAnnotation, flat: the annotation's ts and value (the hash, or the text with
    a decoder), its host (ipv4, port, and service: the id, or the name with a dictionary), and its span's
    id, parent and name. Without a host: Endpoint.Unknown's zeros, and "Unknown" for a service name."""
    ts: int
    value: Union[int, str]
    ipv4: int
    port: int
    service: Union[int, str]
    span_id: int
    parent_id: Optional[int]
    span_name: Union[int, str, None]


def resolve_binary(binaries: Sequence[BinaryAnnotation], decoder=None, services: Optional[Sequence[str]] = None) -> list:
    """BinaryAnnotations for a reader: with a decoder (.string and .bytes by hash) the key becomes text and
    the value its bytes; with the services dictionary a host's service id becomes its name."""
    if decoder is None and services is None:
        return list(binaries)
    out = []
    for b in binaries:
        key, value, host = b.key, b.value, b.host
        if decoder is not None:
            key, value = decoder.string(key), decoder.bytes(value)
        if host is not None and services is not None:
            if host.service_id >= len(services):
                raise ValueError("a service id beyond the services dictionary")
            host = Endpoint(host.ipv4, host.port, services[host.service_id])
        out.append(BinaryAnnotation(key, value, b.type, host, b.span_id))
    return out


class TraceTimeline(NamedTuple):
    """The reference's TraceTimeline(traceId, rootSpanId, annotations, binaryAnnotations).
    binary_annotations is trace.getBinaryAnnotations(): [] unless the trace carries binary-annotation rows
    (binary=, a TraceBinaryAnnotationStore, on the by-id calls)."""
    trace_id: int
    root_span_id: int
    annotations: List[TimelineAnnotation]
    binary_annotations: list

    @staticmethod
    def of(trace: Trace, decoder=None, services: Optional[Sequence[str]] = None) -> Optional["TraceTimeline"]:
        """TraceTimeline.apply: None for a trace without spans; else all annotations of all spans (the spans
        in span order, each span's list in its order), sorted by ts with a STABLE sort, which is the stated
        order of equal timestamps. decoder: anything with .string(hash) (a SpanDecoder) turns values into
        text (a core annotation's is its kind's). services: the service dictionary, by id, as it stands.
        binary_annotations: the trace's (getBinaryAnnotations); with the decoder the keys become text and the
        values bytes (decoder.bytes), with the dictionary a host's service becomes its name."""
        if not trace.spans:
            return None
        given = trace.annotations or {}
        out: List[TimelineAnnotation] = []
        for s in trace.spans:
            for a in given.get(s.id, ()):
                value: Union[int, str] = a.value
                if decoder is not None:
                    value = KIND_NAMES[a.kind] if a.kind else decoder.string(a.value)
                if a.host is None:
                    ipv4, port, svc = 0, 0, (0 if services is None else "Unknown")
                else:
                    ipv4, port, svc = a.host.ipv4, a.host.port, a.host.service_id
                    if services is not None:
                        if svc >= len(services):
                            raise ValueError("a service id beyond the services dictionary")
                        svc = services[svc]
                out.append(TimelineAnnotation(a.ts, value, ipv4, port, svc, s.id, s.parent, s.name))
        out.sort(key=lambda t: t.ts)
        return TraceTimeline(trace.id, trace.getRootMostSpan().id, out, resolve_binary(trace.getBinaryAnnotations(), decoder, services))


class TraceCombo(NamedTuple):
    """The reference's TraceCombo(trace, traceSummary, traceTimeline, spanDepths). timeline is None unless
    the trace was built with an annotation store's rows: a record carries no annotations to lay out."""
    trace: Trace
    summary: Optional[TraceSummary]
    timeline: Optional[TraceTimeline]
    span_depths: Optional[Dict[int, int]]

    @staticmethod
    def of(trace: Trace, timeline: Optional[TraceTimeline] = None) -> "TraceCombo":
        return TraceCombo(trace, TraceSummary.of(trace), timeline, trace.toSpanDepths())


class TraceSpanStore:
    """A zk_sp handle. `with TraceSpanStore() as store:` frees it on exit.

    services / span_names: the decoders' dictionaries (index i of services is service id i, index i of
    span_names is name id i + 1); with them the Traces this store builds give services as lower-cased
    names (Span.serviceNames) and span names as strings; without, as ids."""

    OBSERVE_PHASES = ("count", "size", "scatter")
    EXPIRE_PHASES = ("ends", "size", "rewrite")

    def __init__(self, device: int = 0, timing: bool = False, stream: Optional[int] = None,
                 services: Optional[Sequence[str]] = None, span_names: Optional[Sequence[str]] = None,
                 expire_chunk: int = 0):
        self._L = _abi.lib()
        cfg = _abi.zk_sp_config()
        cfg.device = device
        cfg.timing = 1 if timing else 0
        cfg.stream = stream
        cfg.expire_chunk = expire_chunk  # expire's entries per range of buckets at most (0: 2^24)
        h = C.c_void_p()
        st = self._L.zk_sp_create(C.byref(cfg), C.byref(h))
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, _abi.status_str(st))
        self._h = h
        self.device = device
        self.services = None if services is None else list(services)
        self.span_names = None if span_names is None else list(span_names)
        self._held = None  # device record columns a queued observe may still read (TraceAnnotationStore.observe_stored)

    def _check(self, st: int) -> None:
        if st != _abi.ZK_OK:
            raise _abi.ZkError(st, self._L.zk_sp_last_error(self._h).decode() or _abi.status_str(st))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.zk_sp_destroy(self._h)
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
        """Add a batch's records (host SpanColumns or DeviceColumns, any order) as one segment
        (zk_sp_observe). Observing a batch again adds it again. sync=False leaves the scatter queued on
        the handle's stream: device columns must then stay as they are until the next call that
        synchronises (info, tracesExist, getSpansByTraceIds, compact, observe)."""
        flags = 0
        ab = cols.abi()
        if isinstance(cols, DeviceColumns):
            import torch

            flags |= _abi.ZK_BATCH_DEVICE_PTRS
            torch.cuda.current_stream(self.device).synchronize()  # (torch may still be writing the batch)
        self._check(self._L.zk_sp_observe(self._h, C.byref(ab), flags))
        if sync:
            self.info()

    def reset(self) -> None:
        """Empty the store (zk_sp_reset)."""
        self._check(self._L.zk_sp_reset(self._h))

    def compact(self) -> None:
        """Merge all segments into one (zk_sp_compact)."""
        self._check(self._L.zk_sp_compact(self._h))

    def expire(self, min_end: int, pins: Optional[Dict[int, int]] = None) -> int:
        """Remove every trace whose end (the maximum last_ts of its timed fragments, INT64_MIN without
        one) is below its cutoff, whole (zk_sp_expire): the cutoff is min_end, or pins[trace_id] for a
        pinned trace. The entries removed. More than ZK_SP_MAX_PINS pins are refused: a second call would
        judge the first call's pinned traces by the default."""
        pins = {} if pins is None else dict(pins)
        if len(pins) > _abi.ZK_SP_MAX_PINS:
            raise ValueError("more than ZK_SP_MAX_PINS pins in one expiry")
        ids = np.array([int(k) & _M64 for k in pins], np.uint64)
        cuts = np.array([int(v) for v in pins.values()], np.int64)
        removed = C.c_uint64()
        self._check(self._L.zk_sp_expire(self._h, int(min_end), ids.ctypes.data if len(ids) else None,
                                         cuts.ctypes.data if len(ids) else None, len(ids), C.byref(removed)))
        return int(removed.value)

    def info(self) -> dict:
        """{"entries", "segments", "bytes"} (zk_sp_info); synchronises."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._L.zk_sp_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
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

    def exist(self, ids) -> np.ndarray:
        """found bool[n] for at most ZK_SP_MAX_IDS ids, in the order asked (zk_sp_exist)."""
        keep, ptr, n, flags = self._ask(ids)
        f = np.zeros(n, np.uint8)
        self._check(self._L.zk_sp_exist(self._h, ptr, n, flags, f.ctypes.data_as(C.POINTER(C.c_uint8))))
        return f.astype(bool)

    def gather(self, ids):
        """(counts uint32[n], columns) for at most ZK_SP_MAX_IDS ids (zk_sp_gather): the sizing call, then
        the call that fills seven numpy columns (a dict by column name) of exactly the total."""
        keep, ptr, n, flags = self._ask(ids)
        counts = np.zeros(n, np.uint32)
        cp = counts.ctypes.data_as(_abi._U32P)
        total = C.c_uint64()
        st = self._L.zk_sp_gather(self._h, ptr, n, flags, cp, None, 0, C.byref(total))
        if st not in (_abi.ZK_OK, _abi.ZK_ERR_CAPACITY):
            self._check(st)
        cols = {k: np.zeros(total.value, dt) for k, dt in COLUMNS}
        if st == _abi.ZK_ERR_CAPACITY:
            rows = _abi.zk_sp_rows(*[cols[k].ctypes.data for k, _ in COLUMNS])
            self._check(self._L.zk_sp_gather(self._h, ptr, n, flags, cp, C.byref(rows), total.value, C.byref(total)))
        return counts, cols

    def _chunks(self, ids):
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
        for a in range(0, len(ids), _abi.ZK_SP_MAX_IDS):
            yield ids[a:a + _abi.ZK_SP_MAX_IDS]

    def tracesExist(self, ids) -> set:
        """SpanStore.tracesExist: the asked ids that some observed fragment carries."""
        out = set()
        for part in self._chunks(ids):
            out.update(part[self.exist(part)].tolist())
        return out

    def getSpansByTraceIds(self, ids) -> List[List[Row]]:
        """SpanStore.getSpansByTraceIds: one list of rows, in canonical order, per asked id that was
        found, in the order asked; ids that are not found are left out (SpanStore.scala:76-84), a
        duplicated id is answered as often as asked."""
        out: List[List[Row]] = []
        for part in self._chunks(ids):
            counts, cols = self.gather(part)
            rows = list(zip(*[cols[k].tolist() for k, _ in COLUMNS]))
            at = 0
            for c in counts.tolist():
                if c:
                    out.append(rows[at:at + c])
                at += c
        return out

    def getSpansByTraceId(self, trace_id: int) -> List[Row]:
        """The rows of one trace; [] when it is not found."""
        found = self.getSpansByTraceIds([trace_id])
        return found[0] if found else []

    @staticmethod
    def _adjusters(adjust, annotations) -> tuple:
        """adjust as a tuple of known names; a non-empty one needs an annotation store."""
        adjust = (adjust,) if isinstance(adjust, str) else tuple(adjust)
        for name in adjust:
            if name not in ADJUSTERS:
                raise ValueError(f"unknown adjuster {name!r}: NOTHING or TIME_SKEW")
        if adjust and annotations is None:
            raise ValueError("adjust needs annotations=, a TraceAnnotationStore")
        return adjust

    def _adjust_on_device(self, adjust, annotations, on_device: bool = False) -> None:
        """The rules of adjust_on_device=True: annotations= and "TIME_SKEW" as the only adjuster besides
        "NOTHING", once, and not on_device=True beside it; anything else is a ValueError."""
        adjust = self._adjusters(adjust, annotations)
        if on_device:
            raise ValueError("adjust_on_device=True replaces on_device=True: give one of them")
        if [name for name in adjust if name != "NOTHING"] != ["TIME_SKEW"] or annotations is None:
            raise ValueError('adjust_on_device=True needs annotations= and adjust=("TIME_SKEW",), applied once')

    def _combos_adjusted_on_device(self, ids, annotations, decoder=None, lists=True, timelines=True) -> List[TraceCombo]:
        """getTraceCombosByIds(adjust=("TIME_SKEW",), annotations=) from annotations.adjusted_traces(): the
        adjusted traces with their annotations, summaries, timelines and depths from one answer per chunk; a
        trace above the device's bounds goes the host's way. The cyclic collector is paused while the tuples
        are built, as in _combos_on_device. lists, timelines: _combos_of's."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64))
        out: List[TraceCombo] = []
        paused = gc.isenabled()
        gc.disable()
        try:
            for a in range(0, len(ids), _abi.ZK_AN_MAX_IDS):
                self._combos_of(out, *annotations.adjusted_traces(self, ids[a:a + _abi.ZK_AN_MAX_IDS]), annotations=annotations,
                                decoder=decoder, lists=lists, timelines=timelines)
        finally:
            if paused:
                gc.enable()
        return out

    def _combos_on_host(self, ids, adjust, annotations, decoder=None) -> List[TraceCombo]:
        """The host path of getTraceCombosByIds with an annotation store."""
        return [TraceCombo.of(t, TraceTimeline.of(t, decoder, self.services)) for t in self.getTracesByIds(ids, adjust, annotations)]

    def _attach_binary(self, traces: Sequence[Trace], binary) -> None:
        """Every trace gets its rows of `binary`, a TraceBinaryAnnotationStore, by span id, after it is built
        (and adjusted): one lookup for all of them."""
        traces = [t for t in traces if t.id is not None]
        if not traces:
            return
        for t, rows in zip(traces, binary.getBinaryAnnotationsByTraceIds([t.id for t in traces])):
            t.attach_binary(rows)

    def _combos_with_binary(self, combos: List[TraceCombo], binary, decoder=None) -> List[TraceCombo]:
        """The combos with their traces' binary annotations attached and their timelines' fourth field filled."""
        self._attach_binary([c.trace for c in combos], binary)
        return [c if c.timeline is None else c._replace(timeline=c.timeline._replace(
            binary_annotations=resolve_binary(c.trace.getBinaryAnnotations(), decoder, self.services))) for c in combos]

    def getTracesByIds(self, ids, adjust: Sequence[str] = (), annotations=None, adjust_on_device: bool = False,
                       binary=None) -> List[Trace]:
        """One Trace per asked id that was found, in the order asked. annotations: a TraceAnnotationStore;
        every Trace then carries its annotations (Trace's annotations=). adjust: a sequence of "NOTHING" /
        "TIME_SKEW", folded over each trace in order as QueryService folds its adjusters; it needs
        annotations=. A trace that has no rows in the annotation store is returned unadjusted.
        adjust_on_device: the adjuster runs on the device (zk_an_adjusted_traces; the rules of
        getTraceSummariesByIds' adjust_on_device). The answer is the host path's, with ONE difference:
        Trace.rows is None, as with Trace.of_merged.
        binary: a TraceBinaryAnnotationStore; every Trace then carries its binary annotations
        (Trace.attach_binary, after the adjusters: a pruned span's leave with it). It needs no annotations=."""
        if binary is not None:
            out = self.getTracesByIds(ids, adjust, annotations, adjust_on_device)
            self._attach_binary(out, binary)
            return out
        if adjust_on_device:
            self._adjust_on_device(adjust, annotations)
            return [c.trace for c in self._combos_adjusted_on_device(ids, annotations, timelines=False)]
        adjust = self._adjusters(adjust, annotations)
        found = self.getSpansByTraceIds(ids)
        if annotations is None:
            return [Trace(rows, self.services, self.span_names) for rows in found]
        theirs = annotations.getAnnotationsByTraceIds([rows[0][0] for rows in found])
        out = []
        for rows, a in zip(found, theirs):
            t = Trace(rows, self.services, self.span_names, annotations=a)
            out.append(apply_adjusters(t, adjust) if a else t)
        return out

    def getTraceTimelinesByIds(self, ids, adjust: Sequence[str] = (), annotations=None, decoder=None,
                               adjust_on_device: bool = False, binary=None) -> List[TraceTimeline]:
        """QueryService.getTraceTimelinesByIds: the timeline of every asked trace that was found, in the
        order asked, after the adjusters. annotations=, a TraceAnnotationStore, is required. decoder: turns
        the values into text (TraceTimeline.of); service names come from the store's services dictionary.
        adjust_on_device: as for getTracesByIds; the answer is the same. binary: a TraceBinaryAnnotationStore;
        the timelines' binary_annotations are then the traces' (keys as text and values as bytes with the
        decoder, host services as names with the dictionary); without it they are []."""
        if annotations is None:
            raise ValueError("timelines need annotations=, a TraceAnnotationStore")
        if binary is not None:
            combos = self.getTraceCombosByIds(ids, adjust=adjust, annotations=annotations, adjust_on_device=adjust_on_device,
                                              binary=binary, decoder=decoder)
            return [c.timeline for c in combos if c.timeline is not None]
        if adjust_on_device:
            self._adjust_on_device(adjust, annotations)
            return [c.timeline for c in self._combos_adjusted_on_device(ids, annotations, decoder, lists=False)]
        lines = (TraceTimeline.of(t, decoder, self.services) for t in self.getTracesByIds(ids, adjust, annotations))
        return [t for t in lines if t is not None]

    def summaries(self, ids):
        """(heads, entries) for at most ZK_SP_MAX_IDS ids (zk_sp_summaries): heads, a SUMMARY_HEAD array in
        the order asked, and the (service_id, first, last) entries of all asked traces one after another
        (a dict of three numpy columns of exactly the total). The sizing call, then the call that fills."""
        keep, ptr, n, flags = self._ask(ids)
        heads = np.zeros(n, SUMMARY_HEAD)
        total = C.c_uint64()
        st = self._L.zk_sp_summaries(self._h, ptr, n, flags, heads.ctypes.data, None, 0, C.byref(total))
        if st not in (_abi.ZK_OK, _abi.ZK_ERR_CAPACITY):
            self._check(st)
        cols = {k: np.zeros(total.value, dt) for k, dt in ENTRY_COLUMNS}
        if st == _abi.ZK_ERR_CAPACITY:
            out = _abi.zk_sp_span_ts(*[cols[k].ctypes.data for k, _ in ENTRY_COLUMNS])
            self._check(self._L.zk_sp_summaries(self._h, ptr, n, flags, heads.ctypes.data, C.byref(out), total.value,
                                                C.byref(total)))
        return heads, cols

    def _summaries_on_device(self, ids) -> List[TraceSummary]:
        """getTraceSummariesByIds from summaries(): the services go through the dictionary as in
        Trace._service (lower-cased names; an entry's service id beyond the dictionary is a ValueError)."""
        out: List[TraceSummary] = []
        low = None if self.services is None else [s.lower() for s in self.services]
        for part in self._chunks(ids):
            heads, cols = self.summaries(part)
            svc, first, last = (cols[k].tolist() for k, _ in ENTRY_COLUMNS)
            if low is not None:
                if svc and max(svc) >= len(low):
                    raise ValueError("a service id beyond the services dictionary")
                svc = [low[i] for i in svc]
            entries = list(map(SpanTimestamp, svc, first, last))
            at = 0
            for tid, start, end, _, _, c, state in heads.tolist():
                if state & _abi.ZK_SP_SUM_OVERFLOW:  # a trace too long for the device merge: the host path
                    out += self.getTraceSummariesByIds([tid])
                elif state & _abi.ZK_SP_SUM_TIMED:
                    out.append(TraceSummary(tid, start, end, _to_int(_wrap64(end - start)), entries[at:at + c], []))
                at += c
        return out

    def traces(self, ids):
        """(heads, spans, services) for at most ZK_SP_MAX_IDS ids (zk_sp_traces): heads, a TRACE_HEAD array in
        the order asked; the merged spans of all asked traces one after another, each trace's in span order
        (a TRACE_SPAN array of exactly the total); and the spans' service ids, a uint32 column. The sizing
        call, then the call that fills."""
        keep, ptr, n, flags = self._ask(ids)
        heads = np.zeros(n, TRACE_HEAD)
        total = (C.c_uint64 * 2)()
        st = self._L.zk_sp_traces(self._h, ptr, n, flags, heads.ctypes.data, None, 0, None, 0, total)
        if st not in (_abi.ZK_OK, _abi.ZK_ERR_CAPACITY):
            self._check(st)
        spans, services = np.zeros(total[0], TRACE_SPAN), np.zeros(total[1], np.uint32)
        if st == _abi.ZK_ERR_CAPACITY:
            self._check(self._L.zk_sp_traces(self._h, ptr, n, flags, heads.ctypes.data, spans.ctypes.data, len(spans),
                                             services.ctypes.data, len(services), total))
        return heads, spans, services

    def _combos_on_device(self, ids) -> List[TraceCombo]:
        """getTraceCombosByIds from traces(): spans, summary and depths of a trace from one answer. Names and
        services go through the dictionaries as in Trace._name and Trace._service. The Span and SpanTimestamp
        tuples of a whole chunk are built column by column; per trace only slices are taken. The cyclic
        collector is paused meanwhile: the tuples cannot form cycles, and at 4096 ids its passes over the
        growing lists were two thirds of the call."""
        out: List[TraceCombo] = []
        paused = gc.isenabled()
        gc.disable()
        try:
            for part in self._chunks(ids):
                self._combos_of(out, *self.traces(part))
        finally:
            if paused:
                gc.enable()
        return out

    def _combos_of(self, out: List[TraceCombo], heads, spans, services, rows=None, annotations=None, decoder=None,
                   lists: bool = True, timelines: bool = True) -> None:
        """The TraceCombos of one traces() answer, appended to out. With rows (and annotations, the store they
        came from): of one TraceAnnotationStore.adjusted_traces() answer, whose heads and spans carry the same
        field names; every span is then an AnnotatedSpan with its list, and the timeline is filled. A caller
        that hands on only the timelines, or only the traces, saves the other's tuples (one per row each):
        lists=False leaves the spans' lists empty, timelines=False the timeline None."""
        namer = Trace((), self.services, self.span_names)
        svc = services.tolist() if self.services is None else [namer._service(i) for i in services.tolist()]
        names = spans["name"].tolist()
        if self.span_names is not None:
            names = [namer._name(i) for i in names]
        bits = spans["bits"]
        timed = (bits & _abi.ZK_SP_SPAN_TIMED) != 0
        timed_l = timed.tolist()
        sid = spans["span_id"].tolist()
        parent = [p if b else None for p, b in zip(spans["parent_id"].tolist(), ((bits & _abi.ZK_SP_SPAN_HAS_PARENT) != 0).tolist())]
        first = [v if t else None for v, t in zip(spans["first"].tolist(), timed_l)]
        last = [v if t else None for v, t in zip(spans["last"].tolist(), timed_l)]
        depth = spans["depth"].tolist()
        k = spans["services"].astype(np.int64)
        svc_end = np.cumsum(k)
        mine = [tuple(svc[a:b]) for a, b in zip((svc_end - k).tolist(), svc_end.tolist())]
        c = heads["spans"].astype(np.int64)
        merged = list(map(Span if rows is None else AnnotatedSpan, np.repeat(heads["trace_id"], c).tolist(), sid, parent, names, first,
                          last, mine))
        lines, line_at, over = None, None, _abi.ZK_SP_TR_OVERFLOW
        if rows is not None:
            over |= _abi.ZK_AN_ADJ_OVERFLOW
            lines, line_at = self._annotate_merged(merged, heads, spans, rows, parent, names, decoder, lists, timelines)
        # one SpanTimestamp per (span, service) pair of a timed span, in the pairs' order
        pair_span = np.repeat(np.arange(len(spans)), k)
        keep = timed[pair_span]
        pair_span = pair_span[keep]
        stamps = list(map(SpanTimestamp, [svc[i] for i in np.nonzero(keep)[0].tolist()],
                          spans["first"][pair_span].tolist(), spans["last"][pair_span].tolist()))
        stamp_at = np.concatenate(([0], np.cumsum(np.where(timed, k, 0)))).tolist()
        at = 0
        for q, (tid, start, end, root, _, n_spans, _, state, *_) in enumerate(heads.tolist()):
            if state & over:  # a trace too long for the device merge: the host path
                if rows is None:
                    out += self.getTraceCombosByIds([tid])
                else:
                    out += self._combos_on_host([tid], ("TIME_SKEW",), annotations, decoder)  # (whole: one trace)
                continue
            if not state & _abi.ZK_SP_TR_FOUND:
                continue
            to = at + n_spans
            depths = {i: d for i, d in zip(sid[at:to], depth[at:to]) if d}
            summary = None
            if state & _abi.ZK_SP_TR_TIMED:
                summary = TraceSummary(tid, start, end, _to_int(_wrap64(end - start)), stamps[stamp_at[at]:stamp_at[to]], [])
            trace, timeline = Trace.of_merged(merged[at:to], root, depths), None
            if rows is not None:
                trace.annotations = {s.id: s.annotations for s in trace.spans}
                if timelines:
                    timeline = TraceTimeline(tid, root, lines[line_at[q]:line_at[q + 1]], [])
            out.append(TraceCombo(trace, summary, timeline, depths))
            at = to

    def _annotate_merged(self, merged, heads, spans, rows, parent, names, decoder, lists=True, timelines=True):
        """Every AnnotatedSpan of `merged` gets its list from `rows` (an adjusted_traces() answer: per span, in
        the spans' order, the span's annotations in list order). Returns the chunk's TimelineAnnotations, every
        trace's sorted by ts, and where each asked id's begin. The emitted order is TraceTimeline.of's order
        before its sort, so one stable sort over (asked index, ts) gives all timelines at once."""
        bits = rows.bits
        kind = bits & _abi.ZK_AN_KIND_MASK
        hosted = (bits & _abi.ZK_AN_HAS_HOST) != 0
        port = bits >> _abi.ZK_AN_PORT_SHIFT
        k = spans["rows"].astype(np.int64)
        if lists:
            ends = list(map(Endpoint, rows.ipv4.tolist(), port.tolist(), rows.service_id.tolist()))
            anns = list(map(Annotation, rows.ts.tolist(), rows.value.tolist(), kind.tolist(),
                            [e if h else None for e, h in zip(ends, hosted.tolist())]))
            row_end = np.cumsum(k)
            for s, a, b in zip(merged, (row_end - k).tolist(), row_end.tolist()):
                s.annotations = anns[a:b]
        else:
            for s in merged:
                s.annotations = []
        if not timelines:
            return None, None
        # the timelines: a stable sort by (asked index, ts)
        per_trace = heads["rows"].astype(np.int64)
        order = np.lexsort((rows.ts, np.repeat(np.arange(len(heads)), per_trace)))
        of_span = np.repeat(np.arange(len(spans)), k)[order]
        kind_o, hosted_o = kind[order], hosted[order]
        value = rows.value[order].tolist()
        if decoder is not None:
            value = [KIND_NAMES[c] if c else decoder.string(v) for v, c in zip(value, kind_o.tolist())]
        svc = np.where(hosted_o, rows.service_id[order], 0).tolist()
        if self.services is not None:
            if svc and max(svc) >= len(self.services):
                raise ValueError("a service id beyond the services dictionary")
            svc = [self.services[i] if h else "Unknown" for i, h in zip(svc, hosted_o.tolist())]
        span_of = of_span.tolist()
        lines = list(map(TimelineAnnotation, rows.ts[order].tolist(), value, np.where(hosted_o, rows.ipv4[order], 0).tolist(),
                         np.where(hosted_o, port[order], 0).tolist(), svc, spans["span_id"][of_span].tolist(),
                         [parent[i] for i in span_of], [names[i] for i in span_of]))
        return lines, np.concatenate(([0], np.cumsum(per_trace))).tolist()

    def _host_only(self, on_device: bool, adjust, annotations) -> bool:
        """Whether a call goes the host's way: always with an annotation store (the adjusters and the
        timeline are built on the host). on_device together with TIME_SKEW is refused, not ignored."""
        adjust = self._adjusters(adjust, annotations)
        if on_device and "TIME_SKEW" in adjust:
            raise ValueError("TIME_SKEW is adjusted on the host: on_device=True cannot be combined with it")
        return annotations is not None or not on_device

    def getTraceCombosByIds(self, ids, on_device: bool = False, adjust: Sequence[str] = (), annotations=None,
                            adjust_on_device: bool = False, binary=None, decoder=None) -> List[TraceCombo]:
        """QueryService.getTraceCombosByIds: one TraceCombo (the trace, its summary, its timeline, its span
        depths) per asked id that was found, in the order asked; summary is None for a trace without a timed
        fragment. on_device: spans, summary and depths are merged on the device (zk_sp_traces) and no
        fragment crosses to the host; the answer is the same. adjust, annotations: as for getTracesByIds;
        with an annotation store the host path is used and timeline is filled, without one it is None.
        adjust_on_device: with an annotation store, the adjuster, the spans' lists and the depths come from
        the device too (zk_an_adjusted_traces; the rules of getTraceSummariesByIds' adjust_on_device). The
        answer is the host path's, with ONE difference: Trace.rows is None, as with Trace.of_merged.
        binary: a TraceBinaryAnnotationStore; on every path the traces then carry their binary annotations
        and a timeline's binary_annotations is filled (resolved through decoder= and the services
        dictionary). decoder: turns a timeline's values into text, as in getTraceTimelinesByIds."""
        if binary is not None:
            return self._combos_with_binary(self.getTraceCombosByIds(ids, on_device, adjust, annotations, adjust_on_device,
                                                                     decoder=decoder), binary, decoder)
        if adjust_on_device:
            self._adjust_on_device(adjust, annotations, on_device)
            return self._combos_adjusted_on_device(ids, annotations, decoder)
        if not self._host_only(on_device, adjust, annotations):
            return self._combos_on_device(ids)
        if annotations is None:
            return [TraceCombo.of(t) for t in self.getTracesByIds(ids, adjust, annotations)]
        return self._combos_on_host(ids, adjust, annotations, decoder)

    def _summaries_adjusted_on_device(self, ids, annotations) -> List[TraceSummary]:
        """getTraceSummariesByIds(adjust=("TIME_SKEW",), annotations=) from annotations.adjusted_summaries():
        _summaries_on_device's loop over zk_an_adjusted_summaries' answer; a trace above the device's bounds
        goes the host's way. The cyclic collector is paused while the tuples are built, as in _combos_on_device."""
        out: List[TraceSummary] = []
        paused = gc.isenabled()
        gc.disable()
        try:
            for a in range(0, len(ids), _abi.ZK_AN_MAX_IDS):
                self._adjusted_of(out, annotations, *annotations.adjusted_summaries(self, ids[a:a + _abi.ZK_AN_MAX_IDS]))
        finally:
            if paused:
                gc.enable()
        return out

    def _adjusted_of(self, out: List[TraceSummary], annotations, heads, cols) -> None:
        """The TraceSummaries of one adjusted_summaries() answer, appended to out."""
        low = None if self.services is None else [s.lower() for s in self.services]
        svc, first, last = (cols[k].tolist() for k, _ in ENTRY_COLUMNS)
        if low is not None:
            if svc and max(svc) >= len(low):
                raise ValueError("a service id beyond the services dictionary")
            svc = [low[i] for i in svc]
        entries = list(map(SpanTimestamp, svc, first, last))
        at = 0
        for tid, start, end, _, _, c, state in heads.tolist():
            if state & _abi.ZK_AN_ADJ_OVERFLOW:
                out += self.getTraceSummariesByIds([tid], adjust=("TIME_SKEW",), annotations=annotations)
            elif state & _abi.ZK_SP_SUM_TIMED:
                out.append(TraceSummary(tid, start, end, _to_int(_wrap64(end - start)), entries[at:at + c], []))
            at += c

    def getTraceSummariesByIds(self, ids, on_device: bool = False, adjust: Sequence[str] = (), annotations=None,
                               adjust_on_device: bool = False) -> List[TraceSummary]:
        """QueryService.getTraceSummariesByIds: the summaries in the order asked; ids that are not found
        and traces without a timed fragment (TraceSummary.apply yields None) are left out. on_device:
        the summaries are merged on the device (zk_sp_summaries) and only they cross to the host; the
        answer is the same. adjust, annotations: as for getTracesByIds; with an annotation store the host
        path is used, unless adjust_on_device: then the adjuster runs on the device too
        (zk_an_adjusted_summaries) and only the adjusted summaries cross; the answer is the same. It needs
        annotations= and "TIME_SKEW" as the only adjuster besides "NOTHING", once; anything else is a
        ValueError."""
        if adjust_on_device:
            self._adjust_on_device(adjust, annotations, on_device)
            return self._summaries_adjusted_on_device(np.ascontiguousarray(np.asarray(ids, dtype=np.uint64)), annotations)
        if not self._host_only(on_device, adjust, annotations):
            return self._summaries_on_device(ids)
        return [s for s in (TraceSummary.of(t) for t in self.getTracesByIds(ids, adjust, annotations)) if s is not None]

    # ---- timing ----------------------------------------------------------------------------------------
    def observe_ms(self) -> dict:
        """Device time (ms) of the passes of the last observe (zk_sp_observe_ms; timing=True)."""
        out = (C.c_double * len(self.OBSERVE_PHASES))()
        self._check(self._L.zk_sp_observe_ms(self._h, out))
        return dict(zip(self.OBSERVE_PHASES, out))

    def expire_ms(self) -> dict:
        """Device time (ms) of the passes of the last expire that ran one (zk_sp_expire_ms; timing=True)."""
        out = (C.c_double * len(self.EXPIRE_PHASES))()
        self._check(self._L.zk_sp_expire_ms(self._h, out))
        return dict(zip(self.EXPIRE_PHASES, out))

    def query_ms(self) -> float:
        """Time (ms) on the handle's stream of the last exist, gather, summaries or traces (zk_sp_query_ms;
        timing=True)."""
        ms = C.c_double()
        self._check(self._L.zk_sp_query_ms(self._h, C.byref(ms)))
        return float(ms.value)
