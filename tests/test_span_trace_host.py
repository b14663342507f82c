"""Merged traces without a device: the golden traces of tests/golden/trace_combos.json through the host
classes (Trace, TraceSummary, TraceCombo) and through the model of zk_sp_traces' output (tests/sptraceref.py),
the host Trace against tests/spref.py's own restatement on random traces, getRootSpans, a Trace from merged
spans, zk_sp_traces' refusals that need no device, and the binding's layouts. Every comparison is exact."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

from tests import spref as R
from tests import sptraceref as M
from zipkin_amd import TRACE_HEAD, TRACE_SPAN, Span, Trace, TraceCombo, TraceSummary, _abi

HEADER = (Path(__file__).resolve().parent.parent / "include" / "zkspans.h").read_text()
U64 = 2 ** 64 - 1


def pairs(d):
    return None if d is None else sorted(d.items())


def test_golden_through_the_host_classes():
    g = M.golden()
    assert "QueryServiceSpec.scala:186" in g["cases"][0]["follows"]
    for case in g["cases"]:
        rows, want = R.golden_rows(case, g["services"]), case["expect"]
        t = Trace(rows, g["services"], g["span_names"])
        c = TraceCombo.of(t)
        assert c.trace is t and c.timeline is None, case["name"]
        assert [s.id for s in t.spans] == want["span_order"], case["name"]
        root = t.getRootMostSpan()
        assert (None if root is None else root.id) == want["root_most"], case["name"]
        assert pairs(c.span_depths) == (None if want["depths"] is None else sorted(map(tuple, want["depths"]))), case["name"]
        assert [s.id for s in t.getRootSpans()] == want["root_spans"], case["name"]
        s = want["summary"]
        assert c.summary == (None if s is None else TraceSummary(s[0], s[1], s[2], s[3], [tuple(x) for x in s[4]], [])), case["name"]
        assert c.summary == TraceSummary.of(t)


def test_golden_through_the_model():
    g = M.golden()
    for case in g["cases"]:
        rows, want = R.golden_rows(case, g["services"]), case["expect"]
        head, spans, services = M.one(case["trace_id"], rows, _abi.ZK_SP_TRACE_MAX_ROWS)
        if not rows:
            assert (head, spans, services) == (M.ZERO, [], [])
            continue
        assert head[0] == case["trace_id"] and head[3] == want["root_most"] and head[4:7] == (len(rows), len(spans), len(services))
        assert [s[0] for s in spans] == want["span_order"]
        assert sorted((s[0], s[5]) for s in spans if s[5]) == sorted(map(tuple, want["depths"]))
        assert [s[0] for s in spans if s[7] & M.ROOT_MOST] == [want["root_most"]]
        assert [s[0] for s in spans if not s[7] & M.PARENT_FOUND] == want["root_spans"]
        assert sum(s[6] for s in spans) == len(services)
        summ = want["summary"]
        assert bool(head[7] & M.TIMED) == (summ is not None)
        if summ is not None:
            assert head[1:3] == (summ[1], summ[2])
            at, got = 0, []
            for s in spans:
                got += [[g["services"][v], s[2], s[3]] for v in services[at:at + s[6]] if s[7] & M.SPAN_TIMED]
                at += s[6]
            assert got == summ[4]


def random_rows(rng, tid, n, k):
    """n rows over k span ids from the unsigned order's corners first, parents from the same few ids (so
    that parents hit, chains close on themselves and spans parent themselves) and 7 (never a span)."""
    spans = [0, 1, 2 ** 63, U64, 5, 6, 8, 9][:k]
    rows = []
    for _ in range(n):
        fl = int(rng.integers(0, 16)) | (int(rng.integers(0, 3)) << R.NAME_SHIFT)
        rows.append((tid, spans[int(rng.integers(k))], (spans + [7])[int(rng.integers(k + 1))], int(rng.integers(-3, 4)),
                     int(rng.integers(-3, 4)), int(rng.integers(3)), fl))
    return rows


def test_host_trace_against_the_restatement():
    """Trace (the device call's stated semantics) and tests/spref.py (written apart from it) agree on spans,
    root-most span and depths, cycles and self-parents included; depth = 1 + the parent hops to the root-most
    span, whatever the root-most span's own parent is."""
    rng = np.random.default_rng(1)
    shapes = set()
    for i in range(400):
        rows = random_rows(rng, 9, int(rng.integers(1, 12)), int(rng.integers(1, 7)))
        t = Trace(rows)
        want = R.trace(rows)
        assert [(s.id, s.parent, s.name, s.first, s.last, list(s.services)) for s in t.spans] == \
            [(s["id"], s["parent"], s["name"], s["first"], s["last"], s["services"]) for s in want]
        root = t.getRootMostSpan()
        assert root.id == R.root_most(rows)["id"]
        depths = t.toSpanDepths()
        assert depths == R.span_depths(rows) and depths[root.id] == 1
        by = t.getIdToSpanMap()
        for s in t.spans:  # the header's rule, hop by hop
            hops, at, seen = 0, s, set()
            while at.id != root.id and at.parent in by and at.id not in seen:
                seen.add(at.id)
                at, hops = by[at.parent], hops + 1
            assert depths.get(s.id, 0) == (hops + 1 if at.id == root.id else 0)
        assert [s.id for s in t.getRootSpans()] == [s.id for s in t.spans if s.parent is None or s.parent not in by]
        shapes.add((t.getRootSpan() is None, len(depths) < len(t.spans), root.parent in by))
    assert len(shapes) >= 6  # with and without a parentless span, with spans outside the tree, a root-most span on a cycle


def test_parent_and_name_rules():
    HP, T = R.HAS_PARENT, R.TIMED
    name = lambda i: i << R.NAME_SHIFT  # noqa: E731
    # the parent: the least parent id among the fragments with the bit; U64 and 0 are parents, no bit is none
    t = Trace([(1, 5, U64, 0, 0, 0, HP), (1, 5, 3, 0, 0, 0, 0), (1, 6, 0, 0, 0, 0, HP), (1, 7, 9, 0, 0, 0, 0), (1, U64, 0, 0, 0, 0, 0)])
    assert [(s.id, s.parent) for s in t.spans] == [(5, U64), (6, 0), (7, None), (U64, None)]
    assert t.toSpanDepths() == {7: 1} and [s.id for s in t.getRootSpans()] == [6, 7, U64]
    # the name: the first named fragment by (parent_id, first_ts, last_ts, service_id, flags), an untimed
    # fragment's raw first_ts included
    assert Trace([(1, 5, 2, 0, 0, 0, name(7)), (1, 5, 1, 9, 9, 9, name(8))]).spans[0].name == 8
    assert Trace([(1, 5, 1, 4, 0, 0, name(7)), (1, 5, 1, 3, 0, 0, name(8)), (1, 5, 1, 2, 0, 0, 0)]).spans[0].name == 8
    assert Trace([(1, 5, 1, 3, 0, 0, name(8)), (1, 5, 1, 3, 0, 0, name(7) | T), (1, 5, 1, 3, 0, 0, T)]).spans[0].name == 7


def test_a_trace_from_merged_spans():
    spans = [Span(4, 10, None, 1, 5, 9, (2,)), Span(4, 11, 10, 0, None, None, ())]
    t = Trace.of_merged(spans, 11, {11: 1})
    assert t.rows is None and t.spans == spans and t.id == 4
    assert t.getRootMostSpan() == spans[1] and t.toSpanDepths() == {11: 1}  # what was given, not what the spans say
    assert t.getRootSpan() == spans[0] and [s.id for s in t.getRootSpans()] == [10]
    assert t.serviceCounts() == {2: 1} and TraceSummary.of(t) == TraceSummary(4, 5, 9, 4, [(2, 5, 9)], [])
    assert Trace.of_merged([], None, None).toSpanDepths() is None


def test_trace_combo():
    assert TraceCombo._fields == ("trace", "summary", "timeline", "span_depths")
    c = TraceCombo.of(Trace([(3, 1, 0, 0, 0, 0, 0)]))
    assert c.summary is None and c.timeline is None and c.span_depths == {1: 1}


def test_refusals_without_a_device():
    L = _abi.lib()
    ids, heads, n_out = np.zeros(1, np.uint64), np.zeros(1, TRACE_HEAD), (C.c_uint64 * 2)(7, 7)
    assert L.zk_sp_traces(None, ids.ctypes.data, 1, 0, heads.ctypes.data, None, 0, None, 0, n_out) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_sp_traces(None, ids.ctypes.data, 1, 0, heads.ctypes.data, None, 0, None, 0, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_sp_traces(None, None, 0, 0, None, None, 0, None, 0, None) == _abi.ZK_ERR_INVALID_ARG
    assert list(n_out) == [7, 7]
    assert L.zk_abi_version() == 3


def test_layouts_and_constants():
    for dt, st in ((TRACE_HEAD, _abi.zk_sp_trace), (TRACE_SPAN, _abi.zk_sp_span)):
        assert dt.itemsize == C.sizeof(st) == 48
        assert [(k, dt.fields[k][1], dt.fields[k][0].itemsize) for k in dt.names] == \
            [(k, getattr(st, k).offset, getattr(st, k).size) for k, _ in st._fields_]
    assert TRACE_HEAD.names == M.HEAD and TRACE_SPAN.names == M.SPAN
    for name in ("ZK_SP_TRACE_MAX_ROWS", "ZK_SP_TR_FOUND", "ZK_SP_TR_TIMED", "ZK_SP_TR_OVERFLOW", "ZK_SP_SPAN_HAS_PARENT",
                 "ZK_SP_SPAN_TIMED", "ZK_SP_SPAN_PARENT_FOUND", "ZK_SP_SPAN_ROOT_MOST"):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)u", HEADER)
        assert m and int(m.group(1)) == getattr(_abi, name), name
    assert _abi.ZK_SP_TRACE_MAX_ROWS == _abi.ZK_SP_SUM_MAX_ROWS
    assert (_abi.ZK_SP_TR_FOUND, _abi.ZK_SP_TR_TIMED, _abi.ZK_SP_TR_OVERFLOW) == \
        (_abi.ZK_SP_SUM_FOUND, _abi.ZK_SP_SUM_TIMED, _abi.ZK_SP_SUM_OVERFLOW)
    assert (M.FOUND, M.TIMED, M.OVERFLOW) == (_abi.ZK_SP_TR_FOUND, _abi.ZK_SP_TR_TIMED, _abi.ZK_SP_TR_OVERFLOW)
    assert (M.HAS_PARENT, M.SPAN_TIMED, M.PARENT_FOUND, M.ROOT_MOST) == \
        (_abi.ZK_SP_SPAN_HAS_PARENT, _abi.ZK_SP_SPAN_TIMED, _abi.ZK_SP_SPAN_PARENT_FOUND, _abi.ZK_SP_SPAN_ROOT_MOST)
