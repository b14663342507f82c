"""Time-skew-adjusted trace summaries on the device (zk_an_adjusted_summaries, include/zkannots.h) against
tests/tsaref.py: summary(adjust(annotated(spans, anns)), tid), with the product's host path beside it. Every
comparison is exact equality, the entries' order included; through the raw call no case below the bounds may
carry ZK_AN_ADJ_OVERFLOW, so none passes by the host fallback."""
import ctypes as C

import numpy as np
import pytest

from tests import anref as A
from tests import spref as S
from tests import tsaref as T
from zipkin_amd import AnnotationRows, DeviceAnnotationRows, DeviceColumns, TraceAnnotationStore, TraceSpanStore, ZkError, _abi
from zipkin_amd.spanstore import ENTRY_COLUMNS, SUMMARY_HEAD

pytestmark = pytest.mark.gpu

SKEW = ("TIME_SKEW",)
U64 = 2 ** 64 - 1
FOUND, TIMED = _abi.ZK_SP_SUM_FOUND, _abi.ZK_SP_SUM_TIMED
ANNOTATED, OVERFLOW = _abi.ZK_AN_ADJ_ANNOTATED, _abi.ZK_AN_ADJ_OVERFLOW
MAX_ROWS, MAX_FRAGMENTS, WAVE = _abi.ZK_AN_ADJ_MAX_ROWS, _abi.ZK_SP_TRACE_MAX_ROWS, _abi.ZK_AN_ADJ_WAVE_ROWS
IP_A, IP_B, IP_C = 167772161, 167772162, 167772163
SENTINEL = 0xA5


class World:
    """Traces as (span rows, annotation rows) by trace id, fed to both stores shuffled, in three observes each."""

    def __init__(self):
        self.traces, self._judged = {}, {}

    def add(self, tid, span_rows, ann_rows):
        assert tid not in self.traces
        self.traces[tid] = (list(span_rows), list(ann_rows))

    def add_case(self, case):
        self.add(case["trace_id"], *T.golden_rows(case))

    def feed(self, spans, annots, seed=1, parts=3):
        span_rows = [r for s, _ in self.traces.values() for r in s]
        ann_rows = [r for _, a in self.traces.values() for r in a]
        rng = np.random.default_rng(seed)
        for part in np.array_split(rng.permutation(len(span_rows)), parts):
            spans.observe(DeviceColumns.from_host(S.cols_of([span_rows[i] for i in part])))
        for part in np.array_split(rng.permutation(len(ann_rows)), parts):
            if len(part):
                annots.observe(DeviceAnnotationRows.from_host(AnnotationRows.of_rows([ann_rows[i] for i in part]), annots.device))

    def judge(self, tid):
        """(head, entries, summary) of an asked id as tests/tsaref.py has it."""
        if tid not in self.traces:
            return (0,) * 7, [], None
        if tid not in self._judged:
            self._judged[tid] = self._judge(tid)
        return self._judged[tid]

    def _judge(self, tid):
        s, a = self.traces[tid]
        model = T.annotated(s, a)
        if a:  # a trace without rows in the annotation store is not adjusted
            model = T.adjust(model)
        sm = T.summary(model, tid)
        entries = [] if sm is None else sm[4]
        state = FOUND | (TIMED if sm else 0) | (ANNOTATED if a else 0)
        head = (tid, sm[1] if sm else 0, sm[2] if sm else 0, len(s), len(model), len(entries), state)
        return head, entries, sm


def answers(heads, cols):
    """The raw call's answer per asked id: [(head tuple, [(service, first, last)])]."""
    ent = list(zip(*[cols[k].tolist() for k, _ in ENTRY_COLUMNS]))
    out, at = [], 0
    for h in heads.tolist():
        out.append((tuple(h), ent[at:at + h[5]]))
        at += h[5]
    assert at == len(ent)
    return out


def summary_tuple(s):
    return (s.trace_id, s.start, s.end, s.duration_micro, [tuple(x) for x in s.span_timestamps], s.endpoints)


def check(world, spans, annots, ids, overflowed=()):
    """The raw call, the product's device path and its host path against the judge, for the asked ids."""
    got = answers(*annots.adjusted_summaries(spans, ids))
    want = [world.judge(i) for i in ids]
    for i, (head, entries), (w_head, w_entries, _) in zip(ids, got, want):
        if i in overflowed:
            assert head == (i, 0, 0, w_head[3], 0, 0, FOUND | OVERFLOW | (w_head[6] & ANNOTATED)) and entries == []
        else:
            assert (head, entries) == (w_head, w_entries), f"trace {i}"
    sums = [w[2] for w in want if w[2] is not None]
    assert [summary_tuple(s) for s in spans.getTraceSummariesByIds(ids, adjust=SKEW, annotations=annots, adjust_on_device=True)] == sums
    assert [summary_tuple(s) for s in spans.getTraceSummariesByIds(ids, adjust=SKEW, annotations=annots)] == sums


@pytest.fixture()
def stores(gpu):
    with TraceSpanStore(device=gpu) as spans, TraceAnnotationStore(device=gpu) as annots:
        yield spans, annots


def span(sid, parent, anns):
    return {"id": sid, "parent": parent, "annotations": anns}


def rpc(t0, client, server, c_off=0, s_off=0, lat=5, work=20):
    """cs / sr / ss / cr of one call, each side on its own clock."""
    return [[t0 + c_off, "cs", client], [t0 + lat + s_off, "sr", server], [t0 + lat + work + s_off, "ss", server],
            [t0 + 2 * lat + work + c_off, "cr", client]]


# ---- 1. the hand-worked vectors ------------------------------------------------------------------------------
def test_golden_traces(stores):
    spans, annots = stores
    world = World()
    cases = T.golden()["cases"]
    assert len(cases) == 14
    for c in cases:
        world.add_case(c)
    world.feed(spans, annots, seed=12)
    ids = [c["trace_id"] for c in cases][::-1]
    ids = ids[:5] + [404] + ids[5:] + [ids[2]]  # reversed, a missing id, a duplicate
    check(world, spans, annots, ids)
    sums = spans.getTraceSummariesByIds(ids[:5], adjust=SKEW, annotations=annots, adjust_on_device=True)
    assert [[s.start, s.end] for s in sums] == [c["expect"]["start_end"] for c in cases][::-1][:5]


# ---- 2. seeded random traces -----------------------------------------------------------------------------------
def random_world(seed, n, max_spans):
    rng = np.random.default_rng(seed)
    world = World()
    for k in range(n):
        world.add_case(T.random_case(rng, 1000 + k, max_spans=int(rng.integers(1, max_spans + 1))))
    return world


def padded(tid, n_spans, n_rows):
    """A trace of n_spans spans under one root and exactly n_rows annotation rows: a skewed call per span, the
    rest free annotations of the root."""
    assert n_rows >= 4 * n_spans
    sp = [span(1, None, rpc(1000, IP_A, IP_B, s_off=300))]
    sp += [span(k + 1, 1 + (k - 1) // 2, rpc(1000 + 7 * k, IP_B if k % 2 else IP_C, IP_C if k % 2 else IP_A, s_off=-150 * (k % 3)))
           for k in range(1, n_spans)]
    sp[0]["annotations"] += [[1001 + j, "foo", IP_B] for j in range(n_rows - 4 * n_spans)]
    return {"trace_id": tid, "spans": sp}


def test_random_traces_and_the_work_lists_bound(stores):
    spans, annots = stores
    world = random_world(2024, 200, 64)
    # the second group straddles the wave / workgroup bound: rows, then spans, exactly at it and one above
    world.add_case(padded(5000, 16, WAVE))
    world.add_case(padded(5001, 16, WAVE + 1))
    world.add_case({"trace_id": 5002, "spans": [span(1, None, [[10, "cs", IP_A]])] + [span(k, k - 1, [[10 + k, "sr", IP_B]]) for k in range(2, WAVE + 1)]})
    world.add_case({"trace_id": 5003, "spans": [span(1, None, [[10, "cs", IP_A]])] + [span(k, k - 1, [[10 + k, "sr", IP_B]]) for k in range(2, WAVE + 2)]})
    # (on the CPU, from the cases alone) every trace stays under both bounds, and both work lists are used
    sizes = [(len(s), len(a)) for s, a in world.traces.values()]
    assert all(f <= MAX_FRAGMENTS and r <= MAX_ROWS for f, r in sizes)
    assert any(f <= WAVE and r <= WAVE for f, r in sizes) and any(r > WAVE for f, r in sizes)
    assert sorted(len(world.traces[t][1]) for t in (5000, 5001)) == [WAVE, WAVE + 1]
    assert sorted(len(world.traces[t][0]) for t in (5002, 5003)) == [WAVE, WAVE + 1]
    world.feed(spans, annots, seed=7)
    assert spans.info()["segments"] == 3 and annots.info()["segments"] == 3
    ids = list(world.traces)
    np.random.default_rng(3).shuffle(ids)
    heads, _ = annots.adjusted_summaries(spans, ids)
    assert not (heads["state"] & OVERFLOW).any() and (heads["state"] & FOUND).all()
    check(world, spans, annots, ids)


# ---- 3. shapes where the walk can go wrong -------------------------------------------------------------------
def shapes():
    world = World()
    ips = [IP_A, IP_B, IP_C]
    clock = {IP_A: 0, IP_B: 400, IP_C: -250}
    # a chain of 300 spans: the handed-down skew accumulates
    world.add_case({"trace_id": 1, "spans": [
        span(k + 1, k or None, rpc(1000 + 3 * k, ips[k % 3], ips[(k + 1) % 3], clock[ips[k % 3]], clock[ips[(k + 1) % 3]], lat=2, work=2000 - 6 * k))
        for k in range(300)]})
    # a star: a client-only root with 500 children, several without cs / cr, the first child's lead without a host
    kids = []
    for k in range(500):
        anns = rpc(2000 + k, IP_B, IP_C, c_off=700, s_off=-90)
        if k == 0:
            anns[0][2] = None  # the lead (the first child's first cs / cr) has no host
        if k % 7 == 3:
            anns = [a for a in anns if a[1] in ("sr", "ss")]
        if k % 11 == 5:
            anns = anns[:1]
        kids.append(span(10 + k, 1, anns))
    world.add_case({"trace_id": 2, "spans": [span(1, None, [[1900, "cs", IP_A], [4000, "cr", IP_A]])] + kids})
    # the same star with a hosted lead: every child with cs and cr is shifted by its own skew
    kids2 = [span(s["id"], 1, [list(a) for a in s["annotations"]]) for s in kids[:40]]
    kids2[0]["annotations"][0][2] = IP_B
    world.add_case({"trace_id": 3, "spans": [span(1, None, [[1900, "cs", IP_A], [4000, "cr", IP_A]])] + kids2})
    # no root; spans outside the root's tree (a second root, a parent that is no span, a cycle); a self-parent
    world.add_case({"trace_id": 4, "spans": [span(1, 2, rpc(100, IP_A, IP_B, s_off=50)), span(2, 1, rpc(90, IP_B, IP_C, s_off=-50)),
                                             span(3, 77, rpc(80, IP_A, IP_C, s_off=500))]})
    world.add_case({"trace_id": 5, "spans": [span(1, None, rpc(100, IP_A, IP_B, s_off=60)), span(2, 1, rpc(110, IP_B, IP_C, s_off=-30)),
                                             span(3, None, rpc(120, IP_A, IP_B, s_off=60)), span(4, 3, rpc(125, IP_B, IP_A)),
                                             span(5, 99, rpc(10, IP_B, IP_A)), span(6, 7, rpc(11, IP_B, IP_A)), span(7, 6, rpc(12, IP_B, IP_A)),
                                             span(8, 8, rpc(5, IP_A, IP_B, s_off=9)), span(9, 8, rpc(6, IP_A, IP_B))]})
    # a span without rows under an adjusted parent, and under it an adjusted one; equal timestamps, different hosts
    world.add_case({"trace_id": 6, "spans": [span(1, None, rpc(100, IP_A, IP_B, s_off=300)), span(2, 1, []),
                                             span(3, 2, rpc(104, IP_B, IP_C, c_off=300, s_off=-40)),
                                             span(4, 1, [[100, "cs", IP_B], [100, "cs", IP_A], [100, "sr", IP_C], [100, "sr", IP_A],
                                                         [130, "ss", IP_C], [130, "ss", IP_B], [130, "cr", IP_A], [130, "cr", IP_B]])]})
    # annotation rows for a span id the span store lacks; an untimed record whose span has rows
    s7, a7 = T.golden_rows({"trace_id": 7, "spans": [span(1, None, rpc(100, IP_A, IP_B, s_off=80)), span(2, 1, rpc(110, IP_B, IP_C, c_off=80))]})
    a7 += [(7, 55, 1, T.fnv_mix(b"cs"), IP_A, 1, A.CS | A.HAS_HOST), (7, 0, 5000, T.fnv_mix(b"x"), 0, 0, 0)]
    s7 = [r if r[1] != 2 else r[:3] + (7, 9, r[5], r[6] & ~S.TIMED) for r in s7] + [(7, 3, 1, 123, 456, 9, S.HAS_PARENT | S.SVC_SERVER)]
    a7 += [(7, 3, 140, T.fnv_mix(b"sr"), IP_B, 2, A.SR | A.HAS_HOST), (7, 3, 150, T.fnv_mix(b"ss"), IP_B, 2, A.SS | A.HAS_HOST)]
    world.add(7, s7, a7)
    # trace ids 0 and 2^64 - 1; ts at INT64_MIN and INT64_MAX (the skew wraps)
    lo, hi = S.INT64_MIN, S.INT64_MAX
    world.add_case({"trace_id": 0, "spans": [span(0, None, rpc(100, IP_A, IP_B, s_off=-70)), span(U64, 0, rpc(105, IP_B, IP_A, c_off=-70))]})
    world.add_case({"trace_id": U64, "spans": [span(1, None, [[lo, "cs", IP_A], [hi, "sr", IP_B], [hi, "ss", IP_B], [lo + 10, "cr", IP_A]]),
                                               span(2, 1, [[hi, "cs", IP_B], [lo, "sr", IP_C], [lo + 1, "ss", IP_C], [hi, "cr", IP_B]]),
                                               span(3, 2, [[lo, "foo", IP_C], [hi, "bar", IP_C]])]})
    return world


def test_shapes_of_the_walk(stores):
    spans, annots = stores
    world = shapes()
    assert all(len(s) <= MAX_FRAGMENTS and len(a) <= MAX_ROWS for s, a in world.traces.values())
    world.feed(spans, annots, seed=5)
    ids = [U64, 0, 7, 6, 5, 4, 3, 2, 1]
    heads, _ = annots.adjusted_summaries(spans, ids)
    assert not (heads["state"] & OVERFLOW).any()
    check(world, spans, annots, ids)
    # the cases are what they claim: the chain's skew reaches its end, pruning happens, the no-root trace keeps all
    by = dict(zip(ids, heads.tolist()))
    assert by[1][4] == 300 and by[2][4] == 501 and by[4][4] == 3 and by[5][4] == 2 and by[7][4] == 3
    plain = T.summary(T.annotated(*world.traces[1]), 1)
    assert world.judge(1)[2][4] != plain[4]


# ---- 4. the bounds -----------------------------------------------------------------------------------------------
def test_the_row_bound(stores):
    spans, annots = stores
    world = World()
    world.add_case(padded(11, 400, MAX_ROWS))
    world.add_case(padded(12, 400, MAX_ROWS + 1))
    assert [len(world.traces[t][1]) for t in (11, 12)] == [MAX_ROWS, MAX_ROWS + 1]
    world.feed(spans, annots, seed=2)
    heads, _ = annots.adjusted_summaries(spans, [11, 12])
    assert [int(s) & OVERFLOW for s in heads["state"]] == [0, OVERFLOW]
    check(world, spans, annots, [12, 11, 404], overflowed={12})


def test_the_fragment_bound(stores):
    spans, annots = stores
    world = World()
    for tid, extra in ((21, 0), (22, 1)):
        s, a = T.golden_rows(padded(tid, 1024, 4 * 1024))
        a = [r for r in a if r[1] <= 256]  # rows for a quarter of the spans: the others keep their record times
        s = s + [r[:3] + (r[3] - 1, r[4] + 1) + r[5:] for r in s]  # every span in two fragments
        world.add(tid, s + s[:extra], a)
    assert [len(world.traces[t][0]) for t in (21, 22)] == [MAX_FRAGMENTS, MAX_FRAGMENTS + 1]
    world.feed(spans, annots, seed=4)
    heads, _ = annots.adjusted_summaries(spans, [21, 22])
    assert [int(s) & OVERFLOW for s in heads["state"]] == [0, OVERFLOW]
    check(world, spans, annots, [21, 22], overflowed={22})


def test_both_bounds_at_once(stores):
    """The kernel's largest launch: 2048 merged spans (one fragment each) beside exactly 2048 rows, 159,808 B of
    LDS in one workgroup, span and row numbers up to 2047 in the 16-bit fields."""
    spans, annots = stores
    world = World()
    s, a = T.golden_rows(padded(31, MAX_FRAGMENTS, 4 * MAX_FRAGMENTS))
    a = [r for r in a if r[1] % 4 == 1]  # rows for every fourth span, up and down the tree: the others keep their record times
    world.add(31, s, a)
    assert (len(s), len({r[1] for r in s}), len(a)) == (MAX_FRAGMENTS, MAX_FRAGMENTS, MAX_ROWS)
    world.feed(spans, annots, seed=8)
    heads, _ = annots.adjusted_summaries(spans, [31])
    assert heads.tolist()[0][3:] == (MAX_FRAGMENTS, MAX_FRAGMENTS, MAX_FRAGMENTS, FOUND | TIMED | ANNOTATED)
    check(world, spans, annots, [31])


def test_query_ms_after_a_call_without_an_adjust_pass(gpu):
    with TraceSpanStore(device=gpu, timing=True) as spans, TraceAnnotationStore(device=gpu, timing=True) as annots:
        world = random_world(5, 4, 8)
        world.feed(spans, annots, seed=1, parts=1)
        ids = list(world.traces)
        annots.adjusted_summaries(spans, ids)
        assert annots.query_ms() > 0 and spans.query_ms() > 0
        heads, cols = annots.adjusted_summaries(spans, [404, 405])  # nothing is found: no pass of this handle runs
        assert not heads["state"].any() and len(cols["first"]) == 0
        with pytest.raises(ZkError):
            annots.query_ms()  # never an earlier call's time
        annots.gather(ids)
        assert annots.query_ms() > 0


# ---- 5. absent traces and sizing -------------------------------------------------------------------------------
def raw(annots, spans, ids, cap, flags=0, ptr=None):
    """zk_an_adjusted_summaries into sentinel-filled columns of `cap` entries: (status, n_out, heads, columns)."""
    ids = np.ascontiguousarray(np.asarray(ids, np.uint64))
    heads = np.frombuffer(bytes([SENTINEL]) * (max(len(ids), 1) * SUMMARY_HEAD.itemsize), SUMMARY_HEAD).copy()
    cols = {k: np.frombuffer(bytes([SENTINEL]) * (max(cap, 1) * np.dtype(dt).itemsize), dt).copy() for k, dt in ENTRY_COLUMNS}
    out = _abi.zk_sp_span_ts(*[cols[k].ctypes.data for k, _ in ENTRY_COLUMNS])
    total = C.c_uint64(12345)
    st = annots._L.zk_an_adjusted_summaries(annots._h, spans._h, ids.ctypes.data if ptr is None else ptr, len(ids), flags,
                                            heads.ctypes.data, C.byref(out), cap, C.byref(total))
    return st, int(total.value), heads[:len(ids)], cols


def test_absent_traces_sizing_and_device_ids(stores, gpu):
    import torch

    spans, annots = stores
    world = random_world(77, 12, 24)
    bare = random_world(78, 6, 24)  # the same kind of traces, with nothing in the annotation store
    for k, (tid, (s, a)) in enumerate(bare.traces.items()):
        world.add(3000 + k, [(3000 + k,) + r[1:] for r in s], [])
    ids = list(world.traces) + [404]
    world.feed(spans, annots, seed=9, parts=1)
    # an empty annotation store: zk_sp_summaries' own answer
    with TraceAnnotationStore(device=gpu) as empty:
        h0, c0 = empty.adjusted_summaries(spans, ids)
        h1, c1 = spans.summaries(ids)
        assert h0.tolist() == h1.tolist() and all((c0[k] == c1[k]).all() for k, _ in ENTRY_COLUMNS)
    # a trace absent from the annotation store equals zk_sp_summaries' head and entries
    got = answers(*annots.adjusted_summaries(spans, ids))
    plain = answers(*spans.summaries(ids))
    for i, g, p in zip(ids, got, plain):
        if i >= 3000:
            assert g == p
    check(world, spans, annots, ids)
    # the sizing contract
    total = sum(len(e) for _, e in got)
    assert total > 4
    st, n_out, heads, cols = raw(annots, spans, ids, total - 1)
    assert st == _abi.ZK_ERR_CAPACITY and n_out == total and [tuple(h) for h in heads.tolist()] == [h for h, _ in got]
    assert all((c.view(np.uint8) == SENTINEL).all() for c in cols.values())
    st, n_out, heads, cols = raw(annots, spans, ids, total + 3)
    assert st == _abi.ZK_OK and n_out == total
    assert list(zip(*[cols[k][:total].tolist() for k, _ in ENTRY_COLUMNS])) == [e for _, es in got for e in es]
    assert all((c[total:].view(np.uint8) == SENTINEL).all() for c in cols.values())
    # more than ZK_AN_MAX_IDS ids; the product chunks
    many = np.zeros(_abi.ZK_AN_MAX_IDS + 1, np.uint64)
    assert raw(annots, spans, many, 0)[0] == _abi.ZK_ERR_INVALID_ARG
    rep = (ids * (_abi.ZK_AN_MAX_IDS // len(ids) + 2))[:_abi.ZK_AN_MAX_IDS + 5]
    want = [world.judge(i)[2] for i in rep]
    assert [summary_tuple(s) for s in spans.getTraceSummariesByIds(rep, adjust=SKEW, annotations=annots, adjust_on_device=True)] == \
        [w for w in want if w is not None]
    # device-pointer ids
    dev = torch.from_numpy(np.array(ids, np.uint64).view(np.int64)).to(f"cuda:{gpu}")
    assert answers(*annots.adjusted_summaries(spans, dev)) == got


# ---- 6. the stagings are shared, not corrupted ---------------------------------------------------------------
def test_the_other_calls_answer_as_before(stores):
    spans, annots = stores
    world = random_world(31, 40, 48)
    world.feed(spans, annots, seed=6)
    ids = list(world.traces)[::-1] + [404]

    def others():
        th, ts, tv = spans.traces(ids)
        sh, sc = spans.summaries(ids)
        counts, rows = annots.gather(ids)
        return (th.tolist(), ts.tolist(), tv.tolist(), sh.tolist(), [sc[k].tolist() for k, _ in ENTRY_COLUMNS], counts.tolist(), rows.rows())

    before = others()
    first = answers(*annots.adjusted_summaries(spans, ids))
    assert others() == before
    assert answers(*annots.adjusted_summaries(spans, ids)) == first
    assert annots.getAnnotationsByTraceIds(ids) == A.by_trace_ids([r for _, a in world.traces.values() for r in a], ids)
