"""Time-skew-adjusted traces on the device (zk_an_adjusted_traces, include/zkannots.h) against tests/tsaref.py
through tests/tsatraceref.py: the RAW call's heads, spans, services and rows are compared bit for bit, so a
Python fallback cannot hide a device error, and no trace below the bounds may carry ZK_AN_ADJ_OVERFLOW. The
three Python entry points are then compared with their host paths."""
import numpy as np
import pytest

from tests import anref as A
from tests import spref as S
from tests import tsaref as T
from tests import tsatraceref as X
from tests.tsatraceref import ANNOTATED, FOUND, MAX_FRAGMENTS, MAX_ROWS, OVERFLOW, SENTINEL, WAVE, World
from zipkin_amd import TraceAnnotationStore, TraceSpanStore, _abi
from zipkin_amd.spanstore import ENTRY_COLUMNS

pytestmark = pytest.mark.gpu

SKEW = ("TIME_SKEW",)
U64 = 2 ** 64 - 1
IP_A, IP_B, IP_C = 167772161, 167772162, 167772163


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


def check_raw(world, spans, annots, ids, overflowed=()):
    """The raw call against the helper, trace by trace; returns the answers."""
    got = X.answers(*annots.adjusted_traces(spans, ids))
    for i, g in zip(ids, got):
        w = world.expect(i)
        assert bool(g[0][7] & OVERFLOW) == (i in overflowed), f"trace {i}: state {g[0][7]}"
        assert g[0] == w[0], f"trace {i}: head"
        assert g[1] == w[1], f"trace {i}: spans"
        assert g[2] == w[2], f"trace {i}: services"
        assert g[3] == w[3], f"trace {i}: rows"
    return got


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
    got = check_raw(world, spans, annots, ids)
    assert got[5][0] == X.ZERO_HEAD and got[-1] == got[2]
    assert any(s[9] == 2 for g in got for s in g[1])  # the golden file has a client-only span


# ---- 2. seeded random traces, and the wave / workgroup switch --------------------------------------------------
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


def sr_chain(tid, n):
    """n spans in a chain, the root with a cs and every other span with one sr: n rows."""
    return {"trace_id": tid, "spans": [span(1, None, [[10, "cs", IP_A]])] + [span(k, k - 1, [[10 + k, "sr", IP_B]]) for k in range(2, n + 1)]}


def test_random_traces_and_the_work_lists_bound(stores):
    spans, annots = stores
    world = random_world(2024, 200, 64)
    world.add_case(padded(5000, 16, WAVE))
    world.add_case(padded(5001, 16, WAVE + 1))
    world.add_case(sr_chain(5002, WAVE))
    world.add_case(sr_chain(5003, WAVE + 1))
    sizes = [(len(s), len(a)) for s, a in world.traces.values()]
    assert all(f <= MAX_FRAGMENTS and r <= MAX_ROWS for f, r in sizes)
    assert any(f <= WAVE and r <= WAVE for f, r in sizes) and any(r > WAVE for f, r in sizes)
    assert sorted(len(world.traces[t][1]) for t in (5000, 5001)) == [WAVE, WAVE + 1]
    assert sorted(len(world.traces[t][0]) for t in (5002, 5003)) == [WAVE, WAVE + 1]
    world.feed(spans, annots, seed=7)
    assert spans.info()["segments"] == 3 and annots.info()["segments"] == 3
    ids = list(world.traces)
    np.random.default_rng(3).shuffle(ids)
    got = check_raw(world, spans, annots, ids)
    assert all(g[0][7] & FOUND for g in got)
    assert sum(s[9] for g in got for s in g[1]) > 20  # injections happen among the random traces


# ---- 3. injection ------------------------------------------------------------------------------------------------
def star(tid, n, hosted_lead):
    """A client-only root over n children; several children without cs / cr; the first child's lead with or
    without a host."""
    kids = []
    for k in range(n):
        anns = rpc(2000 + k, IP_B, IP_C, c_off=700, s_off=-90)
        if k == 0 and not hosted_lead:
            anns[0][2] = None
        if k % 7 == 3:
            anns = [a for a in anns if a[1] in ("sr", "ss")]
        if k % 11 == 5:
            anns = anns[:1]
        kids.append(span(10 + k, 1, anns))
    return {"trace_id": tid, "spans": [span(1, None, [[1900, "cs", IP_A], [4000, "cr", IP_A]])] + kids}


def client_chain(tid, n):
    """n spans in a chain, each with a cs and a cr only, on hosts whose clocks differ: every span but the last
    is client-only and gets its sr and ss."""
    ips, clock = [IP_A, IP_B, IP_C], {IP_A: 0, IP_B: 400, IP_C: -250}
    return {"trace_id": tid, "spans": [span(k + 1, k or None, [[1000 + 2 * k + clock[ips[k % 3]], "cs", ips[k % 3]],
                                                                [9000 - 2 * k + clock[ips[k % 3]], "cr", ips[k % 3]]])
                                       for k in range(n)]}


def test_injected_rows(stores):
    spans, annots = stores
    world = World()
    world.add_case(star(1, 500, hosted_lead=False))
    world.add_case(star(2, 500, hosted_lead=True))
    world.add_case(client_chain(3, 300))
    world.add_case(client_chain(4, 1024))
    # a client-only span that also has one sr; its child is shifted by the child's own skew
    world.add_case({"trace_id": 5, "spans": [span(1, None, [[100, "cs", IP_A], [104, "sr", IP_B], [200, "cr", IP_A]]),
                                             span(2, 1, rpc(500, IP_B, IP_C, c_off=390, s_off=10))]})
    assert len(world.traces[4][1]) == MAX_ROWS and len(world.traces[4][0]) == 1024
    world.feed(spans, annots, seed=5)
    got = dict(zip([1, 2, 3, 4, 5], check_raw(world, spans, annots, [1, 2, 3, 4, 5])))
    injected = {i: sum(s[9] for s in g[1]) // 2 for i, g in got.items()}
    assert injected == {1: 1, 2: 1, 3: 299, 4: 1023, 5: 1}
    assert got[4][0][8] == MAX_ROWS + 2 * 1024 - 2  # the largest emitted trace: A + 2 S - 2 rows
    lead = {i: [r for r in got[i][3] if r[1] == 1 and r[3] in (T.H_SR, T.H_SS)] for i in (1, 2)}
    assert [r[4:] for r in lead[1]] == [(0, 0, A.SR), (0, 0, A.SS)]
    assert [r[4:] for r in lead[2]] == [(IP_B, IP_B & 0xFF, A.SR | A.HAS_HOST | (80 << A.PORT_SHIFT)),
                                       (IP_B, IP_B & 0xFF, A.SS | A.HAS_HOST | (80 << A.PORT_SHIFT))]
    assert [r[3] for r in got[5][3] if r[1] == 1] == [T.fnv_mix(b"cs"), T.fnv_mix(b"sr"), T.fnv_mix(b"cr"), T.H_SR, T.H_SS]


# ---- 4. the bounds -----------------------------------------------------------------------------------------------
def test_the_full_lds_shape_and_one_above_each_bound(stores):
    """2048 merged spans beside exactly 2048 rows: the kernel's largest launch, emitted; one row more, and one
    fragment more, overflow and emit nothing."""
    spans, annots = stores
    world = World()
    s, a = T.golden_rows(padded(31, MAX_FRAGMENTS, 4 * MAX_FRAGMENTS))
    a = [r for r in a if r[1] % 4 == 1]  # rows for every fourth span, up and down the tree
    world.add(31, s, a)
    assert (len(s), len({r[1] for r in s}), len(a)) == (MAX_FRAGMENTS, MAX_FRAGMENTS, MAX_ROWS)
    world.add_case(padded(32, 400, MAX_ROWS + 1))
    s3, a3 = T.golden_rows(padded(33, 1024, 4 * 1024))
    a3 = [r for r in a3 if r[1] <= 256]
    s3 = s3 + [r[:3] + (r[3] - 1, r[4] + 1) + r[5:] for r in s3]  # every span in two fragments
    world.add(33, s3 + s3[:1], a3)
    world.add(34, [(34,) + r[1:] for r in s3 + s3[:1]], [])  # above the fragment bound, and not annotated
    assert len(world.traces[32][1]) == MAX_ROWS + 1 and len(world.traces[33][0]) == MAX_FRAGMENTS + 1
    world.feed(spans, annots, seed=8)
    got = check_raw(world, spans, annots, [32, 31, 33, 34], overflowed={32, 33, 34})
    assert got[1][0][4:] == (MAX_FRAGMENTS, MAX_FRAGMENTS, MAX_FRAGMENTS, FOUND | X.TIMED | ANNOTATED, MAX_ROWS, 0)
    for g, frags, rows in ((got[0], 400, True), (got[2], MAX_FRAGMENTS + 1, True), (got[3], MAX_FRAGMENTS + 1, False)):
        assert g[0][4:7] == (frags, 0, 0) and g[0][8] == 0 and g[1:] == ([], [], [])
        assert bool(g[0][7] & ANNOTATED) == rows and bool(g[0][7] & X.TR_OVERFLOW) == (not rows)


# ---- 5. no root, and the other shapes of the walk ---------------------------------------------------------------
def shapes():
    world = World()
    # no root at all. Span 2's record is the earliest, but span 3's rows are: the first span in annotation
    # order (3) is not the first in record order (2); the walk up from 3 ends at 9, whose parent is no span.
    s1, a1 = T.golden_rows({"trace_id": 1, "spans": [span(2, 9, rpc(50, IP_A, IP_B)), span(3, 4, rpc(300, IP_B, IP_C)),
                                                     span(4, 9, rpc(200, IP_A, IP_C, s_off=40)), span(9, 77, rpc(100, IP_C, IP_A)),
                                                     span(5, 3, [])]})
    a1 = [r[:2] + (r[2] - 290,) + r[3:] if r[1] == 3 else r for r in a1]  # span 3's rows are the earliest, its record is not
    world.add(1, s1, a1)
    # no root: an untimed record whose rows are the earliest
    s2, a2 = T.golden_rows({"trace_id": 2, "spans": [span(1, 2, rpc(100, IP_A, IP_B, s_off=50)), span(2, 3, rpc(90, IP_B, IP_C)),
                                                     span(3, 2, rpc(10, IP_A, IP_C))]})
    s2 = [r[:3] + (0, 0, r[5], r[6] & ~S.TIMED) if r[1] == 3 else r for r in s2]
    world.add(2, s2, a2)
    # no root: a cycle of three with a tail, a self-parent with a child, a parent that is no span
    world.add_case({"trace_id": 3, "spans": [span(1, 2, rpc(100, IP_A, IP_B, s_off=50)), span(2, 3, rpc(90, IP_B, IP_C, s_off=-50)),
                                             span(3, 1, rpc(95, IP_A, IP_C)), span(4, 1, rpc(80, IP_A, IP_C, s_off=500)),
                                             span(5, 4, rpc(70, IP_A, IP_C))]})
    world.add_case({"trace_id": 4, "spans": [span(8, 8, rpc(5, IP_A, IP_B, s_off=9)), span(9, 8, rpc(6, IP_A, IP_B)),
                                             span(7, 9, [[1, "cs", IP_A], [90, "cr", IP_A]])]})
    world.add_case({"trace_id": 14, "spans": [span(1, 77, rpc(100, IP_A, IP_B, s_off=50)), span(2, 1, rpc(110, IP_B, IP_C)),
                                              span(3, 78, rpc(1, IP_B, IP_C))]})
    # other roots and what hangs under them (pruned); a cycle and a self-parent beside the root's tree
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
    # traces without rows in the annotation store, next to the annotated ones: with a root, and without
    s8, _ = T.golden_rows({"trace_id": 8, "spans": [span(1, None, rpc(100, IP_A, IP_B)), span(2, 1, rpc(110, IP_B, IP_C)), span(3, 7, rpc(90, IP_B, IP_C))]})
    world.add(8, s8, [])
    s9, _ = T.golden_rows({"trace_id": 9, "spans": [span(1, 2, rpc(100, IP_A, IP_B)), span(2, 1, rpc(110, IP_B, IP_C)), span(3, 2, rpc(90, IP_B, IP_C))]})
    world.add(9, s9, [])
    return world


def test_shapes_of_the_walk(stores, gpu):
    import torch

    spans, annots = stores
    world = shapes()
    # (on the CPU) the no-root cases are what they claim
    m1 = T.annotated(*world.traces[1])
    assert m1[0]["id"] == 3 and S.trace(world.traces[1][0])[0]["id"] == 2 and T.root_most(m1)["id"] == 9
    m2 = T.annotated(*world.traces[2])
    assert m2[0]["id"] == 3 and S.trace(world.traces[2][0])[-1]["id"] == 3
    assert all(s["parent"] is not None for t in (1, 2, 3, 4, 14) for s in T.annotated(*world.traces[t]))
    world.feed(spans, annots, seed=5)
    ids = [U64, 0, 404, 9, 8, 7, 6, 5, 14, 4, 3, 2, 1, 6, 405, U64]  # absent and duplicated ids among them
    got = check_raw(world, spans, annots, ids)
    by = dict(zip(ids, got))
    assert [by[t][0][5] for t in (1, 2, 3, 4, 14, 5, 7)] == [5, 3, 5, 3, 3, 2, 3]
    assert by[1][0][3] == 9 and [(s[0], s[5]) for s in by[1][1]] == [(3, 3), (2, 2), (9, 1), (4, 2), (5, 4)]
    assert by[8][0][7] == FOUND | X.TIMED and by[8][0][8] == 0 and by[9][0][8] == 0
    # a trace without rows is zk_sp_traces' answer span for span
    th, ts, tv = spans.traces([8, 9])
    g = X.answers(*annots.adjusted_traces(spans, [8, 9]))
    assert [x[0][:8] for x in g] == [tuple(h) for h in th.tolist()]
    assert [s[:8] for x in g for s in x[1]] == [tuple(s) for s in ts.tolist()] and [v for x in g for v in x[2]] == tv.tolist()
    # device-pointer ids
    dev = torch.from_numpy(np.array(ids, np.uint64).view(np.int64)).to(f"cuda:{gpu}")
    assert X.answers(*annots.adjusted_traces(spans, dev)) == got


# ---- 6. sizing ---------------------------------------------------------------------------------------------------
def test_the_sizing_contract_and_empty_stores(stores, gpu):
    spans, annots = stores
    # both stores empty: an answer of zeros, no pass
    st, totals, heads, *_ = X.raw(annots, spans, [1, 2], (0, 0, 0))
    assert st == _abi.ZK_OK and totals == (0, 0, 0) and not heads.view(np.uint8).any()
    world = random_world(77, 12, 24)
    world.feed(spans, annots, seed=9, parts=1)
    ids = list(world.traces) + [404]
    # an empty annotation store: zk_sp_traces' own answer, rows = 0 in every head
    with TraceAnnotationStore(device=gpu) as empty:
        g = X.answers(*empty.adjusted_traces(spans, ids))
        th, ts, tv = spans.traces(ids)
        assert [x[0] for x in g] == [tuple(h) + (0, 0) for h in th.tolist()]
        assert [s for x in g for s in x[1]] == [tuple(s) + (0, 0) for s in ts.tolist()] and [v for x in g for v in x[2]] == tv.tolist()
    got = check_raw(world, spans, annots, ids)
    need = tuple(sum(len(g[k]) for g in got) for k in (1, 2, 3))
    assert min(need) > 4
    for short in range(3):  # each capacity short on its own: the totals and the heads, nothing else
        caps = tuple(c - 1 if k == short else c + 2 for k, c in enumerate(need))
        st, totals, heads, o_spans, o_svc, o_rows = X.raw(annots, spans, ids, caps)
        assert st == _abi.ZK_ERR_CAPACITY and totals == need, short
        assert [tuple(h) for h in heads.tolist()] == [g[0] for g in got]
        assert (o_spans.view(np.uint8) == SENTINEL).all() and (o_svc.view(np.uint8) == SENTINEL).all()
        assert all((getattr(o_rows, k).view(np.uint8) == SENTINEL).all() for k in A.COLS)
    caps = tuple(c + 3 for c in need)
    st, totals, heads, o_spans, o_svc, o_rows = X.raw(annots, spans, ids, caps)
    assert st == _abi.ZK_OK and totals == need
    assert X.answers(heads, o_spans[:need[0]], o_svc[:need[1]], o_rows.take(slice(0, need[2]))) == got
    assert (o_spans[need[0]:].view(np.uint8) == SENTINEL).all() and (o_svc[need[1]:].view(np.uint8) == SENTINEL).all()
    assert all((getattr(o_rows, k)[need[2]:].view(np.uint8) == SENTINEL).all() for k in A.COLS)
    many = np.zeros(_abi.ZK_AN_MAX_IDS + 1, np.uint64)
    assert X.raw(annots, spans, many, (0, 0, 0))[0] == _abi.ZK_ERR_INVALID_ARG


# ---- 7. the Python entry points against their host paths --------------------------------------------------------
class Texts:
    """A decoder for timeline text: .string(hash) of the free annotations the cases use."""

    def __init__(self, *texts):
        self.by = {T.fnv_mix(t.encode()): t for t in texts}

    def string(self, h):
        return self.by[h]


def trace_view(t):
    return ([tuple(s) for s in t.spans], [[tuple(a) for a in s.annotations] for s in t.spans],
            {k: [tuple(a) for a in v] for k, v in t.annotations.items()}, tuple(t.getRootMostSpan()), t.toSpanDepths())


def combo_view(c):
    s, ln = c.summary, c.timeline
    return (trace_view(c.trace), s if s is None else (s[:4], [tuple(x) for x in s.span_timestamps], s.endpoints),
            (ln.trace_id, ln.root_span_id, [tuple(a) for a in ln.annotations], ln.binary_annotations), c.span_depths)


def test_the_entry_points_equal_their_host_paths(gpu):
    names = [f"Svc{i}" for i in range(256)]
    span_names = ["get", "put", "scan"]
    with TraceSpanStore(device=gpu, services=names, span_names=span_names) as spans, TraceAnnotationStore(device=gpu) as annots:
        world = random_world(11, 40, 32)
        for c in T.golden()["cases"]:
            world.add_case(c)
        world.add_case(padded(9000, 8, MAX_ROWS + 1))  # above the row bound: the host's way
        world.add(9001, T.golden_rows({"trace_id": 9001, "spans": [span(1, None, rpc(5, IP_A, IP_B)), span(2, 1, rpc(6, IP_B, IP_C))]})[0], [])
        # span names: id (span id % 4), 0 for none
        world.traces = {t: ([r[:6] + (r[6] | ((r[1] % 4) << S.NAME_SHIFT),) for r in s], a) for t, (s, a) in world.traces.items()}
        world.feed(spans, annots, seed=3)
        ids = list(world.traces)[::-1] + [404]
        ids += ids[:3]
        heads = annots.adjusted_traces(spans, ids)[0]
        assert {int(h[0]) for h in heads.tolist() if h[7] & OVERFLOW} == {9000}
        decoder = Texts("foo", "bar", *[a[1] for c in T.golden()["cases"] for sp in c["spans"] for a in sp["annotations"]])
        host = spans.getTraceCombosByIds(ids, adjust=SKEW, annotations=annots)
        dev = spans.getTraceCombosByIds(ids, adjust=SKEW, annotations=annots, adjust_on_device=True)
        assert len(dev) == len(host) == len(ids) - 1
        for h, d in zip(host, dev):
            assert combo_view(d) == combo_view(h), f"trace {h.trace.id}"
            assert d.trace.rows is None or d.trace.id == 9000  # the one difference: rows, as with Trace.of_merged
        t_host = spans.getTracesByIds(ids, adjust=SKEW, annotations=annots)
        t_dev = spans.getTracesByIds(ids, adjust=("NOTHING", "TIME_SKEW"), annotations=annots, adjust_on_device=True)
        assert [trace_view(t) for t in t_dev] == [trace_view(t) for t in t_host]
        assert all(type(s).__name__ == "AnnotatedSpan" for t in t_dev for s in t.spans)
        l_host = spans.getTraceTimelinesByIds(ids, adjust=SKEW, annotations=annots, decoder=decoder)
        l_dev = spans.getTraceTimelinesByIds(ids, adjust=SKEW, annotations=annots, decoder=decoder, adjust_on_device=True)
        assert l_dev == l_host and any(a.value == "foo" for ln in l_dev for a in ln.annotations)
        assert any(a.service == "Unknown" for ln in l_dev for a in ln.annotations)
        # more than ZK_AN_MAX_IDS ids go in chunks
        rep = (ids * (_abi.ZK_AN_MAX_IDS // len(ids) + 2))[:_abi.ZK_AN_MAX_IDS + 5]
        some = [i for i in rep if i not in (9000, 404)]
        many = spans.getTraceTimelinesByIds(rep, adjust=SKEW, annotations=annots, adjust_on_device=True)
        by = {ln.trace_id: ln for ln in spans.getTraceTimelinesByIds(sorted(set(some)), adjust=SKEW, annotations=annots)}
        assert [ln for ln in many if ln.trace_id != 9000] == [by[i] for i in some]


# ---- 8. the stagings are shared, not corrupted ---------------------------------------------------------------
def test_the_other_calls_answer_as_before(stores):
    spans, annots = stores
    world = random_world(31, 40, 48)
    world.feed(spans, annots, seed=6)
    ids = list(world.traces)[::-1] + [404]

    def others():
        th, ts, tv = spans.traces(ids)
        sh, sc = spans.summaries(ids)
        ah, ac = annots.adjusted_summaries(spans, ids)
        counts, rows = annots.gather(ids)
        return (th.tolist(), ts.tolist(), tv.tolist(), sh.tolist(), [sc[k].tolist() for k, _ in ENTRY_COLUMNS], ah.tolist(),
                [ac[k].tolist() for k, _ in ENTRY_COLUMNS], counts.tolist(), rows.rows())

    before = others()
    first = check_raw(world, spans, annots, ids)
    assert others() == before
    assert X.answers(*annots.adjusted_traces(spans, ids)) == first


def test_query_ms_covers_both_streams(gpu):
    with TraceSpanStore(device=gpu, timing=True) as spans, TraceAnnotationStore(device=gpu, timing=True) as annots:
        world = random_world(5, 4, 8)
        world.feed(spans, annots, seed=1, parts=1)
        annots.adjusted_traces(spans, list(world.traces))
        assert annots.query_ms() > 0 and spans.query_ms() > 0
