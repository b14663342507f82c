"""Merged traces on the device (zk_sp_traces, TraceSpanStore.traces, getTraceCombosByIds with on_device=True)
against the model of the call's output (tests/sptraceref.py, built on tests/spref.py's model store and the
host Trace class) and against the default host path. Every comparison is exact equality; nothing depends on
the order in which the device appended a trace's rows."""
import ctypes as C

import numpy as np
import pytest

from tests import spref as R
from tests import sptraceref as M
from zipkin_amd import TRACE_HEAD, TRACE_SPAN, DeviceColumns, TraceSpanStore, ZkError, _abi

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
MAX_ROWS = _abi.ZK_SP_TRACE_MAX_ROWS  # the longest trace merged on the device
WAVE = _abi.ZK_SP_SUM_WAVE_ROWS       # up to here a wave takes the trace, above it a workgroup
CORNERS = (0, 1, 2 ** 63, U64)        # the unsigned order's corners
HP, T, SC, SS = R.HAS_PARENT, R.TIMED, R.SVC_CLIENT, R.SVC_SERVER
SENTINEL = 0xA5


@pytest.fixture()
def make(gpu):
    made = []

    def factory(**kw):
        made.append(TraceSpanStore(device=gpu, **kw))
        return made[-1]

    yield factory
    for s in made:
        s.close()


def observe_all(store, batches, device=True):
    for b in batches:
        b = R.cols_of(b) if isinstance(b, list) else b
        store.observe(DeviceColumns.from_host(b) if device else b)


def name(i):
    return i << R.NAME_SHIFT


def gen_trace(rng, tid, n, n_spans=None):
    """n rows of one trace over few span ids (the corners first); parents drawn from the same ids, so that
    they hit, and from two ids that are never spans; every combination of the four low flag bits; name ids
    0..3; times from a few values; every fifth row a copy of the one before it."""
    k = int(rng.integers(1, 9)) if n_spans is None else n_spans
    spans = [int(x) for x in rng.permutation(np.array(CORNERS, np.uint64))][:k]
    spans += [int(x) for x in rng.integers(2, 2 ** 63, max(0, k - len(spans)), dtype=np.uint64)]
    parents = spans + [7, 2 ** 63 + 7]
    rows = []
    for i in range(n):
        fl = ((i + int(rng.integers(0, 16))) % 16) | name(int(rng.integers(0, 4)))
        rows.append((tid, spans[int(rng.integers(len(spans)))], parents[int(rng.integers(len(parents)))],
                     int(rng.integers(-3, 5)), int(rng.integers(-3, 5)), int(rng.integers(3)), fl))
        if i % 5 == 4:
            rows[i] = rows[i - 1]
    return rows


def check(store, model, ids):
    """traces() against the model, and the device path of getTraceCombosByIds against the host path."""
    heads, spans, services = store.traces(ids)
    want_heads, want_spans, want_services = M.traces(model, ids, MAX_ROWS)
    assert heads.dtype == TRACE_HEAD and spans.dtype == TRACE_SPAN and services.dtype == np.uint32
    assert heads.tolist() == want_heads
    assert spans.tolist() == want_spans
    assert services.tolist() == want_services
    host = store.getTraceCombosByIds(ids)
    dev = store.getTraceCombosByIds(ids, on_device=True)
    assert [M.combo_view(c) for c in dev] == [M.combo_view(c) for c in host]
    return heads, spans, host


def raw(store, ids, cap_spans, cap_services, flags=0, ptr=None):
    """zk_sp_traces into sentinel-filled buffers: (status, n_out, heads, spans, services)."""
    ids = np.ascontiguousarray(np.asarray(ids, np.uint64))
    heads = np.frombuffer(bytes([SENTINEL]) * (max(len(ids), 1) * 48), TRACE_HEAD).copy()
    spans = np.frombuffer(bytes([SENTINEL]) * (max(cap_spans, 1) * 48), TRACE_SPAN).copy()
    services = np.frombuffer(bytes([SENTINEL]) * (max(cap_services, 1) * 4), np.uint32).copy()
    n_out = (C.c_uint64 * 2)(12345, 12345)
    st = store._L.zk_sp_traces(store._h, ids.ctypes.data if ptr is None else ptr, len(ids), flags, heads.ctypes.data,
                               spans.ctypes.data, cap_spans, services.ctypes.data, cap_services, n_out)
    return st, list(n_out), heads, spans, services


def untouched(a):
    return bool((a.view(np.uint8) == SENTINEL).all())


# ---- 1. the reference's vectors --------------------------------------------------------------------------
def test_golden_vectors(make):
    g = M.golden()
    store = make(services=g["services"], span_names=g["span_names"])
    for case in g["cases"]:
        store.reset()
        rows, want, tid = R.golden_rows(case, g["services"]), case["expect"], case["trace_id"]
        observe_all(store, [rows])
        check(store, rows, [tid])
        got = store.getTraceCombosByIds([tid], on_device=True)
        if not rows:
            assert got == []
            continue
        (c,) = got
        assert [s.id for s in c.trace.spans] == want["span_order"] and c.trace.rows is None and c.timeline is None
        assert c.trace.getRootMostSpan().id == want["root_most"]
        assert sorted(c.span_depths.items()) == sorted(map(tuple, want["depths"])) and c.trace.toSpanDepths() == c.span_depths
        assert [s.id for s in c.trace.getRootSpans()] == want["root_spans"]
        s = want["summary"]
        assert c.summary == (None if s is None else (s[0], s[1], s[2], s[3], [tuple(x) for x in s[4]], []))


# ---- 2. row counts -------------------------------------------------------------------------------------------
SMALL = (1, 2, 63, 64, 65, 256, 257)


def test_row_counts(make):
    assert {WAVE - 1, WAVE, WAVE + 1} <= set(SMALL)
    rng = np.random.default_rng(2)
    store = make()
    model, ids = [], []
    for k, n in enumerate(SMALL):
        ids.append(R.id_in_bucket(k % 3, 100 + k))  # (several traces share a bucket)
        model += gen_trace(rng, ids[-1], n, n_spans=max(1, min(n // 3, 60)))
    observe_all(store, [[model[i] for i in rng.permutation(len(model))]])
    heads, _, _ = check(store, model, ids)
    assert heads["fragments"].tolist() == list(SMALL) and not (heads["state"] & M.OVERFLOW).any()
    for i in ids:  # one trace per call: the workgroups' LDS is then sized by that trace alone
        h, s, v = store.traces([i])
        assert (h.tolist(), s.tolist(), v.tolist()) == M.traces(model, [i], MAX_ROWS)


@pytest.mark.parametrize("n", (MAX_ROWS, MAX_ROWS + 1))
def test_row_counts_at_the_bound(make, n):
    rng = np.random.default_rng(n)
    tid, small = R.id_in_bucket(5, 1), R.id_in_bucket(5, 2)
    model = gen_trace(rng, tid, n, n_spans=700) + gen_trace(rng, small, 3)
    store = make()
    observe_all(store, [[model[i] for i in rng.permutation(len(model))]])
    heads, spans, host = check(store, model, [small, tid, small])
    over = n > MAX_ROWS
    assert heads["fragments"].tolist() == [3, n, 3]
    assert [bool(s & M.OVERFLOW) for s in heads["state"].tolist()] == [False, over, False]
    if over:  # exact reductions, nothing emitted, the neighbours as they are alone, completed by the host path
        se = R.start_end([r for r in model if r[0] == tid])
        assert heads[1].tolist() == (tid, se[0], se[1], 0, n, 0, 0, M.FOUND | M.TIMED | M.OVERFLOW)
        assert len(spans) == 2 * heads[0]["spans"] and store.traces([small])[1].tolist() * 2 == spans.tolist()
    assert [c.trace.id for c in host] == [small, tid, small]
    assert len(store.getTraceCombosByIds([tid], on_device=True)[0].trace.spans) > 600


# ---- 3. tree shapes ------------------------------------------------------------------------------------------
def tree(tid, spec):
    """Rows from (span id, parent or None, first or None): one fragment per span, a service each."""
    return [(tid, s, p or 0, f or 0, min((f or 0) + 1, R.INT64_MAX), s % 3, (HP if p is not None else 0) | (T if f is not None else 0) | SC | name(1 + s % 5))
            for s, p, f in spec]


def shapes():
    rng = np.random.default_rng(3)
    times = [int(x) for x in rng.permutation(64)]  # (span order is not the chain's order)
    far = R.INT64_MAX
    return {
        "chain": ([(i + 1, i if i else None, times[i]) for i in range(64)], 1, 64),
        "star": ([(1, None, 50)] + [(i, 1, int(times[i])) for i in range(2, 42)], 1, 2),
        "two_parentless_by_first": ([(9, None, 50), (3, None, 20), (4, 9, 1), (5, 3, 60)], 3, 2),
        "two_parentless_tie_untimed_first": ([(4, None, None), (8, None, far), (5, 8, 1), (6, 4, 2)], 4, 2),
        "two_parentless_tie_timed_first": ([(8, None, None), (4, None, far), (5, 8, 1), (6, 4, 2)], 4, 2),
        "missing_parent_above": ([(10, 999, 30), (20, 10, 5), (30, 20, 40), (40, 10, 6)], 10, 3),
        "cycle_holds_the_first_span": ([(1, 2, 30), (2, 3, 10), (3, 1, 20), (4, 2, 40)], 2, 3),
        "cycle_below_a_tail": ([(9, 1, 5), (1, 2, 30), (2, 3, 10), (3, 1, 20), (4, 3, 50)], 1, 3),
        "self_parent": ([(5, 5, 10), (6, 5, 20), (7, 6, 30)], 5, 3),
        "subtree_off_a_missing_parent": ([(1, None, 10), (2, 1, 20), (3, 555, 5), (4, 3, 6), (5, 4, 7)], 1, 2),
        "corner_ids": ([(U64, None, 9), (0, U64, 3), (2 ** 63, 0, 2), (1, 2 ** 63, 1)], U64, 4),
        "parent_all_ones_beside_no_parent": ([(1, U64, 3), (2, None, 5), (U64, 2, 1), (0, 0, 0)], 2, 3),
    }


@pytest.mark.parametrize("path", ("wave", "workgroup"))
def test_tree_shapes(make, path):
    store = make()
    model, ids, want = [], [], []
    for k, (label, (spec, root, deepest)) in enumerate(shapes().items()):
        tid = R.id_in_bucket(k % 2, 10 + k)
        rows = tree(tid, spec)
        if path == "workgroup":  # more fragments of the same spans, without a parent bit or times of their own
            rows += [(tid, spec[i % len(spec)][0], 77, -9, 99, 1, SS) for i in range(WAVE + 1)]
        model += rows
        ids.append(tid)
        want.append((label, root, deepest))
    observe_all(store, [model])
    heads, spans, host = check(store, model, ids)
    assert (heads["fragments"] > WAVE).all() == (path == "workgroup")
    at = 0
    for (label, root, deepest), h in zip(want, heads.tolist()):
        mine = spans[at:at + h[5]]
        at += h[5]
        assert h[3] == root and int(mine["depth"].max()) == deepest, label
        assert mine["span_id"][(mine["bits"] & M.ROOT_MOST) != 0].tolist() == [root] and mine["depth"][mine["span_id"] == root].tolist() == [1], label
    by = dict(zip([w[0] for w in want], host))
    assert by["chain"].span_depths == {i + 1: i + 1 for i in range(64)}
    assert by["subtree_off_a_missing_parent"].span_depths == {1: 1, 2: 2}
    assert by["cycle_holds_the_first_span"].span_depths == {2: 1, 1: 2, 4: 2, 3: 3}
    assert by["cycle_below_a_tail"].span_depths == {1: 1, 3: 2, 9: 2, 2: 3, 4: 3}
    assert by["self_parent"].span_depths == {5: 1, 6: 2, 7: 3}
    assert by["parent_all_ones_beside_no_parent"].span_depths == {2: 1, U64: 2, 1: 3}
    off = spans[np.isin(spans["span_id"], (3, 4, 5)) & (spans["depth"] == 0)]
    assert len(off) >= 3 and not (off["bits"][off["span_id"] == 3] & M.PARENT_FOUND).any()


def test_a_chain_of_the_most_spans(make):
    """2048 single-fragment spans in one chain: the depth equals the span count."""
    rng = np.random.default_rng(4)
    order = [int(x) for x in rng.permutation(MAX_ROWS)]  # the chain's i-th span has id order[i] + 1
    tid = R.id_in_bucket(9, 9)
    model = [(tid, order[i] + 1, order[i - 1] + 1 if i else 0, int(rng.integers(0, 50)), 60, i % 3, (HP if i else 0) | T | SC)
             for i in range(MAX_ROWS)]
    store = make()
    observe_all(store, [[model[i] for i in rng.permutation(MAX_ROWS)]])
    heads, spans, host = check(store, model, [tid])
    assert heads[0]["spans"] == MAX_ROWS and heads[0]["root_most"] == order[0] + 1
    assert sorted(spans["depth"].tolist()) == list(range(1, MAX_ROWS + 1))
    assert host[0].span_depths[order[-1] + 1] == MAX_ROWS


# ---- 4. the rules ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ("wave", "workgroup"))
def test_parent_name_and_service_rules(make, path):
    a, b, c, d, e = (R.id_in_bucket(3, k) for k in range(5))
    model = [
        # the parent: the least parent id among the fragments with the bit; all ones and 0 are parents
        (a, 5, U64, 0, 0, 0, HP), (a, 5, 3, 0, 0, 0, 0), (a, 6, 0, 0, 0, 0, HP), (a, 6, 1, 0, 0, 0, HP), (a, 7, 9, 0, 0, 0, 0),
        (a, U64, 0, 0, 0, 0, 0),
        # the name: fragments that differ first in parent_id ...
        (b, 5, 2, 0, 0, 0, name(7)), (b, 5, 1, 9, 9, 9, name(8)),
        # ... then only in an UNTIMED fragment's raw first_ts ...
        (c, 5, 1, 4, 0, 0, name(7)), (c, 5, 1, 3, 0, 0, name(8)), (c, 5, 1, 2, 0, 0, 0),
        # ... then only in flags
        (d, 5, 1, 3, 0, 0, name(8)), (d, 5, 1, 3, 0, 0, name(7) | T), (d, 5, 1, 3, 0, 0, T),
        # duplicate fragments; a fragment with neither service bit gives no service and is a fragment of the span
        (e, 1, 0, 1, 2, 4, T | SC), (e, 1, 0, 1, 2, 4, T | SC), (e, 1, 0, 1, 2, 4, T | SS), (e, 1, 0, 0, 9, 2, T), (e, 1, 0, 5, 6, 3, SS),
        (e, 2, 1, 0, 0, 8, HP), (e, 2, 1, 0, 0, 8, HP),
    ]
    if path == "workgroup":
        model += [(t, 5 if t != e else 1, U64, R.INT64_MAX, R.INT64_MAX, 4 if t == e else 0, SC * (t == e)) for t in (a, b, c, d, e)
                  for _ in range(WAVE + 1)]
    store = make()
    observe_all(store, [model])
    heads, spans, host = check(store, model, [a, b, c, d, e])
    assert [(s.id, s.parent) for s in host[0].trace.spans] == [(5, U64), (6, 0), (7, None), (U64, None)]
    assert [x.trace.spans[0].name for x in host[1:4]] == [8, 8, 7]
    assert [(s.id, s.first, s.last, s.services) for s in host[4].trace.spans] == [(1, 0, 9, (3, 4)), (2, None, None, ())]
    assert host[4].trace.serviceCounts() == {3: 1, 4: 1} and host[4].span_depths == {1: 1, 2: 2}


# ---- 5. the ask ------------------------------------------------------------------------------------------------
def test_the_ask(make, gpu):
    import torch

    rng = np.random.default_rng(6)
    model = []
    for tid in (0, U64, 5, 6):
        model += gen_trace(rng, tid, 20)
    store = make()
    assert store.getTraceCombosByIds([0, 5], on_device=True) == []  # the empty store: no device pass
    st, n_out, heads, spans, services = raw(store, [0, 5, U64], 4, 4)
    assert (st, n_out) == (_abi.ZK_OK, [0, 0]) and not heads.view(np.uint8).any() and untouched(spans) and untouched(services)
    observe_all(store, [model])
    ids = [5, 404, 0, 5, U64, 405, 5, 6]
    heads, _, host = check(store, model, ids)
    assert heads.tolist()[1] == heads.tolist()[5] == M.ZERO and heads.tolist()[0] == heads.tolist()[3] == heads.tolist()[6]
    assert [c.trace.id for c in host] == [5, 0, 5, U64, 5, 6]
    # n == 0
    h0, s0, v0 = store.traces([])
    assert len(h0) == len(s0) == len(v0) == 0
    st, n_out, heads, spans, services = raw(store, [], 4, 4)
    assert (st, n_out) == (_abi.ZK_OK, [0, 0]) and untouched(heads) and untouched(spans) and untouched(services)
    assert store.getTraceCombosByIds([], on_device=True) == []
    # device-pointer ids
    dev = torch.from_numpy(np.array(ids, np.uint64).view(np.int64)).to(f"cuda:{gpu}")
    hd, sd, vd = store.traces(dev)
    assert (hd.tolist(), sd.tolist(), vd.tolist()) == M.traces(model, ids, MAX_ROWS)
    # NULL arguments, a cap without its buffer, an unknown flag and one id too many, with a live handle
    a, t = np.array(ids, np.uint64), (C.c_uint64 * 2)()
    L, h, H = store._L, store._h, hd.ctypes.data
    assert L.zk_sp_traces(h, None, 8, 0, H, None, 0, None, 0, t) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_sp_traces(h, a.ctypes.data, 8, 0, None, None, 0, None, 0, t) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_sp_traces(h, a.ctypes.data, 8, 0, H, None, 0, None, 0, None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_sp_traces(h, a.ctypes.data, 8, 0, H, None, 3, None, 0, t) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_sp_traces(h, a.ctypes.data, 8, 0, H, None, 0, None, 3, t) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_sp_traces(h, a.ctypes.data, 8, 2, H, None, 0, None, 0, t) == _abi.ZK_ERR_INVALID_ARG
    with pytest.raises(ZkError) as e:
        store.traces(list(range(_abi.ZK_SP_MAX_IDS + 1)))
    assert e.value.status == _abi.ZK_ERR_INVALID_ARG and "ZK_SP_MAX_IDS" in e.value.message


def test_an_ask_of_the_most_ids_and_one_more(make):
    n = _abi.ZK_SP_MAX_IDS + 1
    rng = np.random.default_rng(7)
    tids = np.unique(rng.integers(0, 2 ** 64, n + 50, dtype=np.uint64))[:n].tolist()
    model = [(t, k % 3, k % 2, k, k + 1, k % 5, (k % 16) | name(1)) for k, t in enumerate(tids)]
    store = make()
    observe_all(store, [model])
    heads, spans, services = store.traces(tids[:n - 1])  # exactly ZK_SP_MAX_IDS one-row traces in one call
    assert len(heads) == _abi.ZK_SP_MAX_IDS == 4096
    assert (heads.tolist(), spans.tolist(), services.tolist()) == M.traces(model, tids[:n - 1], MAX_ROWS)
    got = store.getTraceCombosByIds(tids, on_device=True)  # 4097: the Python call asks in parts
    assert [M.combo_view(c) for c in got] == [M.combo_view(c) for c in store.getTraceCombosByIds(tids)]
    assert [c.trace.id for c in got] == tids


# ---- 6. capacity -----------------------------------------------------------------------------------------------
def test_capacity(make):
    rng = np.random.default_rng(8)
    model = gen_trace(rng, 5, 30, n_spans=5) + gen_trace(rng, 6, 80, n_spans=5) + [(9, 1, 0, 1, 2, 3, T | SC)]
    store = make()
    observe_all(store, [model])
    ids = [6, 404, 5, 6, 9]
    want_heads, want_spans, want_services = M.traces(model, ids, MAX_ROWS)
    ns, nv = len(want_spans), len(want_services)
    assert ns > 10 and nv > 10
    for cs, cv in ((0, 0), (ns - 1, nv), (ns, nv - 1), (ns - 1, nv - 1)):  # the sizing call; each cap one short in turn
        st, n_out, heads, spans, services = raw(store, ids, cs, cv)
        assert (st, n_out) == (_abi.ZK_ERR_CAPACITY, [ns, nv]) and heads.tolist() == want_heads
        assert untouched(spans) and untouched(services)
    st, n_out, heads, spans, services = raw(store, ids, ns, nv)
    assert (st, n_out) == (_abi.ZK_OK, [ns, nv]) and heads.tolist() == want_heads
    assert spans.tolist() == want_spans and services.tolist() == want_services
    st, n_out, heads, spans, services = raw(store, ids, ns + 2, nv + 3)  # what lies past the totals stays as it was
    assert st == _abi.ZK_OK and spans[:ns].tolist() == want_spans and services[:nv].tolist() == want_services
    assert untouched(spans[ns:]) and untouched(services[nv:])
    t = (C.c_uint64 * 2)()
    st = store._L.zk_sp_traces(store._h, np.array(ids, np.uint64).ctypes.data, 5, 0, heads.ctypes.data, None, 0, None, 0, t)
    assert (st, list(t)) == (_abi.ZK_ERR_CAPACITY, [ns, nv])  # both caps 0 with NULL buffers


# ---- 7. segments and expiry ------------------------------------------------------------------------------
def test_segments_compact_and_expire(make):
    rng = np.random.default_rng(5)
    spread, old, other = R.id_in_bucket(77, 0), R.id_in_bucket(77, 1), R.id_in_bucket(78, 0)
    parts = []
    for k in range(3):
        part = gen_trace(rng, spread, 30 + k, n_spans=6) + gen_trace(rng, other, 4)
        part += [(old, 1, 0, 0, 10, 1, T | SS)] * 2
        parts.append(part)
    parts[1].append((spread, 1, 0, 2000, 3000, 2, T | SC))
    parts[2].append((other, 1, 0, 2000, 3000, 2, T | SC))
    model = parts[0] + parts[1] + parts[2]
    ids = [spread, old, other]
    store = make()
    observe_all(store, parts)
    assert store.info()["segments"] == 3
    before, spans_before, _ = check(store, model, ids)
    assert before["fragments"].tolist() == [94, 6, 13]
    store.compact()
    assert store.info()["segments"] == 1
    after, spans_after, _ = check(store, model, ids)
    assert after.tolist() == before.tolist() and spans_after.tolist() == spans_before.tolist()
    observe_all(store, [parts[0]])  # two segments again, then the neighbour in the bucket goes
    model += parts[0]
    assert store.expire(2500) == 8
    model = [r for r in model if r[0] != old]
    heads, _, _ = check(store, model, ids)
    assert heads.tolist()[1] == M.ZERO and heads["fragments"].tolist() == [94 + 30, 0, 13 + 4]


# ---- 8. random traces ----------------------------------------------------------------------------------------
def test_random_traces(make):
    rng = np.random.default_rng(9)
    model, ids = [], []
    for k in range(300):
        ids.append(int(rng.integers(0, 2 ** 64, dtype=np.uint64)))
        model += gen_trace(rng, ids[-1], int(rng.integers(1, 40)) if k % 10 else int(rng.integers(WAVE, 200)))
    assert {r[6] & 15 for r in model} == set(range(16)) and len(set(model)) < len(model)
    store = make()
    batches = [[model[i] for i in part] for part in np.array_split(rng.permutation(len(model)), 3)]
    observe_all(store, batches)
    heads, spans, host = check(store, model, ids)
    roots = [c.trace.getRootSpan() is None for c in host]
    assert any(roots) and not all(roots) and any(len(c.span_depths) < len(c.trace.spans) for c in host)
    assert (spans["bits"] & M.PARENT_FOUND).any() and (spans["depth"] > 2).any()
    # the append order does not show: the same multiset observed in another order and cut
    again = make()
    observe_all(again, [[model[i] for i in part] for part in np.array_split(rng.permutation(len(model)), 5)], device=False)
    assert [x.tolist() for x in again.traces(ids)] == [x.tolist() for x in store.traces(ids)]


# ---- 9. dictionaries and timing --------------------------------------------------------------------------------
def test_dictionaries(make):
    rng = np.random.default_rng(10)
    model = gen_trace(rng, 5, 40) + gen_trace(rng, 6, 100)
    names, spans = ["Alpha", "BETA", "gamma"], ["get", "put", "scan"]
    store = make(services=names, span_names=spans)
    observe_all(store, [model])
    got = store.getTraceCombosByIds([6, 5], on_device=True)
    assert [M.combo_view(c) for c in got] == [M.combo_view(c) for c in store.getTraceCombosByIds([6, 5])]
    assert {v for c in got for s in c.trace.spans for v in s.services} == {"alpha", "beta", "gamma"}
    assert {s.name for c in got for s in c.trace.spans} <= {None, "get", "put", "scan"}
    short = make(services=names[:2], span_names=spans)
    observe_all(short, [model])
    for on_device in (False, True):
        with pytest.raises(ValueError):
            short.getTraceCombosByIds([5, 6], on_device=on_device)


def test_timing(make):
    rng = np.random.default_rng(11)
    store = make(timing=True)
    observe_all(store, [gen_trace(rng, 5, 40) + gen_trace(rng, 6, 100)])
    with pytest.raises(ZkError):
        store.query_ms()
    store.traces([5, 6, 7])
    assert store.query_ms() > 0
