"""The case list of tests/carryref.py reaches what tests/test_gpu_carry_bounds.py needs it to reach:
every branch class of the held-trace plan is populated, the builder's record counts are exact, and
the whole-stream reference is the oracle where no trace is too long. No device."""
import ctypes as C
from collections import Counter

import numpy as np

from oracle import oracle
from tests import carryref
from tests.carryref import CLASSES, LS, TARGETS, cases, classify, expected, runs, target_len, trace_of
from zipkin_amd import _abi
from zipkin_amd.columns import SpanColumns


def test_trace_of_builds_exact_record_counts():
    S = 7
    for n in (1, 2, 3, 4, 5, 511, 512, 513, 514, 1029, 2005):
        t = trace_of(99, n, S)
        assert len(t) == n and (t.trace_id == 99).all()
        ref = oracle.aggregate(t, S)
        assert ref.stats["records"] == n
        # the root and one merged span per child; every child joins its parent
        assert ref.stats["merged_spans"] == 1 + n // 2
        assert ref.stats["joined_links"] == n // 2 and ref.stats["missing_parent"] == 0
        assert len(np.unique(t.span_id)) == 1 + n // 2


def test_a_lost_fragment_or_a_piece_joined_alone_changes_the_table():
    S = 7
    t = trace_of(5, 41, S)
    whole = carryref.expected_cells(oracle.aggregate(t, S))
    # without one client fragment the child's duration is its server fragment's
    assert carryref.expected_cells(oracle.aggregate(t.take(np.r_[0:10, 11:41]), S)) != whole
    # any six consecutive records hold a parent and a child of its
    for at in range(1, 35):
        assert oracle.aggregate(t.take(slice(at, at + 6)), S).stats["joined_links"] >= 1, at


def test_expected_is_the_oracle_where_no_trace_is_too_long():
    S = 41
    key, cols, a, b = carryref.stream(1000, S, "L")
    ref, want = expected(cols, S, 1000), oracle.aggregate(cols, S)
    assert ref.stats == want.stats and np.array_equal(ref.cells, want.cells)
    # one record more: the trace is removed whole, counted once, wherever the batches are cut
    key, cols, a, b = carryref.stream(1000, S, "L+1")
    ref = expected(cols, S, 1000)
    rest = SpanColumns.concat([cols.take(slice(0, a)), cols.take(slice(b, len(cols)))])
    want = oracle.aggregate(rest, S)
    assert ref.stats["trace_too_large"] == 1 and ref.stats["records"] == len(cols) - 1001
    assert np.array_equal(ref.cells, want.cells)
    cutref = expected(carryref.cut(cols, [a + 3, a + 700]), S, 1000)
    assert cutref.stats == ref.stats and np.array_equal(cutref.cells, ref.cells)


def test_classify_on_hand_made_streams():
    L, S = 512, 7
    A, B = trace_of(1, 30, S), trace_of(3, 40, S)

    def cls(stream, points, flags=None):
        parts = carryref.cut(stream, points)
        return classify(L, parts, flags or [True] * (len(parts) - 1) + [False])

    for n, name in ((L, "held_L"), (L + 1, "held_L_plus_1")):
        s = SpanColumns.concat([A, trace_of(2, n, S), B])
        got = cls(s, [30 + n])  # cut at the trace's end: its run is held whole, then flushed
        assert {"lead_round1", "tail_round2"} <= got[0] and name in got[1]
        got = cls(s, [30, 30 + n])  # ... as a batch of its own
        assert "one_run_short_fresh" in got[1] and name in got[2]
        got = cls(s, [30 + 100])  # cut inside: held 100, the leading run brings it to n
        assert ("append_to_L" if n == L else "append_to_L_plus_1") in got[1]
        assert "held_L" not in got[1] and "held_L" not in got[2]
    s = SpanColumns.concat([A, trace_of(2, 2 * L + 5, S), B])
    got = cls(s, [30 + 600])  # the last run has 600 records: only known to be long
    assert {"tail_unknown", "long_tail_continues"} <= got[0] and "lead_round1" in got[0]
    assert {"dropped_rest_leading", "dropped_then_other_trace", "lead_round2"} <= got[1]
    got = cls(s, [30, 30 + L + 2, 30 + L + 4])
    assert {"one_run_long_fresh", "long_tail_continues"} <= got[1]
    assert {"dropped_whole_batch", "one_run_short_held", "n2"} <= got[2]
    assert {"dropped_rest_leading", "lead_unknown"} <= got[3]
    got = cls(s, [30 + 10, 30 + 10 + L + 2])
    assert "one_run_long_held" in got[1] and "dropped_whole_batch" in got[1]
    assert "long_tail_continues" not in got[1]  # the plan itself dropped the held trace
    got = classify(L, [A.take(slice(0, 1)), SpanColumns.empty(0), SpanColumns.empty(0)], [True, True, False])
    assert got[0] == {"n1", "one_run_short_fresh"} and got[1] == {"empty_continues"} and got[2] == {"empty_plain"}
    # the search rounds: a boundary at 256 is the first round's last record, 257 the second's first
    s = SpanColumns.concat([trace_of(2, 256, S), B, trace_of(4, 257, S)])
    assert {"lead_round1", "tail_round2"} <= cls(s, [])[0]
    s = SpanColumns.concat([trace_of(2, 257, S), B, trace_of(4, 256, S)])
    assert {"lead_round2", "tail_round1"} <= cls(s, [])[0]


def test_case_list_reaches_every_class():
    seen = Counter()
    per_family = {}
    for c in cases():
        assert c.L in LS and 7 <= c.S <= 41 and len(c.parts) == len(c.flags)
        assert sum(len(p) for p in c.parts) == len(c.stream) < 5000
        lens = runs(c.stream.trace_id)[1]
        assert (lens > 128).sum() == 1  # the target alone is long
        for cls in classify(c.L, c.parts, c.flags):
            seen.update(cls)
            per_family.setdefault(c.key, set()).update(cls)
    print(len(cases()), "cases;", {k: seen[k] for k in CLASSES})
    for k in CLASSES:
        assert seen[k] >= 1, k
    assert set(seen) <= set(CLASSES)
    for L in LS:
        # every way of flushing is covered where it matters most: the targets of L and L + 1 records, held whole
        for target, name in (("L", "held_L"), ("L+1", "held_L_plus_1")):
            ends = {c.end for c in cases() if c.key == f"L{L}-{target}-last" and c.name.split(":")[1] == "a"}
            assert ends == {"finalize", "empty", "partial"}
            assert name in per_family[f"L{L}-{target}-last"] and name in per_family[f"L{L}-{target}"]
        assert "append_to_L" in per_family[f"L{L}-L"] and "append_to_L_plus_1" in per_family[f"L{L}-L+1"]
        assert "long_tail_continues" in per_family[f"L{L}-L+2"] and "long_tail_continues" in per_family[f"L{L}-2L+5"]
        for target in TARGETS:
            key, cols, a, b = carryref.stream(L, carryref.S_OF[L], target)
            assert b - a == target_len(L, target)


def test_ctx_create_refuses_a_bound_below_one_join_window():
    """0 < max_trace_records < 512 is refused before a device is touched (zkagg.h): the streaming join
    aggregates every trace that fits one of its windows, so a smaller bound would hold for a trace cut
    over two batches only. 0 (the default) and 512 pass the argument checks."""
    L = _abi.lib()
    h = C.c_void_p()
    for bound, refused in ((1, True), (511, True), (0, False), (512, False), (1 << 20, False), ((1 << 20) + 1, True)):
        cfg = _abi.zk_config()
        cfg.num_services = 7
        cfg.device = 1 << 20  # no such device: a config that passes the argument checks stops there
        cfg.max_trace_records = bound
        st = L.zk_ctx_create(C.byref(cfg), C.byref(h))
        assert st == (_abi.ZK_ERR_INVALID_ARG if refused else _abi.ZK_ERR_NO_DEVICE), bound
        assert not h.value
