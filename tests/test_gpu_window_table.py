"""The trace-time table and the table-mode partition (include/zkwindow.h: zk_win_observe,
ZK_WIN_TRACE_TABLE) against tests/winref_table.py. Every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

from tests import wincases, winref, winref_table
from tests.sketchref import mix64, unmix64
from tests.wincases import HOUR, INT64_MAX, INT64_MIN, T0
from zipkin_amd import DeviceColumns, SpanColumns, WindowPartition, ZkError, _abi

pytestmark = pytest.mark.gpu

SALT = _abi.ZK_WIN_TABLE_SALT
ABSENT = np.array([3, 0xDEADBEEF, 2 ** 63, 2 ** 64 - 2], np.uint64)


@pytest.fixture()
def h(gpu):
    with WindowPartition(window_us=HOUR, origin_us=T0, num_windows=8, device=gpu) as w:
        yield w


def check_table(h, batches, extra_ids=()):
    """trace_times over every id that occurs (and some that do not) equals table_of(batches)."""
    table = winref_table.table_of(batches)
    ids = np.unique(np.concatenate([b.trace_id for b in batches] + [ABSENT, np.array(extra_ids, np.uint64)]))
    t, found = h.trace_times(ids)
    for i, tid in enumerate(ids.tolist()):
        assert bool(found[i]) == (tid in table), tid
        if tid in table:
            assert int(t[i]) == table[tid], tid
    assert h.table_info()["traces"] == len(table)
    return table, ids, t, found


def observe_all(h, batches, device=True):
    for b in batches:
        h.observe(DeviceColumns.from_host(b) if device else b)


# ---- the table's content -----------------------------------------------------------------------------
def test_one_record(h):
    b = wincases.build([(77, [(T0 + 5, True)])])
    observe_all(h, [b])
    check_table(h, [b])
    assert h.table_info()["slots"] == 1024 and h.table_info()["bytes"] == 1025 * 16


def test_extreme_ids_and_times(h):
    b = wincases.build([
        (0, [(T0 + 9, True), (T0 + 3, True)]),
        (2 ** 64 - 1, [(INT64_MAX, True)]),
        (5, [(INT64_MIN, True), (7, True)]),
        (6, [(INT64_MAX, True), (INT64_MIN, False)]),       # an untimed INT64_MIN must not win
        (7, [(INT64_MIN, False), (INT64_MIN, False)]),      # no timed fragment: absent
        (8, [(INT64_MIN, False), (-1, True), (INT64_MIN, False)]),
    ])
    observe_all(h, [b])
    table, ids, t, found = check_table(h, [b])
    assert table == {0: T0 + 3, 2 ** 64 - 1: INT64_MAX, 5: INT64_MIN, 6: INT64_MAX, 8: -1}


def test_minimum_over_batches(h):
    late = 900  # timed only in batch 3
    b1 = wincases.build([(1, [(T0 + 10, True)]), (2, [(T0 + 50, True)]), (3, [(T0 + 50, True)]),
                         (late, [(INT64_MIN, False)]), (0, [(T0 + 70, True)])])
    b2 = wincases.build([(2, [(T0 + 20, True)]), (1, [(T0 + 50, True)]), (3, [(T0 + 60, True)]),
                         (late, [(INT64_MIN, False)] * 3), (0, [(T0 + 60, True)])])
    b3 = wincases.build([(3, [(T0 + 30, True)]), (late, [(T0 + 40, True)]), (1, [(T0 + 11, True)]),
                         (2, [(T0 + 21, True)]), (0, [(T0 + 65, True)])])
    observe_all(h, [b1, b2])
    _, found = h.trace_times(np.array([late], np.uint64))
    assert not found[0]
    observe_all(h, [b3])
    table, *_ = check_table(h, [b1, b2, b3])
    assert table == {1: T0 + 10, 2: T0 + 20, 3: T0 + 30, late: T0 + 40, 0: T0 + 60}


def test_observing_twice_changes_nothing(h):
    b = winref_table.shuffled(wincases.build(wincases.random_runs(61, 5000)), 61)
    d = DeviceColumns.from_host(b)
    h.observe(d)
    _, ids, t1, f1 = check_table(h, [b])
    info = h.table_info()
    h.observe(d)
    t2, f2 = h.trace_times(ids)
    assert t1.tobytes() == t2.tobytes() and f1.tobytes() == f2.tobytes()
    assert h.table_info() == info


def test_a_probe_chain_that_wraps(h):
    """300 traceIds (0 among them) whose home slot is 2040 of 2048: the chain runs off the table's end
    and goes on from slot 0. Shuffled single records: later lanes find keys earlier ones claimed."""
    slots, home = 2048, 2040
    ids = [0] + [unmix64((k << 11) | home) ^ SALT for k in range(1, 300)]
    assert all(mix64(i ^ SALT) & (slots - 1) == home for i in ids[1:]) and len(set(ids)) == 300
    rng = np.random.default_rng(5)
    tid = np.repeat(np.array(ids, np.uint64), 3)
    ts = T0 + rng.integers(0, 8 * HOUR, len(tid))
    perm = rng.permutation(len(tid))
    b = wincases.fill(tid[perm], ts[perm], np.ones(len(tid), bool))
    h.reserve(1024)
    assert h.table_info()["slots"] == slots
    observe_all(h, [b])
    assert h.table_info()["slots"] == slots
    check_table(h, [b], extra_ids=[unmix64((k << 11) | home) ^ SALT for k in range(300, 310)])


def test_one_trace_every_lane_contends(h):
    """One trace of 4096 records with distinct shuffled times: as one run (one update per row of 64,
    every wave on one slot), then as two traces whose records alternate, so that every record is a run
    of its own and every lane of every wave goes for one of two slots."""
    rng = np.random.default_rng(8)
    ts = T0 + rng.permutation(4096) * 7
    b = wincases.fill(np.full(4096, 12345, np.uint64), ts, np.ones(4096, bool))
    other = wincases.fill(np.arange(4096, dtype=np.uint64) % np.uint64(2) + np.uint64(50), ts[::-1].copy(),
                          np.ones(4096, bool))  # 50, 51, 50, 51, ...
    observe_all(h, [b, other])
    table, *_ = check_table(h, [b, other])
    assert table[12345] == T0 and min(table[50], table[51]) == T0


def test_growth_keeps_the_content(h):
    ids = wincases.Ids(9)
    rng = np.random.default_rng(9)
    batches, slots = [], []
    for n in (500, 3000, 20000):
        tid = np.array([ids() for _ in range(n)], np.uint64)
        b = wincases.fill(tid, T0 + rng.integers(0, 8 * HOUR, n), rng.integers(0, 8, n) != 0)
        batches.append(b)
        h.observe(DeviceColumns.from_host(b))
        check_table(h, batches)
        slots.append(h.table_info()["slots"])
    assert slots[0] < slots[1] < slots[2]
    for s, seen, n in zip(slots, (0, 500, 3500), (500, 3000, 20000)):
        assert s & (s - 1) == 0 and s >= 2 * (seen + n)


def test_reserve_then_reset_keeps_the_slots(h):
    b = wincases.build(wincases.random_runs(62, 2000))
    h.reserve(10_000)
    info = h.table_info()
    assert info["slots"] == 32768 and info["traces"] == 0 and info["bytes"] == (32768 + 1) * 16
    observe_all(h, [b])
    check_table(h, [b])
    h.reserve(10)  # never shrinks
    h.reset_table()
    assert h.table_info() == info
    _, found = h.trace_times(np.unique(b.trace_id))
    assert not found.any()
    observe_all(h, [b])
    check_table(h, [b])


def test_host_pointer_input(h):
    batches = winref_table.cut(winref_table.shuffled(wincases.build(wincases.random_runs(63, 4000)), 63), [1500])
    observe_all(h, batches, device=False)
    table, *_ = check_table(h, batches)
    h.set_windows(T0, HOUR, 8)
    for b in batches:
        check_partition(h, b, table, (T0, HOUR, 8), device=False)


# ---- the table-mode partition ------------------------------------------------------------------------
def check_partition(h, cols, table, rule, device=True, clustered=False):
    origin, window, W = rule
    ref_out, ref_off, ref_cnt = winref_table.partition(cols, table, origin, window, W)
    src = DeviceColumns.from_host(cols) if device else cols
    out, off, cnt = h.partition(src, table=True, clustered=clustered)
    assert np.array_equal(off, ref_off), (off, ref_off)
    assert cnt == ref_cnt
    got = out.to_host(int(off[-1]))
    for k in winref.COLS:
        assert np.array_equal(getattr(got, k), ref_out[k]), k
    return got, off, cnt


def run_case(h, cols, origin, window, W, clustered):
    h.set_windows(origin, window, W)
    h.reset_table()
    h.observe(DeviceColumns.from_host(cols))
    table = winref_table.table_of(cols)
    return check_partition(h, cols, table, (origin, window, W), clustered=clustered)


SHAPES = [f"shape_{x}" for x in wincases.SHAPE_LABELS]


@pytest.mark.parametrize("name", SHAPES + ["W1", "W1024_round_robin", "ids_0_and_max", "all_in_the_rest",
                                           "untimed_int64_min_inside_timed_runs", "crosses_edge_last"])
def test_clustered_batch(h, name):
    """n = 1, 2, chunk - 1, chunk, chunk + 1 and three ranges (zk_win_plan); W = 1 and 1024; before, after
    and untimed runs (the random runs carry all three)."""
    _, cols, origin, window, W, _ = wincases.case(name)
    _, _, cnt = run_case(h, cols, origin, window, W, clustered=True)
    if name == "W1":
        assert cnt["before_runs"] and cnt["after_runs"] and cnt["untimed_runs"]


@pytest.mark.parametrize("name", SHAPES + ["W1", "W1024_round_robin", "ids_0_and_max", "ids_repeated_not_adjacent",
                                           "covers_two_first", "rule_o-1_w1_W1024", "rule_o0_w3600000000_W1"])
def test_globally_shuffled_batch(h, name):
    _, cols, origin, window, W, _ = wincases.case(name)
    run_case(h, winref_table.shuffled(cols, 7), origin, window, W, clustered=False)


def test_cut_trace_whose_earliest_time_comes_second(h):
    """A clustered pair of batches cut inside a trace whose earliest timed fragment lies in batch 2: by
    batch 1's own records the trace belongs to window 5, by the table to window 2. Both halves land in
    window 2, at the end of batch 1's part and at the start of batch 2's."""
    cut = 0xC0FFEE
    head = wincases.random_runs(71, 1500)
    tail = wincases.random_runs(72, 1500)
    first = [(T0 + 5 * HOUR + 9, True), (INT64_MIN, False), (T0 + 5 * HOUR + 1, True)]
    second = [(INT64_MIN, False), (T0 + 2 * HOUR + 4, True), (T0 + 6 * HOUR, True)]
    b1 = wincases.build(head + [(cut, first)])
    b2 = wincases.build([(cut, second)] + tail)
    assert winref.index(min(t for t, f in first if f), T0, HOUR, 8) == 5
    h.set_windows(T0, HOUR, 8)
    observe_all(h, [b1, b2])
    table, *_ = check_table(h, [b1, b2])
    assert table[cut] == T0 + 2 * HOUR + 4
    o1, f1, _ = check_partition(h, b1, table, (T0, HOUR, 8), clustered=True)
    o2, f2, _ = check_partition(h, b2, table, (T0, HOUR, 8), clustered=True)
    a, b = int(f1[3]) - 3, int(f1[3])
    assert o1.trace_id[a:b].tolist() == [cut] * 3 and np.array_equal(o1.span_id[a:b], b1.span_id[-3:])
    a = int(f2[2])
    assert o2.trace_id[a:a + 3].tolist() == [cut] * 3 and np.array_equal(o2.span_id[a:a + 3], b2.span_id[:3])
    assert cut not in o1.trace_id[int(f1[5]):int(f1[6])].tolist()


def test_unobserved_batch_is_counted(h):
    seen = wincases.build(wincases.random_runs(73, 1200))
    unseen = wincases.build(wincases.random_runs(74, 1300))
    both = SpanColumns.concat([seen, unseen])
    both.span_id[:] = np.arange(len(both), dtype=np.uint64)
    h.set_windows(T0, HOUR, 8)
    observe_all(h, [seen])
    table = winref_table.table_of(seen)
    _, _, cnt = check_partition(h, both, table, (T0, HOUR, 8), clustered=True)
    timed = (unseen.flags & np.uint32(winref.HAS_ANNOTATIONS)) != 0
    assert cnt["unobserved_records"] == int(timed.sum()) > 0
    h.reset_table()
    _, _, cnt = check_partition(h, seen, {}, (T0, HOUR, 8), clustered=True)
    assert cnt["untimed_records"] == len(seen)


def test_counts_outside_table_mode_report_no_unobserved_records(h):
    cols = wincases.build(wincases.random_runs(75, 900))
    h.set_windows(T0, HOUR, 8)
    src = DeviceColumns.from_host(cols)
    h.observe(src)  # (a table in the handle changes nothing without the flag)
    off = (C.c_uint64 * 10)()
    raw = _abi.zk_win_counts()
    raw.unobserved_records = 99
    ab, ob = src.abi(), DeviceColumns(len(cols), device=src.trace_id.device).abi(len(cols))
    st = _abi.lib().zk_win_partition(h._h, C.byref(ab), _abi.ZK_BATCH_DEVICE_PTRS | _abi.ZK_BATCH_TRACE_CLUSTERED,
                                     C.byref(ob), off, C.byref(raw))
    assert st == _abi.ZK_OK and raw.unobserved_records == 0 and not any(raw.reserved)
    assert raw.as_dict() == winref.partition(cols, T0, HOUR, 8)[2]


def test_refusals_leave_out_unwritten(h, gpu):
    import torch

    cols = wincases.build(wincases.random_runs(76, 3000))
    src = DeviceColumns.from_host(cols)
    h.observe(src)
    out = DeviceColumns(len(cols), device=f"cuda:{gpu}")
    for k in winref.COLS:
        getattr(out, k).fill_(0x5A5A5A5A)
    torch.cuda.synchronize()
    before = out.to_host()
    with pytest.raises(ZkError) as e:
        h.partition(src, out=out, table=True, hold_last=True)
    assert e.value.status == _abi.ZK_ERR_INVALID_ARG
    with pytest.raises(ZkError) as e:
        h.partition(src, out=out, clustered=False)  # without the flag: as before
    assert e.value.status == _abi.ZK_ERR_UNSUPPORTED
    ab, ob = src.abi(), out.abi(len(cols))
    ob.first_ts = src.last_ts.data_ptr()
    off = (C.c_uint64 * 10)()
    st = _abi.lib().zk_win_partition(h._h, C.byref(ab), _abi.ZK_BATCH_DEVICE_PTRS | _abi.ZK_WIN_TRACE_TABLE,
                                     C.byref(ob), off, None)
    assert st == _abi.ZK_ERR_INVALID_ARG
    L = _abi.lib()
    assert L.zk_win_observe(h._h, None, 0) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_win_observe(h._h, C.byref(ab), 1 << 20) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_win_table_lookup(h._h, None, 4, 0, None, None) == _abi.ZK_ERR_INVALID_ARG
    after = out.to_host()
    for k in winref.COLS:
        assert np.array_equal(getattr(after, k), getattr(before, k)), k


def test_repeatable_bytes(h, gpu):
    cols = winref_table.shuffled(wincases.build(wincases.random_runs(77, wincases.smallest_n_with_ranges(3) + 77)), 77)
    a, off_a, _ = run_case(h, cols, T0, HOUR, 8, clustered=False)
    table = winref_table.table_of(cols)
    b, off_b, _ = check_partition(h, cols, table, (T0, HOUR, 8))
    with WindowPartition(window_us=HOUR, origin_us=T0, num_windows=8, device=gpu) as fresh:
        c, off_c, _ = run_case(fresh, cols, T0, HOUR, 8, clustered=False)
    for k in winref.COLS:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes() == getattr(c, k).tobytes()
    assert off_a.tobytes() == off_b.tobytes() == off_c.tobytes()


def test_phase_times_in_table_mode(gpu):
    cols = wincases.build(wincases.random_runs(78, 5000))
    with WindowPartition(window_us=HOUR, origin_us=T0, num_windows=8, device=gpu, timing=True) as t:
        t.observe(DeviceColumns.from_host(cols))
        ms = t.observe_ms()
        assert set(ms) == {"runs", "grow", "insert"} and all(v >= 0 for v in ms.values())
        t.partition(DeviceColumns.from_host(cols), table=True)
        ph = t.phase_ms()
        assert ph["resolve"] == 0.0 and ph["time"] > 0
