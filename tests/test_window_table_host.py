"""The table-mode window partition without a device: the reference's own invariants (tests/winref_table.py),
the cut-trace property that lets ZK_BATCH_CONTINUES join a trace cut at a batch edge, and the additions
to the C ABI (include/zkwindow.h) as far as a host without a GPU can see them."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import wincases, winref, winref_table
from tests.wincases import HOUR, T0
from zipkin_amd import _abi

ROOT = Path(__file__).resolve().parent.parent
W = 8


def clustered_set(seed, n=6000):
    """A trace-clustered batch whose runs have times in and around W windows."""
    return wincases.build(wincases.random_runs(seed, n))


def windows_of(parts_cls):
    """{traceId: set of parts it lies in} over [(cols, cls)]."""
    seen = {}
    for cols, cls in parts_cls:
        for tid, c in zip(cols.trace_id.tolist(), np.minimum(cls, W).tolist()):
            seen.setdefault(tid, set()).add(c)
    return seen


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reference_is_a_stable_permutation(seed):
    cols = winref_table.shuffled(clustered_set(seed), seed)
    table = winref_table.table_of(cols)
    out, off, cnt = winref_table.partition(cols, table, T0, HOUR, W)
    # span_id is the record's index in the unshuffled batch: every record once
    assert sorted(out["span_id"].tolist()) == list(range(len(cols.trace_id)))
    assert int(off[-1]) == len(cols.trace_id) and cnt["unobserved_records"] == 0
    pos = {s: i for i, s in enumerate(cols.span_id.tolist())}
    for w in range(W + 1):
        inp = [pos[s] for s in out["span_id"][int(off[w]):int(off[w + 1])].tolist()]
        assert inp == sorted(inp)  # the input's relative order is kept inside a part


@pytest.mark.parametrize("seed", [4, 5])
@pytest.mark.parametrize("order", ["rows", "any"])
def test_every_trace_of_every_batch_lands_in_one_window(seed, order):
    cols = clustered_set(seed)
    if order == "any":
        cols = winref_table.shuffled(cols, seed)
    rng = np.random.default_rng(seed)
    batches = winref_table.cut(cols, rng.integers(1, len(cols.trace_id), 4))
    table = winref_table.table_of(batches)
    seen = windows_of([(b, winref_table.classify(b, table, T0, HOUR, W)) for b in batches])
    assert all(len(v) == 1 for v in seen.values())
    # ... and it is the window the whole set's own rule gives the trace
    starts, cls = winref.classify(clustered_set(seed), T0, HOUR, W)
    whole = clustered_set(seed)
    for s, c in zip(starts.tolist(), cls.tolist()):
        assert seen[int(whole.trace_id[s])] == {min(c, W)}


@pytest.mark.parametrize("seed", [6, 7, 8])
def test_clustered_parts_stay_clustered_and_cut_traces_meet(seed):
    cols = clustered_set(seed)
    rng = np.random.default_rng(seed)
    # random cuts, and one placed inside a run of more than one record
    starts = winref.run_starts(cols.trace_id)
    long_runs = starts[:-1][np.diff(starts) > 3]
    cuts = sorted(set(rng.integers(1, len(cols.trace_id), 3).tolist() + [int(long_runs[len(long_runs) // 2]) + 2]))
    batches = winref_table.cut(cols, cuts)
    table = winref_table.table_of(batches)
    parts = [winref_table.partition(b, table, T0, HOUR, W) for b in batches]
    for out, off, _ in parts:
        for w in range(W + 1):
            ids = out["trace_id"][int(off[w]):int(off[w + 1])]
            assert len(winref.run_starts(ids)) == len(set(ids.tolist()))  # no id recurs after its run
    met = 0
    for k, c in enumerate(cuts):
        tid = int(cols.trace_id[c])
        if int(cols.trace_id[c - 1]) != tid:
            continue  # the cut fell between two traces
        w = min(int(winref_table.classify(batches[k], table, T0, HOUR, W)[-1]), W)
        (oa, fa, _), (ob, fb, _) = parts[k], parts[k + 1]
        assert int(oa["trace_id"][int(fa[w + 1]) - 1]) == tid  # the last run of batch k's part ...
        assert int(ob["trace_id"][int(fb[w])]) == tid         # ... is the first run of batch k + 1's
        met += 1
    assert met >= 1


def test_unobserved_records_are_untimed_and_counted():
    cols = clustered_set(9, 500)
    out, off, cnt = winref_table.partition(cols, {}, T0, HOUR, W)
    timed = (cols.flags & np.uint32(winref.HAS_ANNOTATIONS)) != 0
    assert cnt["unobserved_records"] == int(timed.sum()) > 0
    assert cnt["untimed_records"] == len(cols.trace_id) == int(off[W + 1]) - int(off[W])
    assert np.array_equal(out["span_id"], cols.span_id)


# ---- the C ABI ---------------------------------------------------------------------------------------
def test_counts_struct_keeps_its_size_and_earlier_offsets():
    c = _abi.zk_win_counts
    assert C.sizeof(c) == 16 * 8
    earlier = ("partitioned_runs", "partitioned_records", "before_runs", "before_records", "after_runs",
               "after_records", "untimed_runs", "untimed_records", "held_runs", "held_records", "held_from")
    for k, name in enumerate(earlier):
        assert getattr(c, name).offset == 8 * k, name
    assert c.unobserved_records.offset == 8 * 11
    assert c.reserved.offset == 8 * 12 and c.reserved.size == 4 * 8
    assert "unobserved_records" in c().as_dict(table=True) and "unobserved_records" not in c().as_dict()


def test_header_and_mirror_agree():
    h = (ROOT / "include" / "zkwindow.h").read_text()
    assert re.search(r"#define\s+ZK_WIN_TRACE_TABLE\s+\(1u << 9\)", h)
    assert _abi.ZK_WIN_TRACE_TABLE == 1 << 9 and _abi.ZK_WIN_HOLD_LAST == 1 << 8
    m = re.search(r"#define\s+ZK_WIN_TABLE_SALT\s+0x([0-9A-Fa-f]+)ull", h)
    assert m and int(m.group(1), 16) == _abi.ZK_WIN_TABLE_SALT
    assert re.search(r"uint64_t\s+unobserved_records;", h) and re.search(r"uint64_t\s+reserved\[4\];", h)
    # the header states the table's semantics
    for word in ("MEMBERSHIP", "IDEMPOTENCE", "SIZING", "zk_mix64(trace_id ^ ZK_WIN_TABLE_SALT) & (slots - 1)"):
        assert word in h, word


def test_abi_version_is_unchanged():
    assert _abi.lib().zk_abi_version() == 3


NEW = ("zk_win_observe", "zk_win_observe_ms", "zk_win_table_reset", "zk_win_table_reserve", "zk_win_table_info",
       "zk_win_table_lookup")


@pytest.mark.parametrize("name", NEW)
def test_new_symbols_exist(name):
    assert getattr(_abi.lib(), name) is not None
    assert re.search(r"zk_status\s+%s\(" % name, (ROOT / "include" / "zkwindow.h").read_text())


def test_null_handles_are_refused_without_a_device():
    L = _abi.lib()
    bad = _abi.ZK_ERR_INVALID_ARG
    cols = wincases.build(wincases.random_runs(1, 10)).abi()
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    ids = (C.c_uint64 * 2)(1, 2)
    t = (C.c_int64 * 2)()
    f = (C.c_uint8 * 2)()
    ms = (C.c_double * 3)()
    assert L.zk_win_observe(None, C.byref(cols), 0) == bad
    assert L.zk_win_observe_ms(None, ms) == bad
    assert L.zk_win_table_reset(None) == bad
    assert L.zk_win_table_reserve(None, 100) == bad
    assert L.zk_win_table_info(None, C.byref(a), C.byref(b), C.byref(c)) == bad
    assert L.zk_win_table_lookup(None, ids, 2, 0, t, f) == bad
    off = (C.c_uint64 * 10)()
    flags = _abi.ZK_WIN_TRACE_TABLE | _abi.ZK_WIN_HOLD_LAST
    assert L.zk_win_partition(None, C.byref(cols), flags, C.byref(cols), off, None) == bad
    assert (a.value, b.value, c.value) == (0, 0, 0) and not any(t) and not any(f)


def test_python_surface():
    from zipkin_amd import WindowPartition
    from zipkin_amd.windows import WindowedAggregateJob

    for name in ("observe", "reset_table", "reserve", "table_info", "trace_times", "observe_ms"):
        assert callable(getattr(WindowPartition, name))
    assert WindowedAggregateJob([], window_us=HOUR).order == "whole"
    for order in ("rows", "any"):
        assert WindowedAggregateJob([], window_us=HOUR, order=order).order == order
    with pytest.raises(ValueError):
        WindowedAggregateJob([], window_us=HOUR, order="sorted")
