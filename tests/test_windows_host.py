"""The host half of the window partition (include/zkwindow.h), no GPU: zk_win_index against the
reference rule at every boundary, zk_win_create's argument checks, zk_win_plan's geometry, and the
reference's own invariants on the case list the GPU tests run."""
import ctypes as C

import numpy as np
import pytest

from tests import wincases, winref
from tests.wincases import HOUR, I64_EDGES, INT64_MAX, INT64_MIN, WINDOWS, WS
from zipkin_amd import _abi
from zipkin_amd.windows import plan, window_index


def test_index_equals_the_reference_at_every_boundary():
    checked = 0
    for origin in I64_EDGES:
        for window in WINDOWS:
            for W in WS:
                for t in wincases.rule_times(origin, window, W):
                    assert window_index(t, origin, window, W) == winref.index(t, origin, window, W), (t, origin, window, W)
                    checked += 1
    assert checked >= 5 * 3 * 2 * 5


def test_index_known_values():
    assert window_index(0, 0, HOUR, 8) == 0
    assert window_index(HOUR - 1, 0, HOUR, 8) == 0
    assert window_index(HOUR, 0, HOUR, 8) == 1
    assert window_index(8 * HOUR - 1, 0, HOUR, 8) == 7
    assert window_index(8 * HOUR, 0, HOUR, 8) == 8  # after
    assert window_index(-1, 0, HOUR, 8) == 8  # before
    assert window_index(INT64_MAX, INT64_MIN, INT64_MAX, 1024) == 2  # no signed subtraction
    assert window_index(INT64_MIN, INT64_MAX, 1, 1) == 1


def test_index_rejects_a_bad_rule():
    L = _abi.lib()
    w = C.c_uint32()
    for window, W in ((0, 1), (-1, 1), (1, 0), (1, 1025)):
        assert L.zk_win_index(0, 0, window, W, C.byref(w)) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_win_index(0, 0, 1, 1, None) == _abi.ZK_ERR_INVALID_ARG


@pytest.mark.parametrize("window,W", [(0, 1), (-5, 1), (HOUR, 0), (HOUR, 1025)])
def test_create_rejects_a_bad_config_without_a_device(window, W):
    L = _abi.lib()
    cfg = _abi.zk_win_config()
    cfg.device = 12345  # never looked at: the rule is checked first
    cfg.window_us, cfg.num_windows = window, W
    h = C.c_void_p()
    assert L.zk_win_create(C.byref(cfg), C.byref(h)) == _abi.ZK_ERR_INVALID_ARG
    assert not h.value
    assert L.zk_win_create(None, C.byref(h)) == _abi.ZK_ERR_INVALID_ARG


def test_null_handle_calls_are_errors():
    L = _abi.lib()
    assert L.zk_win_destroy(None) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_win_set_windows(None, 0, 1, 1) == _abi.ZK_ERR_INVALID_ARG
    assert L.zk_win_partition(None, None, 0, None, None, None) == _abi.ZK_ERR_INVALID_ARG


def test_plan_cuts_whole_chunks_and_covers_n():
    c = plan(1)[0]
    assert plan(0) == (c, c, 0)
    for n in (1, c - 1, c, c + 1, 2 * c, 2 * c + 1, 10 ** 6 + 3, 10 ** 8, 2 ** 33 + 1):
        ch, rr, k = plan(n)
        assert ch == c and rr % c == 0 and rr >= c
        assert (k - 1) * rr < n <= k * rr  # the ranges cover n and the last is not empty
        assert k <= 2048
    assert wincases.smallest_n_with_ranges(3) == 2 * c + 1
    assert wincases.smallest_n_with_ranges(4) == 3 * c + 1


NAMES = wincases.names()


@pytest.mark.parametrize("name", NAMES)
def test_reference_invariants(name):
    _, cols, origin, window, W, hold = wincases.case(name)
    n = len(cols)
    out, offsets, counts = winref.partition(cols, origin, window, W, hold)
    kept = counts["held_from"]
    assert len(offsets) == W + 2 and offsets[0] == 0 and int(offsets[-1]) == kept
    assert all(int(a) <= int(b) for a, b in zip(offsets, offsets[1:]))  # monotone
    # a permutation of the records before held_from (span_id is the input index)
    assert np.array_equal(np.sort(out["span_id"]), np.arange(kept, dtype=np.uint64))
    for k in winref.COLS:
        assert np.array_equal(out[k], getattr(cols, k)[out["span_id"].astype(np.int64)])
    # every run is intact: its records adjacent and in input order, inside one part
    starts = winref.run_starts(cols.trace_id)
    ends = np.concatenate((starts[1:], [n]))
    where = np.empty(kept, np.int64)
    where[out["span_id"].astype(np.int64)] = np.arange(kept)
    part_of = np.searchsorted(offsets[1:].astype(np.int64), np.arange(kept), side="right")
    for a, b in zip(starts.tolist(), ends.tolist()):
        if a >= kept:
            assert hold and b == n
            continue
        assert np.array_equal(where[a:b], where[a] + np.arange(b - a))
        assert len(set(part_of[where[a:b]].tolist())) == 1
    # inside each part the input order is kept
    for w in range(W + 1):
        ids = out["span_id"][int(offsets[w]):int(offsets[w + 1])]
        assert np.all(ids[1:] > ids[:-1])
    assert counts["partitioned_records"] == int(offsets[W])
    assert (counts["before_records"] + counts["after_records"] + counts["untimed_records"]
            == int(offsets[W + 1]) - int(offsets[W]))
    assert (counts["partitioned_runs"] + counts["before_runs"] + counts["after_runs"] + counts["untimed_runs"]
            + counts["held_runs"] == len(starts))
