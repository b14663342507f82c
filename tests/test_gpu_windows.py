"""The device trace-time partition (include/zkwindow.h, zk_win.hip) against tests/winref.py: exact
equality of all seven output columns, the offsets and the counts, on batches aimed at the edges of
the kernels' geometry (tests/wincases.py), then the dependency path over the slices."""
import ctypes as C

import numpy as np
import pytest

from tests import wincases, winref
from tests.wincases import HOUR, T0
from zipkin_amd import DepsContext, DeviceColumns, WindowPartition, ZkError, _abi, tracegen_host
from zipkin_amd.windows import window_slice

pytestmark = pytest.mark.gpu

NAMES = wincases.names()
SHAPES = [x for x in NAMES if x.startswith("shape_")]


@pytest.fixture(scope="module")
def handle(gpu):
    with WindowPartition(window_us=HOUR, origin_us=T0, num_windows=8, device=gpu) as h:
        yield h


def check(h, case, device_ptrs=True):
    _, cols, origin, window, W, hold = case
    h.set_windows(origin, window, W)
    ref_out, ref_off, ref_cnt = winref.partition(cols, origin, window, W, hold)
    src = DeviceColumns.from_host(cols) if device_ptrs else cols
    out, off, cnt = h.partition(src, hold_last=hold)
    assert np.array_equal(off, ref_off), (off, ref_off)
    assert cnt == ref_cnt
    got = out.to_host(int(off[-1]))
    for k in winref.COLS:
        assert np.array_equal(getattr(got, k), ref_out[k]), k
    return out, off, cnt


@pytest.mark.parametrize("name", NAMES)
def test_partition_equals_the_reference(handle, name):
    check(handle, wincases.case(name))


@pytest.mark.parametrize("name", SHAPES)
def test_host_pointer_input(handle, name):
    check(handle, wincases.case(name), device_ptrs=False)


def test_empty_batch(handle):
    handle.set_windows(T0, HOUR, 8)
    out, off, cnt = handle.partition(wincases.build([]))
    assert not off.any() and not any(cnt.values())


def _prefilled(n, gpu):
    import torch

    out = DeviceColumns(n, device=f"cuda:{gpu}")
    for k in winref.COLS:
        getattr(out, k).fill_(0x5A5A5A5A)
    torch.cuda.synchronize()
    return out


def test_refusals_leave_out_unwritten(handle, gpu):
    cols = wincases.build(wincases.random_runs(41, 3000))
    handle.set_windows(T0, HOUR, 8)
    src = DeviceColumns.from_host(cols)
    out = _prefilled(len(cols), gpu)
    before = out.to_host()
    with pytest.raises(ZkError) as e:
        handle.partition(src, out=out, clustered=False)
    assert e.value.status == _abi.ZK_ERR_UNSUPPORTED
    # out overlapping in: one column of out IS a column of in, then overlaps it partly
    for shift in (0, 1000):
        ab, ob = src.abi(), out.abi(len(cols))
        ob.first_ts = src.last_ts.data_ptr() + 8 * shift
        off = (C.c_uint64 * 10)()
        st = _abi.lib().zk_win_partition(handle._h, C.byref(ab), _abi.ZK_BATCH_DEVICE_PTRS | _abi.ZK_BATCH_TRACE_CLUSTERED,
                                         C.byref(ob), off, None)
        assert st == _abi.ZK_ERR_INVALID_ARG
    after = out.to_host()
    for k in winref.COLS:
        assert np.array_equal(getattr(after, k), getattr(before, k)), k
    same = src.to_host()
    for k in winref.COLS:
        assert np.array_equal(getattr(same, k), getattr(cols, k)), k


def test_repeatable_bytes(handle, gpu):
    case = ("repeat", wincases.build(wincases.random_runs(43, wincases.smallest_n_with_ranges(4) + 77)), T0, HOUR, 8, False)
    a, off_a, _ = check(handle, case)
    b, off_b, _ = check(handle, case)
    with WindowPartition(window_us=HOUR, origin_us=T0, num_windows=8, device=gpu) as fresh:
        c, off_c, _ = check(fresh, case)
    ha, hb, hc = a.to_host(), b.to_host(), c.to_host()
    for k in winref.COLS:
        assert getattr(ha, k).tobytes() == getattr(hb, k).tobytes() == getattr(hc, k).tobytes()
    assert off_a.tobytes() == off_b.tobytes() == off_c.tobytes()


# ---- the dependency path over the slices ----------------------------------------------------------
S = 61
BASE_TS = 1_421_053_208_373_000


@pytest.fixture(scope="module")
def tracegen(gpu):
    """About 2e5 TraceGen records (traces start 1-8 hours before BASE_TS), partitioned by the hour."""
    cols = tracegen_host(seed=7, num_traces=5500, max_depth=7, num_services=S, base_ts=BASE_TS)
    timed = (cols.flags & np.uint32(_abi.ZK_F_HAS_ANNOTATIONS)) != 0
    origin = int(cols.first_ts[timed].min()) // HOUR * HOUR
    W = (int(cols.first_ts[timed].max()) - origin) // HOUR + 1
    with WindowPartition(window_us=HOUR, origin_us=origin, num_windows=W, device=gpu) as h:
        out, off, cnt = check(h, ("tracegen", cols, origin, HOUR, W, False))
    return cols, origin, W, out, off, cnt


def _finalized(ctx):
    t = ctx.finalize()
    return t, ctx.stats()


def test_whole_equals_the_parts(tracegen, gpu):
    cols, origin, W, out, off, _ = tracegen
    assert 150_000 <= len(cols) <= 400_000 and 7 <= W <= 10
    with DepsContext(S, device=gpu) as ctx:
        ctx.accumulate(DeviceColumns.from_host(cols), clustered=True, verify=True)
        whole, whole_stats = _finalized(ctx)
        ctx.reset()
        for w in range(W + 1):
            a, b = int(off[w]), int(off[w + 1])
            if b > a:
                ctx.accumulate(window_slice(out, a, b), clustered=True, verify=True)
        parts, parts_stats = _finalized(ctx)
    for k in ("m0", "m1", "m2", "m3", "m4", "present"):
        assert getattr(whole, k).tobytes() == getattr(parts, k).tobytes(), k
    assert whole_stats == parts_stats


def test_each_window_equals_the_oracle(tracegen, gpu):
    from oracle import oracle

    cols, origin, W, out, off, _ = tracegen
    with DepsContext(S, device=gpu) as ctx:
        ctx.accumulate(DeviceColumns.from_host(cols), clustered=True, verify=True)
        plain = ctx.finalize()
        total = np.zeros_like(plain.m0)
        nonempty = 0
        for w in range(W + 1):
            a, b = int(off[w]), int(off[w + 1])
            sel = winref.window_records(cols, origin, HOUR, W, w)
            assert len(sel) == b - a
            if b == a:
                continue
            ctx.reset()
            ctx.accumulate(window_slice(out, a, b), clustered=True, verify=True)
            got = ctx.finalize()
            ref = oracle.aggregate(cols.take(sel), S)
            m0, ms = ref.dense()
            assert np.array_equal(got.m0, m0), w
            for x, y, name in zip((got.m1, got.m2, got.m3, got.m4), ms, ("m1", "m2", "m3", "m4")):
                assert np.array_equal(x, y), (w, name)
            total += got.m0
            nonempty += int(got.m0.sum() > 0)
    assert nonempty >= 7
    assert np.array_equal(total, plain.m0)
