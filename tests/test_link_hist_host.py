"""The per-link duration histogram (include/zksketch.h zk_lh_*) without a device: the Python bin
helper LinkHistogram maps bin indices with against the oracle's layout (oracle/realtime.py), the
argument checks that come before any device is touched, and the struct sizes the additive ABI change
must keep."""
import ctypes as C

import pytest

from oracle.realtime import bin_bounds, bins_of, nbins
from zipkin_amd import _abi
from zipkin_amd.realtime import link_hist_bin_bounds, link_hist_bins


@pytest.mark.parametrize("m", range(2, 8))
def test_bin_helper_equals_the_oracle_layout(m):
    assert link_hist_bins(m) == nbins(m)
    for d in (0, 1, (1 << m) - 1, 1 << m, (1 << m) + 1, 1 << 20, (1 << 40) - 1):
        b = int(bins_of([d], m)[0])
        lo, hi = link_hist_bin_bounds(b, m)
        assert (lo, hi) == bin_bounds(b, m)
        assert lo <= d <= hi
    assert int(bins_of([(1 << 40) - 1], m)[0]) == nbins(m) - 1
    # every bin: the same bounds, and the bins tile [0, 2^40) without gaps
    nxt = 0
    for b in range(nbins(m)):
        lo, hi = link_hist_bin_bounds(b, m)
        assert (lo, hi) == bin_bounds(b, m) and lo == nxt
        nxt = hi + 1
    assert nxt == 1 << 40


def test_create_rejects_bad_config_without_touching_a_device():
    L = _abi.lib()
    h = C.c_void_p()
    assert L.zk_lh_create(None, C.byref(h)) == _abi.ZK_ERR_INVALID_ARG
    for S, m in ((0, 0), (5000, 0), (10, 1), (10, 8)):
        cfg = _abi.zk_lh_config()
        cfg.num_services, cfg.sub_bits = S, m
        assert L.zk_lh_create(C.byref(cfg), C.byref(h)) == _abi.ZK_ERR_INVALID_ARG, (S, m)
        assert not h.value


def test_null_handle_calls_are_errors():
    L = _abi.lib()
    E = _abi.ZK_ERR_INVALID_ARG
    q = (C.c_double * 1)(0.5)
    lo, hi = (C.c_int64 * 1)(), (C.c_int64 * 1)()
    n, b = C.c_uint64(), C.c_uint32()
    p = C.c_void_p()
    out = (C.c_uint32 * 4)()
    assert L.zk_lh_destroy(None) == E
    assert L.zk_lh_reset(None) == E
    assert L.zk_lh_geometry(None, C.byref(b)) == E
    assert L.zk_lh_bind(None, None) == E
    assert L.zk_lh_quantiles(None, 0, 0, q, 1, lo, hi, C.byref(n)) == E
    assert L.zk_lh_quantiles_all(None, q, 1, lo, hi, C.byref(n)) == E
    assert L.zk_lh_read(None, 0, 0, out) == E
    assert L.zk_lh_partial(None, C.byref(p), C.byref(n)) == E
    assert L.zk_lh_dropped(None, C.byref(n)) == E
    assert L.zk_lh_allreduce(None, None) == E
    assert L.zk_lh_last_error(None)


def test_struct_sizes_are_those_of_the_parent_abi():
    # zk_timing: 9 x 8 B + reserved[2] doubles -> link_hist_ms / link_hist_ms_total in their place
    assert C.sizeof(_abi.zk_timing) == 88
    assert C.sizeof(_abi.zk_config) == 80
    assert _abi.zk_timing.link_hist_ms.offset == 72 and _abi.zk_timing.link_hist_ms_total.offset == 80
    assert _abi.lib().zk_abi_version() == 3
