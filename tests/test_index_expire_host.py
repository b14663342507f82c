"""The host side of index retention (zipkin_amd/retention.py; zk_ix_expire, zk_ax_expire, zk_td_expire and
their *_expire_ms): the NULL-handle refusals, which touch no device, and IndexRetention's arithmetic over
duck-typed indices."""
import ctypes as C

import pytest

import zipkin_amd
from zipkin_amd import IndexRetention, _abi

INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
DAY_US = 24 * 3600 * 1_000_000


def test_null_handles_are_refused():
    L = _abi.lib()
    n = C.c_uint64(99)
    ms = (C.c_double * 3)(7.0, 7.0, 7.0)
    for pre in ("zk_ix", "zk_ax", "zk_td"):
        assert getattr(L, pre + "_expire")(None, 0, C.byref(n)) == _abi.ZK_ERR_INVALID_ARG
        assert getattr(L, pre + "_expire")(None, INT64_MIN, None) == _abi.ZK_ERR_INVALID_ARG
        assert getattr(L, pre + "_expire_ms")(None, ms) == _abi.ZK_ERR_INVALID_ARG
    assert n.value == 99 and list(ms) == [7.0] * 3


class FakeIndex:
    """expire(cutoff) -> the number of its timestamps below the cutoff, which leave."""

    def __init__(self, ts):
        self.ts = list(ts)
        self.cutoffs = []

    def expire(self, cutoff):
        self.cutoffs.append(cutoff)
        before = len(self.ts)
        self.ts = [t for t in self.ts if t >= cutoff]
        return before - len(self.ts)


def test_default_ttl_is_the_references_three_days():
    r = IndexRetention()
    assert r.getDataTimeToLive() == 3 * 24 * 3600 and isinstance(r.getDataTimeToLive(), int)
    assert r.expire(10 * DAY_US) == {"cutoff": 7 * DAY_US, "names": 0, "annotations": 0, "durations": 0}
    assert zipkin_amd.IndexRetention is IndexRetention and "IndexRetention" in zipkin_amd.__all__


def test_cutoff_arithmetic_and_removed_counts():
    names, anns, durs = FakeIndex([5, 999_999, 1_000_000, 2_000_000]), FakeIndex([0, 1_000_001]), FakeIndex([-7, 1_000_000])
    r = IndexRetention(1, names=names, annotations=anns, durations=durs)
    assert r.getDataTimeToLive() == 1
    assert r.expire(2_000_000) == {"cutoff": 1_000_000, "names": 2, "annotations": 1, "durations": 1}
    assert names.ts == [1_000_000, 2_000_000] and anns.ts == [1_000_001] and durs.ts == [1_000_000]  # ts == cutoff stays
    assert names.cutoffs == anns.cutoffs == durs.cutoffs == [1_000_000]  # ONE cutoff for all three
    assert r.expire(2_000_000) == {"cutoff": 1_000_000, "names": 0, "annotations": 0, "durations": 0}


def test_negative_now_and_the_ends_of_int64():
    idx = FakeIndex([-5_000_000, -3_000_001, -3_000_000, 0])
    r = IndexRetention(2, names=idx)
    assert r.expire(-1_000_000) == {"cutoff": -3_000_000, "names": 2, "annotations": 0, "durations": 0}
    assert idx.ts == [-3_000_000, 0]
    assert r.cutoff(INT64_MIN) == INT64_MIN and r.cutoff(INT64_MIN + 2_000_000) == INT64_MIN  # no wrap below int64
    assert r.cutoff(INT64_MIN + 2_000_001) == INT64_MIN + 1
    assert r.cutoff(INT64_MAX) == INT64_MAX - 2_000_000
    assert r.expire(INT64_MIN)["names"] == 0 and idx.ts == [-3_000_000, 0]


def test_sharded_lists_are_summed():
    n0, n1 = FakeIndex([1, 2, 30_000_000]), FakeIndex([3, 40_000_000])
    d0, d1, d2 = FakeIndex([1]), FakeIndex([]), FakeIndex([2, 50_000_000])
    r = IndexRetention(10, names=[n0, n1], annotations=(), durations=(d0, d1, d2))
    assert r.expire(30_000_000) == {"cutoff": 20_000_000, "names": 3, "annotations": 0, "durations": 2}
    assert [len(x.ts) for x in (n0, n1, d0, d1, d2)] == [1, 1, 0, 0, 1]


@pytest.mark.parametrize("ttl", (0, -1, -3 * 24 * 3600))
def test_a_ttl_that_is_not_positive_is_refused(ttl):
    with pytest.raises(ValueError):
        IndexRetention(ttl)
    with pytest.raises(ValueError):
        IndexRetention(ttl_seconds=ttl, names=FakeIndex([]))
