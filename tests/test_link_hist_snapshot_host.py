"""The host side of link-histogram snapshots (include/zksketch.h zk_lh_snapshot_*, include/zkstore.h
zk_store_put_dependencies_hist / zk_store_get_link_hist), on the CPU: validate, plus, remap and
quantiles against the independent format reference tests/lhsnap.py and the oracle's nearest-rank rule,
the store's attachment under each backend's window semantics, and the ASan + UBSan fuzz program of
tools/sanitize."""
import ctypes as C
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle.realtime import bin_bounds, nearest_rank
from tests import lhsnap
from zipkin_amd import ZkError, _abi
from zipkin_amd.aggregates import DAY_US, Dependencies, DependencyLink, Dictionary, GpuAggregates, Moments, Service
from zipkin_amd.realtime import LinkHistogramSnapshot

ROOT = Path(__file__).resolve().parent.parent
U32 = 2**32 - 1


def validate(blob: bytes) -> int:
    buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(blob or b"\0")  # exactly the blob, no slack after it
    return _abi.lib().zk_lh_snapshot_validate(buf if blob else None, len(blob))


def sparse(seed, S, m, cells=6, per_row=5, high=1000):
    rng = np.random.default_rng(seed)
    d = np.zeros((S * S, lhsnap.nbins(m)), np.uint32)
    for c in rng.choice(S * S, min(cells, S * S), replace=False):
        b = rng.choice(lhsnap.nbins(m), per_row, replace=False)
        d[c, b] = rng.integers(1, high, per_row)
    return d


# ---- validate ---------------------------------------------------------------------------------------
def test_validate_accepts_the_reference_encoding():
    for m in (2, 3, 4, 5, 6, 7):
        for S in (1, 3, 7):
            blob = lhsnap.encode(sparse(m * 10 + S, S, m), S, m, dropped=S)
            assert validate(blob) == _abi.ZK_OK
            got, gm, dropped = lhsnap.decode(blob, S)
            assert gm == m and dropped == S
    empty = lhsnap.encode(np.zeros((9, lhsnap.nbins(4)), np.uint32), 3, 4)
    assert len(empty) == 64 and validate(empty) == _abi.ZK_OK
    assert lhsnap.pack(2, [(0, 1, 0), (2, 0, 2)], [(0, 1), (155, 7), (3, U32)]) == lhsnap.encode(
        np.array(lhsnap.decode(lhsnap.pack(2, [(0, 1, 0), (2, 0, 2)], [(0, 1), (155, 7), (3, U32)]), 3)[0]), 3, 2)


GOOD_ROWS = [(0, 1, 0), (0, 2, 2), (3, 0, 3)]
GOOD_ENTRIES = [(0, 5), (9, 1), (4, 2), (1, 1), (155, 3)]


def _with(rows=GOOD_ROWS, entries=GOOD_ENTRIES, **kw):
    return lhsnap.pack(2, rows, entries, **kw)


def _head(blob, **kw):
    """The blob under another header (rows / entries / links as the blob's unless given)."""
    _, m, _, rows, entries, links, dropped = struct.unpack_from("<IIIQQQQ", blob, 4)
    args = dict(m=m, rows=rows, entries=entries, links=links, dropped=dropped)
    args.update(kw)
    return lhsnap.header(**args) + blob[64:]


BAD = {
    "magic": _head(_with(), magic=b"ZKLX"),
    "version": _head(_with(), version=2),
    "m below 2": _head(_with(), m=1, bins=lhsnap.nbins(2)),
    "m above 7": _head(_with(), m=8, bins=lhsnap.nbins(2)),
    "another m than the bins": _head(_with(), m=3, bins=lhsnap.nbins(2)),
    "bins != (41 - m) << m": _head(_with(), bins=157),
    "padding": _with()[:48] + b"\1" + _with()[49:],
    "length: a byte more": _with() + b"\0",
    "length: an entry more": _with() + bytes(8),
    "length: rows claim more": _head(_with(), rows=4),
    "length: entries claim fewer": _head(_with(), entries=4, links=9),
    "length: huge rows": _head(_with(), rows=2**60),
    "length: rows * 16 wraps": _head(_with(), rows=2**60 + 3, entries=5),
    "rows equal": _with(rows=[(0, 1, 0), (0, 1, 2), (3, 0, 3)]),
    "rows descending by child": _with(rows=[(0, 2, 0), (0, 1, 2), (3, 0, 3)]),
    "rows descending by parent": _with(rows=[(3, 0, 0), (0, 2, 2), (0, 3, 3)]),
    "first of row 0 not 0": _with(rows=[(0, 1, 1), (0, 2, 2), (3, 0, 3)]),
    "first equal (an empty row)": _with(rows=[(0, 1, 0), (0, 2, 2), (3, 0, 2)]),
    "first descending": _with(rows=[(0, 1, 0), (0, 2, 3), (3, 0, 2)]),
    "first at entries": _with(rows=[(0, 1, 0), (0, 2, 2), (3, 0, 5)]),
    "first past entries": _with(rows=[(0, 1, 0), (0, 2, 2), (3, 0, 2**40)]),
    "entries without a row": lhsnap.pack(2, [], [(0, 1)]),
    "bin == bins": _with(entries=[(0, 5), (9, 1), (4, 2), (1, 1), (156, 3)]),
    "bin 2^32 - 1": _with(entries=[(0, 5), (9, 1), (4, 2), (1, 1), (U32, 3)]),
    "bins equal in a row": _with(entries=[(9, 5), (9, 1), (4, 2), (1, 1), (155, 3)]),
    "bins descending in a row": _with(entries=[(0, 5), (9, 1), (4, 2), (155, 1), (1, 3)]),
    "zero count": _with(entries=[(0, 5), (9, 0), (4, 2), (1, 1), (155, 3)], links=11),
    "links too small": _with(links=11),
    "links too large": _with(links=13),
}


def test_validate_accepts_the_hand_made_blob_the_bad_ones_are_made_from():
    assert validate(_with()) == _abi.ZK_OK
    # descending bins across a row edge are fine: order holds inside a row only
    assert validate(_with(entries=[(8, 5), (9, 1), (4, 2), (1, 1), (155, 3)])) == _abi.ZK_OK


@pytest.mark.parametrize("rule", sorted(BAD))
def test_validate_rejects(rule):
    assert validate(BAD[rule]) == _abi.ZK_ERR_INVALID_ARG
    with pytest.raises(ZkError) as e:
        LinkHistogramSnapshot(BAD[rule])
    assert e.value.status == _abi.ZK_ERR_INVALID_ARG


def test_validate_rejects_every_truncation():
    blob = _with()
    assert len(blob) == 64 + 3 * 16 + 5 * 8
    for n in range(len(blob)):
        assert validate(blob[:n]) == _abi.ZK_ERR_INVALID_ARG, n
    assert _abi.lib().zk_lh_snapshot_validate(None, 64) == _abi.ZK_ERR_INVALID_ARG


# ---- plus -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 4, 7])
def test_plus_is_the_encoding_of_the_sum(m):
    S = 5
    a, b = sparse(1, S, m, cells=9), sparse(2, S, m, cells=9)
    b[np.flatnonzero(a.any(axis=1))[0]] += 3  # a shared row with shared and unshared bins
    A, B = LinkHistogramSnapshot(lhsnap.encode(a, S, m, 2)), LinkHistogramSnapshot(lhsnap.encode(b, S, m, 5))
    want = lhsnap.encode(a + b, S, m, 7)
    assert A.plus(B).blob == want and B.plus(A).blob == want
    zero = LinkHistogramSnapshot(lhsnap.encode(np.zeros_like(a), S, m))
    assert A.plus(zero).blob == A.blob == zero.plus(A).blob
    assert (A.links, A.dropped, A.m, A.bins, len(A)) == (int(a.sum()), 2, m, lhsnap.nbins(m), int(a.any(axis=1).sum()))


def test_plus_refuses_another_sub_bits():
    a = LinkHistogramSnapshot(lhsnap.encode(sparse(1, 3, 2), 3, 2))
    b = LinkHistogramSnapshot(lhsnap.encode(sparse(1, 3, 4), 3, 4))
    with pytest.raises(ZkError) as e:
        a.plus(b)
    assert e.value.status == _abi.ZK_ERR_INVALID_ARG


def test_plus_at_the_counter_bound():
    one = LinkHistogramSnapshot(lhsnap.pack(4, [(1, 2, 0)], [(7, 1)]))
    below = LinkHistogramSnapshot(lhsnap.pack(4, [(1, 2, 0)], [(3, 5), (7, U32 - 1)]))
    full = LinkHistogramSnapshot(lhsnap.pack(4, [(1, 2, 0)], [(3, 5), (7, U32)]))
    assert below.plus(one).blob == full.blob == one.plus(below).blob  # exactly 2^32 - 1 answers
    for x, y in ((full, one), (one, full), (full, full)):
        with pytest.raises(ZkError) as e:
            x.plus(y)
        assert e.value.status == _abi.ZK_ERR_CAPACITY
    # `links` is a u64: it passes 2^32 when the counters themselves do not
    other = LinkHistogramSnapshot(lhsnap.pack(4, [(1, 2, 0)], [(8, U32)]))
    assert full.plus(other).links == 2 * U32 + 5


def test_two_phase_outputs():
    L = _abi.lib()
    a, b = lhsnap.encode(sparse(1, 3, 2), 3, 2), lhsnap.encode(sparse(2, 3, 2), 3, 2)
    n = C.c_uint64()
    assert L.zk_lh_snapshot_plus(a, len(a), b, len(b), None, 0, C.byref(n)) == _abi.ZK_OK
    small = (C.c_uint8 * n.value)(*([0xCD] * n.value))
    assert L.zk_lh_snapshot_plus(a, len(a), b, len(b), small, n.value - 1, C.byref(n)) == _abi.ZK_ERR_CAPACITY
    assert bytes(small) == b"\xcd" * n.value  # nothing written


# ---- remap ------------------------------------------------------------------------------------------
def test_remap():
    S, m = 5, 4
    d = sparse(4, S, m, cells=11)
    snap = LinkHistogramSnapshot(lhsnap.encode(d, S, m, 3))
    perm = np.array([3, 0, 4, 1, 2])
    want = np.zeros_like(d)
    for c in np.flatnonzero(d.any(axis=1)).tolist():
        want[perm[c // S] * S + perm[c % S]] = d[c]
    got = snap.remap(perm)
    assert got.blob == lhsnap.encode(want, S, m, 3)
    assert got.remap(np.argsort(perm)).blob == snap.blob
    # into a larger id space: the rows carry (parent, child), not a cell index
    wide = snap.remap(np.arange(S) + 100)
    assert np.array_equal(wide.rows["parent"], snap.rows["parent"] + 100) and np.array_equal(wide.entries, snap.entries)
    with pytest.raises(ZkError) as e:
        snap.remap(perm[: int(max(snap.rows["parent"].max(), snap.rows["child"].max()))])  # an id >= n_map
    assert e.value.status == _abi.ZK_ERR_SERVICE_RANGE
    two = LinkHistogramSnapshot(lhsnap.pack(4, [(0, 2, 0), (1, 2, 1)], [(5, 1), (6, 1)]))
    with pytest.raises(ZkError) as e:
        two.remap([7, 7, 2])  # not injective: both rows land on (7, 2)
    assert e.value.status == _abi.ZK_ERR_INVALID_ARG
    assert two.remap([7, 7, 2][::-1] + [9]).blob == lhsnap.pack(4, [(2, 7, 0), (7, 7, 1)], [(5, 1), (6, 1)])


# ---- quantiles --------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 4, 7])
def test_quantiles_follow_the_nearest_rank_rule(m):
    S, bins = 4, lhsnap.nbins(m)
    qs = (0.0, 0.25, 0.5, 0.99, 1.0)
    d = sparse(m, S, m, cells=8, per_row=9, high=50)
    free = np.flatnonzero(~d.any(axis=1))
    d[free[0], 17] = 1                      # N = 1
    d[free[1], 0] = 1000                    # all mass in bin 0
    d[free[2], bins - 1] = 77               # all mass in the last bin
    d[free[3], [0, bins - 1]] = [1, 1]      # q = 0 and q = 1 at the two ends
    d[free[4], [3, 9]] = [U32, U32]         # N above 2^32
    snap = LinkHistogramSnapshot(lhsnap.encode(d, S, m))
    lo, hi, cnt = snap.quantiles(qs)
    cells = np.flatnonzero(d.any(axis=1))
    assert len(snap) == len(cells) == 13
    assert np.array_equal(snap.rows["parent"] * S + snap.rows["child"], cells)
    for r, c in enumerate(cells.tolist()):
        cum = np.cumsum(d[c].astype(np.int64))
        n = int(cum[-1])
        assert cnt[r] == n
        for k, q in enumerate(qs):
            want = bin_bounds(int(np.searchsorted(cum, nearest_rank(q, n), side="left")), m)
            assert (lo[r, k], hi[r, k]) == want, (c, q)
    r = int(np.searchsorted(cells, free[3]))
    assert (lo[r, 0], hi[r, 0]) == (0, 0) and (lo[r, -1], hi[r, -1]) == bin_bounds(bins - 1, m)
    assert hi[r, -1] == 2**40 - 1
    with pytest.raises(ZkError):
        snap.quantiles((1.5,))
    lo0, hi0, cnt0 = snap.quantiles(())
    assert lo0.shape == (13, 0) and np.array_equal(cnt0, cnt)


# ---- the store --------------------------------------------------------------------------------------
HS, HM = 4, 4  # services and sub_bits of the attached histograms
NAMES = [f"s{i}" for i in range(16)]


class StoreCase:
    """A GpuAggregates in one mode. Record i carries the single link (s_i, s_i), so the links
    getDependencies returns name the records it read; records with an attachment carry the snapshot of
    their own random histogram."""

    def __init__(self, mode, now=10 * DAY_US):
        self.agg = GpuAggregates(mode, services=Dictionary(NAMES), clock=lambda: now)
        self.dense = {}

    def put(self, i, start, end, hist=True):
        deps = Dependencies(start, end, (DependencyLink(Service(NAMES[i]), Service(NAMES[i]), Moments.of(i)),))
        if hist:
            self.dense[i] = sparse(100 + i, HS, HM, cells=5)
            self.dense[i][5, 20] += 1  # a row and a bin every attachment shares
            self.agg.storeDependencies(deps, link_hist=lhsnap.encode(self.dense[i], HS, HM, dropped=i))
        else:
            self.dense.pop(i, None)
            self.agg.storeDependencies(deps)

    def check(self, start, end, want_ids):
        deps = self.agg.getDependencies(start, end)
        ids = sorted(int(l.parent.name[1:]) for l in deps.links)
        assert ids == sorted(want_ids)
        snap, records, with_hist = self.agg.getLinkHistogram(start, end)
        carried = [i for i in ids if i in self.dense]
        assert (records, with_hist) == (len(ids), len(carried))
        total = np.zeros((HS * HS, lhsnap.nbins(HM)), np.uint32)
        for i in carried:
            total += self.dense[i]
        assert snap.blob == lhsnap.encode(total, HS, HM, dropped=sum(carried))
        want = LinkHistogramSnapshot(lhsnap.encode(np.zeros_like(total), HS, HM))
        for i in carried:  # and it is the plus of the attachments
            want = want.plus(LinkHistogramSnapshot(lhsnap.encode(self.dense[i], HS, HM, dropped=i)))
        assert snap.blob == want.blob
        # getLinkDurations answers from the same sum
        lo, hi, cnt = snap.quantiles((0.5, 0.99))
        got = self.agg.getLinkDurations(start, end)
        assert [(x.parent, x.child, x.count) for x in got] == [
            (NAMES[int(r["parent"])], NAMES[int(r["child"])], int(cnt[k])) for k, r in enumerate(snap.rows)]
        assert [x.quantiles for x in got] == [{0.5: (lo[k, 0], hi[k, 0]), 0.99: (lo[k, 1], hi[k, 1])}
                                              for k in range(len(snap))]
        return snap


def test_store_anorm_containment():
    h = 3_600_000_000
    s = StoreCase("anorm")
    s.put(0, 1 * h, 2 * h)
    s.put(1, 2 * h, 3 * h, hist=False)
    s.put(2, 3 * h, 4 * h)
    s.put(3, 1 * h, 4 * h)            # spans the others: contained only in the widest window
    s.put(4, 10 * DAY_US - h, 10 * DAY_US)  # inside the default window (now - 1 day, now)
    s.put(5, 10 * DAY_US - h, 10 * DAY_US + 1, hist=True)  # ends after now
    s.check(0, 5 * h, [0, 1, 2, 3])
    s.check(1 * h, 3 * h, [0, 1])      # bounds inclusive; 3 starts inside and ends outside
    s.check(1 * h + 1, 4 * h, [1, 2])  # 0 and 3 start before the window
    s.check(2 * h, 3 * h, [1])         # a record without an attachment only: the empty snapshot
    s.check(5 * h, 6 * h, [])          # an empty window
    s.check(4 * h, 1 * h, [])          # reversed bounds contain nothing
    s.check(None, None, [4])
    s.check(None, 10 * DAY_US + 1, [4, 5])
    empty, records, with_hist = s.agg.getLinkHistogram(5 * h, 6 * h)
    assert (len(empty.blob), len(empty), records, with_hist) == (64, 0, 0, 0)


def test_store_cassandra_clobber():
    h = 3_600_000_000
    s = StoreCase("cassandra")
    s.put(0, 0 * DAY_US + h, 1 * DAY_US)
    s.put(1, 2 * DAY_US + h, 2 * DAY_US + 2 * h)
    s.put(2, 2 * DAY_US + 5 * h, 2 * DAY_US + 6 * h, hist=False)  # the same day row: record 1 and its snapshot are gone
    s.check(None, None, [0, 2])
    s.check(0, 5 * DAY_US, [0, 2])     # the bounds compare with the column name 0, not with a time
    s.put(3, 2 * DAY_US + 7 * h, 2 * DAY_US + 8 * h)              # ... and an attachment replaces none
    s.put(4, 3 * DAY_US, 3 * DAY_US + h)
    s.check(None, None, [0, 3, 4])
    s.check(7 * DAY_US, 8 * DAY_US, [0, 3, 4])
    s.check(-1, None, [])              # a negative bound drops column 0 of every row
    s.check(None, -5, [])
    assert s.agg.count() == 3


def test_store_hbase_replace_and_reversed_scan():
    ms = 1000
    s = StoreCase("hbase")
    s.put(0, 100 * ms, 200 * ms)
    s.put(1, 300 * ms, 400 * ms)
    s.put(2, 300 * ms + 999, 500 * ms, hist=False)  # the same ms key: replaces record 1 and its snapshot
    s.put(3, 500 * ms, 600 * ms)
    s.put(4, 700 * ms, 800 * ms, hist=False)
    s.put(5, 700 * ms + 1, 900 * ms)                # ... and an attachment replaces none
    assert s.agg.count() == 4
    s.check(None, None, [0, 2, 3, 5])
    # the scan runs from the start bound DOWN to the end bound: end ms < record start ms <= start ms
    s.check(700 * ms, 100 * ms, [2, 3, 5])
    s.check(500 * ms, 300 * ms, [3])
    s.check(699 * ms, 299 * ms, [2, 3])
    s.check(100 * ms, 700 * ms, [])     # start < end scans nothing
    s.check(300 * ms, 300 * ms, [2])    # a get-scan of one key: the record without an attachment
    s.check(600 * ms, None, [0, 2, 3])
    s.check(None, 300 * ms, [3, 5])
    s.check(99 * ms, 0, [])             # an empty window


def test_store_put_validates_and_get_refuses_mixed_sub_bits():
    L = _abi.lib()
    agg = GpuAggregates("anorm", services=Dictionary(NAMES), clock=lambda: 0)
    good = lhsnap.encode(sparse(1, HS, 4), HS, 4)
    for bad in (BAD["links too small"], good[:-1], b""):
        assert L.zk_store_put_dependencies_hist(agg._h, 0, 1, None, 0, bad, len(bad)) == _abi.ZK_ERR_INVALID_ARG
    assert agg.count() == 0
    assert L.zk_store_put_dependencies_hist(agg._h, 0, 1, None, 0, None, 0) == _abi.ZK_OK  # no attachment
    assert agg.getLinkHistogram(0, 1)[1:] == (1, 0)
    agg.storeDependencies(Dependencies(0, 1, ()), link_hist=good)
    agg.storeDependencies(Dependencies(0, 1, ()), link_hist=LinkHistogramSnapshot(good))
    snap, records, with_hist = agg.getLinkHistogram(0, 1)
    assert (records, with_hist) == (3, 2) and snap.blob == LinkHistogramSnapshot(good).plus(LinkHistogramSnapshot(good)).blob
    n = C.c_uint64()
    s0, e0 = C.c_int64(0), C.c_int64(1)
    out = (C.c_uint8 * len(snap.blob))()
    assert L.zk_store_get_link_hist(agg._h, C.byref(s0), C.byref(e0), 0, out, len(snap.blob) - 1, C.byref(n), None,
                                    None) == _abi.ZK_ERR_CAPACITY
    assert n.value == len(snap.blob) and not any(out)
    agg.storeDependencies(Dependencies(0, 1, ()), link_hist=lhsnap.encode(sparse(1, HS, 2), HS, 2))
    with pytest.raises(ZkError) as e:
        agg.getLinkHistogram(0, 1)
    assert e.value.status == _abi.ZK_ERR_INVALID_ARG
    assert len(agg.getDependencies(0, 1).links) == 0  # the dependencies themselves are unaffected


def test_store_remaps_a_jobs_snapshot_like_its_links():
    """A LinkList record keeps the job's service ids; the store's dictionary has other ids for the same
    names. storeDependencies moves the snapshot's rows to the store's ids exactly as it moves the links."""
    from zipkin_amd.aggregates import LinkList
    from zipkin_amd.context import LinkTable

    S = 3
    job_names = ["web", "db", "cache"]
    agg = GpuAggregates("anorm", services=Dictionary(["cache", "x", "web", "db"]), clock=lambda: 0)
    z = np.zeros(S * S)
    present = np.zeros(S * S, np.uint8)
    m0 = np.zeros(S * S, np.uint64)
    for c in (0 * S + 1, 1 * S + 2):  # web -> db, db -> cache
        present[c], m0[c] = 1, 4
    table = LinkTable(S, m0, z + 5.0, z.copy(), z.copy(), z.copy(), present)
    d = np.zeros((S * S, lhsnap.nbins(4)), np.uint32)
    d[1, [3, 40]] = [1, 3]
    d[5, 100] = 4
    agg.storeDependencies(Dependencies(0, 1, LinkList(table, job_names)), link_hist=lhsnap.encode(d, S, 4))
    got = agg.getLinkDurations(0, 1, qs=(1.0,))
    assert [(x.parent, x.child, x.count) for x in got] == [("web", "db", 4), ("db", "cache", 4)]
    assert {(l.parent.name, l.child.name): l.duration_moments.m0 for l in agg.getDependencies(0, 1).links} == \
        {("web", "db"): 4, ("db", "cache"): 4}
    assert got[0].quantiles == {1.0: bin_bounds(40, 4)} and got[1].quantiles == {1.0: bin_bounds(100, 4)}


# ---- sanitizers -------------------------------------------------------------------------------------
def test_snapshot_functions_are_sanitizer_clean():
    """tools/sanitize/fuzz_lh_snapshot: zk_lh_snapshot.cpp under ASan + UBSan in a program of its own,
    fed seeded mutations of valid snapshots in heap blocks of exactly their length."""
    if not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    subprocess.run(["make", "-s", "-C", str(ROOT / "tools" / "sanitize"), "lhsnap"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(ROOT / "build" / "sanitize" / "fuzz_lh_snapshot"), "30000", "7"], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "sanitized run ok" in r.stdout
