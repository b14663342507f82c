"""The compact word of the bucket-ordered links (zipkin_amd/csrc/zk_internal.h): between
K2 k_link_scatter and its readers a link is 4 bytes -- (cell_local << 21) | d when d < 2^21, else an
escape holding the link's slot in the K1 lists, where the reader finds the full (cell << 40) | d.

Placed by star traces as in tests/test_gpu_exact_bounds.py and checked against tests/exactref.py
(Python integers): the format's edges (both sides of 2^21, the last cell of a bucket, the word
0x7FFFFFFF), escapes over K2's chunk and carry boundaries and in every list position, the S = 500
geometry of the benchmark, every producer of the lists an escape points into (K1, the group join and
its fallback, a held trace's extended list, a second join that overwrites the lists), and the link
histogram's reader against the host reference of tests/test_gpu_link_hist.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle
from oracle.realtime import joined_links
from tests.exactref import DMAX
from tests.test_gpu_exact_bounds import (mixed, random_durations, run_and_check, star_batch, traces_of, unclustered_batch,
                                         wide, with_over_range)
from tests.test_gpu_link_hist import expected_hist
from tests.test_gpu_parity import assert_parity
from zipkin_amd import DepsContext, SpanColumns, _abi
from zipkin_amd.realtime import LinkHistogram

pytestmark = pytest.mark.gpu

SHORT_MAX = (1 << 21) - 1
FORMAT_EDGES = (0, 1, SHORT_MAX, 1 << 21, (1 << 21) + 1, 1 << 32, DMAX)
K2_CHUNK = 8192  # links of one k_link_scatter chunk (kK2U * kK2WG)


def pair(cell, S):
    return cell // S, cell % S


def reduce_geometry(n):
    """(K1 lists, records per list, K2 lists per workgroup) of a clustered batch of n records."""
    import torch

    f = _abi.lib().zk_internal_reduce_geometry
    f.restype = None
    f.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lists, lpw, compact = C.c_uint32(), C.c_uint32(), C.c_uint32()
    per, stride = C.c_uint64(), C.c_uint64()
    f(n, torch.cuda.get_device_properties(0).multi_processor_count, C.byref(lists), C.byref(per), C.byref(stride),
      C.byref(lpw), C.byref(compact))
    return lists.value, per.value, lpw.value


# ---- 1. the format's edges ----------------------------------------------------------------------
@pytest.mark.parametrize("over_range", [0, 1])
@pytest.mark.parametrize("S,last_local", [(23, 511), (725, 1023)])
def test_format_edges(gpu, S, last_local, over_range):
    """S = 23: k_bucket_lds_reduce_wide<9>, 2 buckets, atomic flush; S = 725: k_bucket_reduce<10>. Every
    edge duration in an ordinary cell, in the last cell of bucket 0 (cell_local 511 / 1023: at S = 725
    (1023 << 21) | (2^21 - 1) = 0x7FFFFFFF is a short word, neither escape nor pad) and in the last cell
    of the table; over_range: a child of exactly 2^40 us beside them, counted and dropped."""
    reps = list(FORMAT_EDGES) * 5
    cells = {(0, 1): reps, pair(last_local, S): reps + [SHORT_MAX] * 3, (S - 1, S - 1): reps + [DMAX, 1 << 21]}
    assert (last_local << 21 | SHORT_MAX) < 1 << 31 and ((last_local << 21 | SHORT_MAX) == 0x7FFFFFFF) == (S == 725)
    rng = np.random.default_rng(S)
    tr = traces_of(cells, rng, per_trace=40)
    if over_range:
        tr = with_over_range(*tr, at_trace=1)
    run_and_check([star_batch(*tr)], S, cells, over_range=over_range)


# ---- 2. carries and chunk boundaries with escapes -------------------------------------------------
_CHUNKED = {}


def chunked_batch(layout):
    """S = 23 (buckets: cells [0, 512) and [512, 529)). The smallest clustered batch (in steps of 2^16
    records) of whose K1 lists a K2 workgroup walks more than a chunk's worth as one stream, so its
    per-bucket carries cross a chunk boundary; K1 writes many lists, so long links lie in lists other
    than 0 and at the ends of lists.
    layout 'split': bucket 0 holds only long links, bucket 1 only short ones; 'alternate': long and
    short links alternate in every cell of both buckets."""
    if layout not in _CHUNKED:
        S = 23
        n = 1 << 16
        while True:
            lists, per, lpw = reduce_geometry(n)
            if lpw * per >= K2_CHUNK + 2048:
                break
            n += 1 << 16
        assert lists >= 2
        rng = np.random.default_rng(len(layout))
        links = n - n // 200  # (one root per trace of <= 255 children; the rest of n is slack)
        longs = np.asarray([1 << 21, (1 << 21) + 1, 1 << 32, DMAX, DMAX - 1] + wide(rng, 20), np.int64)
        shorts = np.asarray([0, 1, SHORT_MAX, SHORT_MAX - 1] + random_durations(rng, 20, classes=(21,)), np.int64)
        b0 = [(0, 1), (3, 4), pair(511, S)]
        b1 = [pair(512, S), (22, 22)]
        sizes = {}
        for k in b0:
            sizes[k] = links * 3 // 4 // len(b0) + len(sizes)
        for k in b1:
            sizes[k] = links // 4 // len(b1) + 2 * len(sizes) + 1
        for b in (b0, b1):  # no bucket ends on a line boundary (16 words)
            if sum(sizes[k] for k in b) % 16 == 0:
                sizes[b[0]] += 1
        cells = {}
        for k, m in sizes.items():
            if layout == "split":
                pool = longs if k in b0 else shorts
                cells[k] = pool[rng.integers(0, len(pool), m)]
            else:
                d = np.empty(m, np.int64)
                d[0::2] = longs[rng.integers(0, len(longs), len(d[0::2]))]
                d[1::2] = shorts[rng.integers(0, len(shorts), len(d[1::2]))]
                cells[k] = d
        for b in (b0, b1):
            assert sum(len(cells[k]) for k in b) % 16
        cols = star_batch(*traces_of(cells, rng))
        lists, per, lpw = reduce_geometry(len(cols))
        assert lists >= 2 and lpw * per > K2_CHUNK and len(cols) > lpw * per
        _CHUNKED[layout] = (cols, cells)
    return _CHUNKED[layout]


@pytest.mark.parametrize("layout", ["split", "alternate"])
def test_escapes_across_chunks_and_carries(gpu, layout):
    cols, cells = chunked_batch(layout)
    run_and_check([cols], 23, cells)


# ---- 3. the benchmark's geometry -----------------------------------------------------------------
def s500_cells(rng):
    """489 buckets (the last one partial: cells [249856, 250000)), splits == 1: owner stores."""
    S = 500
    return {(0, 0): mixed(rng, 900), pair(511, S): mixed(rng, 700), pair(512, S): random_durations(rng, 800, classes=(21,)),
            (250, 250): wide(rng, 600), (250, 251): mixed(rng, 500), pair(488 * 512 - 1, S): mixed(rng, 300),
            (499, 499): [1 << 21]}


def test_s500_geometry(gpu):
    S = 500
    rng = np.random.default_rng(500)
    cells = s500_cells(rng)
    assert (S * S - 1) >> 9 == 488 and (S * S) % 512
    run_and_check([star_batch(*traces_of(cells, rng))], S, cells)


# ---- 4. the other producers of the lists ---------------------------------------------------------
def test_group_join_and_its_fallback(gpu):
    """An unclustered batch just over 2^18 records: k_group_join writes the lists an escape points
    into, K1 appends the fallback's links to them."""
    cols, cells = unclustered_batch(0)
    assert any((np.asarray(v) > SHORT_MAX).any() for v in cells.values())
    assert any((np.asarray(v) <= SHORT_MAX).any() for v in cells.values())
    run_and_check([cols], 23, cells, ctx_kw={"trace_pass": False}, acc_kw={"clustered": False, "verify": False})


def test_held_trace_extends_list_zero(gpu):
    """ZK_BATCH_CONTINUES: the first batch ends inside a trace, whose links the next batch's K1 appends
    to list 0 (every list's stride is then a tile longer): escapes into the appended part."""
    rng = np.random.default_rng(41)
    cells = {(0, 1): mixed(rng, 90), (22, 22): mixed(rng, 90), (22, 0): wide(rng, 30)}
    held = {(4, 1): [5, 1 << 21, DMAX, 1 << 32, SHORT_MAX], (4, 7): [DMAX, DMAX - 1, 0]}
    a = traces_of(cells, rng, per_trace=50)
    h = traces_of(held, rng)
    assert len(h[0]) == 1
    k = len(a[0]) // 2
    na = int(np.sum(a[1][:k]))
    b1 = star_batch(a[0][:k] + h[0], a[1][:k] + h[1], np.concatenate([a[2][:na], h[2]]), np.concatenate([a[3][:na], h[3]]))
    b2 = star_batch(a[0][k:], a[1][k:], a[2][na:], a[3][na:], tid0=10_000)
    edge = len(b1) - 5  # the held trace's root and three of its children stay on the near side
    assert b1.trace_id[edge - 4] == b1.trace_id[-1] and b1.trace_id[edge - 5] != b1.trace_id[-1]
    batches = [(b1.take(slice(0, edge)), {"clustered": True, "continues": True}),
               (SpanColumns.concat([b1.take(slice(edge, len(b1))), b2]), {"clustered": True})]
    run_and_check(batches, 23, {**cells, **held})


def test_second_join_overwrites_the_lists(gpu):
    """Two accumulates without a reset: the second join overwrites the lists the first batch's escapes
    pointed into, after the first reduce has read them (one stream)."""
    rng = np.random.default_rng(42)
    first = {(0, 1): mixed(rng, 400), (22, 22): wide(rng, 300), (5, 5): [DMAX] * 77}
    second = {(0, 1): random_durations(rng, 500, classes=(21,)), (22, 22): mixed(rng, 200), (7, 8): wide(rng, 111)}
    b1 = star_batch(*traces_of(first, rng, per_trace=60))
    b2 = star_batch(*traces_of(second, rng, per_trace=60), tid0=50_000)
    both = {k: list(first.get(k, [])) + list(second.get(k, [])) for k in {**first, **second}}
    run_and_check([b1, b2], 23, both)


# ---- 5. the link histogram's reader ----------------------------------------------------------------
def lh_cells(S, rng):
    last = 511 if S == 23 else 488 * 512 - 1
    return {(0, 1): mixed(rng, 300), pair(last, S): mixed(rng, 200) + [SHORT_MAX] * 5, pair(last + 1, S): wide(rng, 150),
            (S - 1, S - 1): random_durations(rng, 250)}


@pytest.mark.parametrize("S,m", [(23, 0), (23, 7), (500, 0), (500, 2)])
def test_bound_link_histogram(gpu, S, m):
    """m = 0: the default sub_bits (4: 8 tiles per 512-cell bucket); m = 7 / 2: 64 / 4 tiles per bucket.
    The rows of the cells in use against the join rows of the host oracle, and every cell's count
    against the table's m0 (a count in a wrong row would show there)."""
    rng = np.random.default_rng(1000 * S + m)
    cells = lh_cells(S, rng)
    cols = star_batch(*traces_of(cells, rng, per_trace=60))
    links = joined_links(cols, S)
    with DepsContext(S) as ctx, LinkHistogram(S, sub_bits=m) as lh:
        lh.bind(ctx)
        ctx.accumulate(cols, clustered=True, verify=True)
        got = ctx.finalize()
        assert_parity(got, ctx.stats(), oracle.aggregate(cols, S))
        assert np.array_equal(lh.quantiles_all(())[2], got.m0)
        p, c, d, _ = links
        for (pp, cc), v in cells.items():
            sel = (p == pp) & (c == cc)
            assert sel.sum() == len(v)
            one = (np.zeros(sel.sum(), p.dtype), np.zeros(sel.sum(), c.dtype), d[sel], None)
            want = expected_hist(one, 1, lh.m)
            assert np.array_equal(lh.read(pp * S + cc, 1), want), (pp, cc)
        assert lh.dropped() == 0
