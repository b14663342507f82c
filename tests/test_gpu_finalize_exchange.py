"""k_finalize, k_table_pack and k_table_unpack on crafted sums, through the public exchange path.

zk_deps_partial hands out the exchange buffer that ranks all-reduce; whatever the caller leaves in it
is, to zk_deps_note_merged, the all-reduce's result. Writing tests/exactref.py's case list there
(one multiset per cell of a 64 x 64 table) puts sums in front of k_table_unpack and k_finalize that
no real batch of test size can produce: counts up to 2^32 - 1, durations up to 2^40 - 1, numerators
up to 284 bits, exact ties, the mantissa carry, negative numerators and div_round's right-shift
path. The caller-owned table is the other door: the limb state after 2^32 - 1 worst-case flushes is
copied into it and packed by zk_deps_partial. Every comparison is exact equality with Python
integers and Fractions."""
import random

import numpy as np
import pytest

from tests import exactref
from tests.exactref import DMAX, NMAX, finalize_cases, power_sums
from tests.test_gpu_sharded import Shard
from zipkin_amd import _abi, table
from zipkin_amd.shards import device_view

pytestmark = pytest.mark.gpu


def exchange_view(sh):
    """The shard's exchange buffer (zk_deps_partial) as an int64 device tensor, the ctx stream idle."""
    import torch

    ptr, nbytes = sh.ctx.partial()
    assert nbytes == _abi.xchg_words(sh.ctx.num_services) * 8
    sh.ctx.sync()
    return device_view(ptr, nbytes, torch.int64)


def put(dst, host):
    import torch

    dst.copy_(torch.from_numpy(np.ascontiguousarray(host)).to(dst.device))
    torch.cuda.synchronize()


def test_finalize_of_crafted_sums_through_the_exchange_buffer(gpu):
    S = 64
    cells = {(i // S, i % S): ms for i, (_, ms) in enumerate(finalize_cases())}
    assert len(cells) == S * S
    want = {k: power_sums(ms) for k, ms in cells.items()}
    x = table.encode_exchange(want, S)
    sh = Shard(S)
    try:
        sh.ctx.reset()
        view = exchange_view(sh)
        assert not view.cpu().numpy().any()
        put(view, x)
        sh.ctx.note_merged(NMAX)
        got = sh.ctx.finalize()
        st = sh.ctx.stats()
        sh.ctx.sync()
        acc = sh.table.cpu().numpy()
    finally:
        sh.close()
    assert np.array_equal(acc, table.unpack(x, S))
    assert table.decode(acc, S) == want
    exactref.assert_moments(got, cells, S)
    assert st["duration_range"] == 0 and st["joined_links"] == 0


def test_pack_of_the_worst_limb_state(gpu):
    """The accumulator after 2^32 - 1 flushes of one link of 2^40 - 1 each (every limb below a sum's top
    one near 2^64) and a few case cells, written into the caller-owned table: zk_deps_partial packs
    them into the exchange form exactly, note_merged unpacks them, finalize rounds them."""
    S = 5
    limbs, worst = exactref.worst_flush_cell()
    cases = dict(finalize_cases())
    cells = {(0, 0): cases["largest_numerators"], (1, 3): cases["tie_odd_m1"], (2, 2): cases["left_skewed"],
             (4, 3): cases["carry_m1"], (4, 4): [(DMAX, NMAX)]}
    want = {k: power_sums(ms) for k, ms in cells.items()}
    assert want[(4, 4)] == worst
    acc = table.encode({k: v for k, v in want.items() if k != (4, 4)}, S).view(np.uint64)
    acc[24 * table.LIMBS: 25 * table.LIMBS] = np.array(limbs, np.uint64)
    acc = acc.view(np.int64)
    assert table.decode(acc, S) == want
    sh = Shard(S)
    try:
        sh.ctx.reset()
        sh.ctx.sync()
        put(sh.table, acc)
        x = exchange_view(sh).cpu().numpy()
        assert np.array_equal(x, table.pack(acc, S))
        assert table.decode_exchange(x, S) == want
        assert int(x.view(np.uint64).max()) <= (1 << 56) - 1  # room for 256 ranks in every limb
        sh.ctx.note_merged(NMAX)
        got = sh.ctx.finalize()
        sh.ctx.sync()
        back = sh.table.cpu().numpy()
    finally:
        sh.close()
    assert np.array_equal(back, table.unpack(x, S)) and table.decode(back, S) == want
    exactref.assert_moments(got, cells, S)


def test_256_rank_sum_of_the_largest_cell(gpu):
    """256 ranks each hold 1/256 of the largest cell ((2^32 - 1) // 256 links of 2^40 - 1) and a share
    of a second, random cell; the SUM of their exchange buffers (an int64 add, what the all-reduce
    computes) must not carry out of any limb: the table decodes to the exact union."""
    import torch

    S, ranks = 3, 256
    share_n = NMAX // ranks
    rng = random.Random(256)
    shares = [[(rng.randrange(1 << 40), rng.randrange(1, 1 << 16)) for _ in range(rng.randint(1, 3))]
              for _ in range(ranks)]
    bufs = np.stack([table.encode_exchange({(2, 2): power_sums([(DMAX, share_n)]), (0, 1): power_sums(ms)}, S)
                     for ms in shares])
    cells = {(2, 2): [(DMAX, ranks * share_n)], (0, 1): [pair for ms in shares for pair in ms]}
    want = {k: power_sums(ms) for k, ms in cells.items()}
    sh = Shard(S)
    try:
        sh.ctx.reset()
        view = exchange_view(sh)
        total = torch.from_numpy(bufs).to(view.device).sum(0)  # the all-reduce's SUM
        view.copy_(total)
        torch.cuda.synchronize()
        sh.ctx.note_merged(ranks * share_n)
        got = sh.ctx.finalize()
        sh.ctx.sync()
        acc = sh.table.cpu().numpy()
    finally:
        sh.close()
    assert table.decode_exchange(total.cpu().numpy(), S) == want
    assert table.decode(acc, S) == want
    exactref.assert_moments(got, cells, S)
