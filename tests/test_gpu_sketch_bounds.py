"""The two per-service sketches at the bounds of their domain: the crafted cases of
tests/sketchref.py through zk_kv.hip and zk_rt.hip, every answer equal -- exactly -- to the independent
integer reference there (tests/test_sketch_cases.py holds that reference against oracle/ on the CPU
and requires the cases to reach every rare branch `classify_kv` / `classify_rt` name).

State near 2^32 is written straight into the library's buffers through the zero-copy views of
zipkin_amd.shards (kv_views, rt_views), as test_gpu_finalize_exchange.py does with the exchange
buffer; everything else goes through the public calls. Shapes are the smallest that reach the branch."""
import numpy as np
import pytest

from oracle.realtime import tdigest as oracle_tdigest
from oracle.realtime import tdigest_quantile as oracle_tdigest_quantile
from tests import sketchref as R
from tests.test_sketch_cases import single_span_columns
from zipkin_amd import ZkError, _abi
from zipkin_amd import shards as sh

pytestmark = pytest.mark.gpu


def _i64(values):
    return np.array(values, np.uint64).view(np.int64)


def _i32(values):
    return np.array(values, np.uint64).astype(np.uint32).view(np.int32)


# ------------------------------------------------------------------------------ count-min + top-K
def _kv_open(cfg):
    from zipkin_amd.kv import KvSketch

    kv = KvSketch(cfg["S"], width=cfg["width"], depth=cfg["depth"], candidates=cfg["candidates"], seed=cfg["seed"])
    assert (kv.width, kv.depth, kv.candidates) == (cfg["width"], cfg["depth"], cfg["candidates"])
    return kv


def _kv_apply(kv, ref, op):
    """One op of a case on the device; `ref` has already taken it."""
    import torch

    S, C = kv.num_services, kv.candidates
    if op[0] == "acc":
        kv.accumulate(op[1], op[2])
        return
    torch.cuda.synchronize()
    counters, totals, ckeys, cest = sh.kv_views(kv)
    if op[0] == "state":
        want = np.stack([ref.counters(s) for s in range(S)])
        counters.copy_(torch.from_numpy(_i32(want.reshape(-1))))
        totals.copy_(torch.from_numpy(_i64(ref.totals)))
        for s, lst in op[2].items():
            pad = list(lst) + [(0, 0)] * (C - len(lst))
            ckeys[s].copy_(torch.from_numpy(_i64([k for k, _ in pad])))
            cest[s].copy_(torch.from_numpy(_i32([e for _, e in pad])))
    elif op[0] == "total":
        totals[op[1]] = int(_i64([op[2]])[0])
    elif op[0] == "merge":
        L = len(op[1])
        gk = np.zeros((max(L, 1), S, C), np.uint64)
        ge = np.zeros((max(L, 1), S, C), np.uint64)
        for l, lists in enumerate(op[1]):
            for s, lst in lists.items():
                assert len(lst) <= C
                for i, (k, e) in enumerate(lst):
                    gk[l, s, i], ge[l, s, i] = k, e
        dk = torch.from_numpy(_i64(gk.reshape(-1))).cuda()
        de = torch.from_numpy(_i32(ge.reshape(-1))).cuda()
        torch.cuda.synchronize()
        kv.merge_candidates(dk, de, L)
        kv.totals()  # (synchronises the sketch's stream: dk / de are read until then)
    torch.cuda.synchronize()


def _kv_assert(kv, ref, keys, where):
    import torch

    S, C = kv.num_services, kv.candidates
    for k in (C, 1):
        gk, ge, gc = kv.topk_all(k)
        rk, re_, rc = ref.topk_all(k)
        assert np.array_equal(gc, rc), f"{where}: list lengths (k = {k})"
        assert np.array_equal(ge.astype(np.uint64), re_), f"{where}: estimates (k = {k})"
        assert np.array_equal(gk, rk), f"{where}: keys (k = {k})"
    for s in range(S):
        assert kv.topk(s, C) == ref.lists[s], f"{where}: topk of service {s}"
    assert [int(t) for t in kv.totals()] == ref.totals, f"{where}: totals"
    torch.cuda.synchronize()
    got = sh.kv_views(kv)[0].cpu().numpy().view(np.uint32).reshape(S, kv.depth, kv.width)
    for s in range(S):
        assert np.array_equal(got[s].astype(np.uint64), ref.counters(s)), f"{where}: counters of service {s}"
        if keys:
            want = [ref.estimate(s, k) for k in keys]
            assert kv.estimate(s, np.array(keys, np.uint64)).tolist() == want, f"{where}: estimates of service {s}"


def _kv_run(case):
    cfg = case["cfg"]
    ref = R.run_kv_ref({**case, "ops": []})
    keys = R.offered_keys(case)
    if len(keys) > 600:  # point estimates of a sample: both ends of the key order and a stride between
        keys = keys[:200] + keys[200:-200:max(1, len(keys) // 200)] + keys[-200:]
    kv = _kv_open(cfg)
    try:
        for i, op in enumerate(case["ops"]):
            R.apply_kv_ref(ref, op)
            _kv_apply(kv, ref, op)
            _kv_assert(kv, ref, keys if cfg["S"] <= 4 or i == len(case["ops"]) - 1 else [], f"{case['name']} after op {i}")
    finally:
        kv.close()


KV_RUN = [c for c in R.kv_cases() if not any(op[0] == "total" for op in c["ops"])]


@pytest.mark.parametrize("case", KV_RUN, ids=lambda c: c["name"])
def test_kv_case_equals_the_reference(gpu, case):
    """Every case as it stands: below S * 8192 keys the counters stay in global memory (kSmall), the
    S = 1 runs of 65536 keys and more keep the rows in LDS."""
    _kv_run(case)


@pytest.mark.parametrize("case", [c for c in KV_RUN if c["cfg"]["S"] == 1
                                  and any(op[0] == "acc" and len(op[1]) < R.KV_SMALL for op in c["ops"])
                                  and not c["name"].startswith("edge_run_")], ids=lambda c: c["name"])
def test_kv_case_with_rows_in_lds(gpu, case):
    """The S = 1 cases again with every batch repeated up to 8192 keys: the same branches of the
    hash set, the ties and the hot-key combine with the count-min rows in LDS."""
    _kv_run(R.tiled_for_lds(case))


def test_kv_capacity_rule(gpu):
    """A service that counted 2^32 keys: every top-K query is ZK_ERR_CAPACITY; at 2^32 - 1 they answer."""
    for name, refused in (("u32_total_2^32-1_answers", False), ("u32_total_2^32_is_capacity", True)):
        case = R.kv_case(name)
        ref = R.run_kv_ref({**case, "ops": []})
        kv = _kv_open(case["cfg"])
        try:
            for op in case["ops"]:
                R.apply_kv_ref(ref, op)
                _kv_apply(kv, ref, op)
            assert [int(t) for t in kv.totals()] == ref.totals
            C = kv.candidates
            if refused:
                for query in (lambda: kv.topk_all(C), lambda: kv.topk_all(1), lambda: kv.topk(0, C), lambda: kv.topk(1, 1)):
                    with pytest.raises(ZkError) as e:
                        query()
                    assert e.value.status == _abi.ZK_ERR_CAPACITY
                assert kv.estimate(0, np.array([21], np.uint64)).tolist() == [5]  # point estimates still answer
            else:
                _kv_assert(kv, ref, [21, 22], name)
        finally:
            kv.close()


# ------------------------------------------------------------------ HyperLogLog + duration histogram
def _rt_open(cfg):
    from zipkin_amd.realtime import RtSketch

    rt = RtSketch(cfg["S"], hll_p=cfg["p"], sub_bits=cfg["m"], seed=cfg["seed"])
    assert (rt.registers, rt.bins) == (1 << cfg["p"], R.rt_nbins(cfg["m"]))
    return rt


def _rt_write(rt, op):
    import torch

    torch.cuda.synchronize()
    regs, hist = sh.rt_views(rt)
    if op[0] == "regs":
        regs.view(rt.num_services, rt.registers)[op[1]].fill_(op[2])
    else:
        row = hist.view(rt.num_services, rt.bins)[op[1]]
        for b, c in op[2].items():
            row[b] = int(_i32([c])[0])
    torch.cuda.synchronize()


def _rt_assert(rt, ref, where):
    regs, hist = rt.read()
    assert np.array_equal(regs, np.array(ref.regs, np.uint8)), f"{where}: registers"
    assert np.array_equal(hist.astype(np.uint64), np.array(ref.bins, np.uint64)), f"{where}: bins"
    assert rt.distinct_traces().tolist() == ref.distinct(), f"{where}: distinct traces"
    lo, hi, cnt = rt.quantiles_all(R.QS)  # the device scan (k_rt_query)
    for s in range(ref.S):
        want = ref.quantiles(s, R.QS)
        assert rt.quantiles(s, R.QS) == want, f"{where}: quantiles of service {s} (host scan)"
        assert (list(zip(lo[s].tolist(), hi[s].tolist())), int(cnt[s])) == want, f"{where}: quantiles_all, service {s}"
        mean, weight, val, n = rt.tdigest(s, 100.0, R.QS)
        cent, vmin, vmax, N = oracle_tdigest(np.array(ref.bins[s], np.uint64), ref.m, 100.0)
        assert n == N == ref.count(s) and sum(weight.tolist()) == N, f"{where}: t-digest counts of service {s}"
        assert mean.tolist() == [c[0] for c in cent] and weight.tolist() == [c[1] for c in cent]
        assert val.tolist() == [oracle_tdigest_quantile(cent, vmin, vmax, N, q) for q in R.QS]
    assert rt.dropped() == (ref.dropped_service, ref.dropped_duration), f"{where}: dropped"


@pytest.mark.parametrize("case", R.rt_cases(), ids=lambda c: c["name"])
def test_rt_case_equals_the_reference(gpu, case):
    ref = R.RtRef(**case["cfg"])
    rt = _rt_open(case["cfg"])
    try:
        for i, op in enumerate(case["ops"]):
            R.apply_rt_ref(ref, op)
            if op[0] == "acc":
                rt.accumulate_merged(op[1], op[2], op[3])
                _rt_assert(rt, ref, f"{case['name']} after batch {i}")
            else:
                _rt_write(rt, op)
        _rt_assert(rt, ref, case["name"])
    finally:
        rt.close()


@pytest.mark.parametrize("case", [c for c in R.rt_cases() if c["ops"][0][0] == "acc"], ids=lambda c: c["name"])
def test_rt_case_through_a_bound_context(gpu, case):
    """The register and duration cases as single-span traces through K1's emit path and the list
    partition (bind(only=True)): the same registers, bins and answers."""
    from zipkin_amd import DepsContext

    cfg = case["cfg"]
    ref = R.RtRef(**cfg)
    ctx = DepsContext(cfg["S"], device=0, strict=False)
    rt = _rt_open(cfg)
    try:
        rt.bind(ctx, only=True)
        first = 1
        for op in case["ops"]:
            R.apply_rt_ref(ref, op)
            cols = single_span_columns(*op[1:])
            cols.span_id[:] = np.arange(first, first + len(cols), dtype=np.uint64)
            first += len(cols)
            ctx.accumulate(cols)
        _rt_assert(rt, ref, case["name"])
    finally:
        rt.close()
        ctx.close()


def test_rt_bin_capacity_rule(gpu):
    """A u32 bin holds at most 2^32 - 1 spans since reset (include/zksketch.h). At 2^32 - 2 one more
    span of the bin is counted and every query answers; the next one wraps the bin, which the
    flush of k_rt_sketch sees: from then until reset the queries that read the bins are
    ZK_ERR_CAPACITY, and zk_rt_read / zk_rt_distinct_traces go on answering.

    (Before the rule existed the wrapped bin read 0 and zk_rt_quantiles answered count = 0 without an
    error.)"""
    cfg = dict(S=3, p=4, m=2, seed=9)
    d = 1000
    b = R.bin_of(d, cfg["m"])
    ref = R.RtRef(**cfg)
    rt = _rt_open(cfg)
    try:
        R.apply_rt_ref(ref, ("bins", 1, {b: R.M32 - 1}))
        _rt_write(rt, ("bins", 1, {b: R.M32 - 1}))
        one = (np.array([1], np.uint32), np.array([77], np.uint64), np.array([d], np.int64))
        ref.accumulate(*one)
        rt.accumulate_merged(*one)
        assert ref.bins[1][b] == R.M32
        _rt_assert(rt, ref, "bin at 2^32 - 1")
        rt.accumulate_merged(*one)  # 2^32 spans in the bin
        regs, hist = rt.read()
        print(f"bin {b} of service 1 after 2^32 spans reads {int(hist[1, b])}")
        assert np.array_equal(regs, np.array(ref.regs, np.uint8))
        assert rt.distinct_traces().tolist() == ref.distinct()
        for query in (lambda: rt.quantiles(1, R.QS), lambda: rt.quantiles(0, R.QS), lambda: rt.quantiles_all(R.QS),
                      lambda: rt.tdigest(1, 100.0, R.QS)):
            with pytest.raises(ZkError) as e:
                query()
            assert e.value.status == _abi.ZK_ERR_CAPACITY and "2^32" in str(e.value)
        rt.reset()
        assert rt.quantiles(1, R.QS) == ([(0, 0)] * len(R.QS), 0)
        fresh = R.RtRef(**cfg)
        fresh.accumulate(*one)
        rt.accumulate_merged(*one)
        _rt_assert(rt, fresh, "after reset")
    finally:
        rt.close()
