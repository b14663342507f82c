"""The crafted sketch cases of tests/sketchref.py, on the CPU: they reach every rare branch that
`classify_kv` / `classify_rt` name, and the independent reference agrees with oracle/kv.py,
oracle/realtime.py and the C ports on every case those can express -- before any of them is held
against the device (tests/test_gpu_sketch_bounds.py)."""
import random
from collections import Counter

import numpy as np
import pytest

from oracle.kv import KvOracle, kv_port
from oracle.kv import mix64 as oracle_mix64
from oracle.realtime import RtOracle, merged_span_items, rt_port
from oracle.realtime import tdigest as oracle_tdigest
from tests import sketchref as R
from zipkin_amd import SpanColumns


# ------------------------------------------------------------------------------------ the helpers
def test_unmix64_inverts_mix64():
    from tests.test_gpu_order import unmix64

    rng = random.Random(1)
    for z in [0, 1, R.M64, R.M64 - 1, 1 << 63, R.GOLDEN] + [rng.getrandbits(64) for _ in range(2000)]:
        assert R.mix64(R.unmix64(z)) == z and R.unmix64(R.mix64(z)) == z
        assert R.unmix64(z) == unmix64(z) and R.mix64(z) == oracle_mix64(z)


def test_keys_and_traces_with_a_chosen_hash():
    rng = random.Random(2)
    for seed in (0, 11, R.M64, rng.getrandbits(64)):
        s0 = R.kv_seed0(seed)
        assert s0 == KvOracle(1, width=64, seed=seed).seeds[0]
        for h in (0, R.EMPTY, 1 << 63, rng.getrandbits(64)):
            assert R.mix64(R.key_with_hash(h, s0) ^ s0) == h
            assert R.mix64(R.trace_with_hash(h, seed) ^ seed ^ R.RT_SALT) == h
    # the key that takes the empty-slot path is not the key ~0 (whose hash is an ordinary word)
    assert R.special_key() != R.M64 and R.mix64(R.M64 ^ R.kv_seed0(R.SPECIAL_SEED)) != R.EMPTY


def test_bins_tile_the_duration_range_and_are_found_by_search():
    from oracle.realtime import bins_of

    for m in (2, 7, 8):
        d = R.edge_durations(m)
        assert [R.bin_of(x, m) for x in d] == bins_of(np.array(d, np.uint64), m).tolist()
        assert R.bin_of(R.DMAX, m) == R.rt_nbins(m) - 1 and R.bin_of(0, m) == 0


# -------------------------------------------------------------------- every class has its cases
def _coverage(cases, classify):
    seen = Counter()
    for c in cases:
        seen.update(classify(c))
    return seen


def test_kv_cases_reach_every_class():
    seen = _coverage(R.kv_cases(), R.classify_kv)
    assert [k for k in R.KV_CLASSES if seen[k] < 1] == []
    assert seen["tie_at_cut"] >= 3
    # the LDS variant of the S = 1 cases: the same classes with the rows in LDS
    for name in ("special_at_cut", "chain_top_0x3ff_with_special", "hot_majority_changes", "tie_wider_than_list_c256"):
        c = R.kv_case(name)
        small, lds = R.classify_kv(c), R.classify_kv(R.tiled_for_lds(c))
        assert "rows_in_lds" in lds and "rows_in_global" not in lds
        assert {k for k in small if not k.startswith(("rows_", "run=="))} <= lds


def test_rt_cases_reach_every_class():
    seen = _coverage(R.rt_cases(), R.classify_rt)
    assert [k for k in R.RT_CLASSES if seen[k] < 1] == []
    assert seen["rank_on_chunk_edge"] >= 3
    for m in (2, 7, 8):  # both kinds of edge, at more than one of the ranks asked for
        ref = R.run_rt_ref(R.rt_case(f"queries_m{m}"))
        assert sum(R.chunk_edge_ranks(ref.bins[s]) for s in range(ref.S)) >= 6


# ------------------------------------------------------------- the reference against oracle/kv.py
SHRINK = 20  # counts of a weighted state are cut by 2^20 in the unweighted copy


def _oracle_for(ref):
    return KvOracle(ref.S, width=ref.width, depth=ref.depth, candidates=ref.cand, seed=ref.seed)


def _shard(o, lists_of_service):
    f = KvOracle(o.S, width=o.width, depth=o.depth, candidates=o.cand)
    f.seeds = list(o.seeds)
    for s, lst in lists_of_service.items():
        f.lists[s] = [(k, e) for k, e in lst if e]
    return f


def _shrunk(op):
    if op[0] != "state":
        return op
    return ("state", {s: {k: c >> SHRINK if c >> SHRINK else c for k, c in counts.items()} for s, counts in op[1].items()}, op[2])


def _apply_oracle(o, op, weighted):
    """One op on KvOracle. A weighted state is added to its counters directly (uint64 sums); its
    unweighted copy goes through accumulate, item by item."""
    if op[0] == "acc":
        o.accumulate(op[1], op[2])
    elif op[0] == "state":
        for s, counts in op[1].items():
            if weighted:
                for k, c in counts.items():
                    idx = o.rows(np.array([k], np.uint64))[:, 0]
                    for r in range(o.depth):
                        o.cm[s, r, idx[r]] += np.uint64(c)
                    o.totals[s] += np.uint64(c)
            else:
                ks = [k for k, c in counts.items() for _ in range(c)]
                o.accumulate(np.full(len(ks), s, np.uint32), np.array(ks, np.uint64))
        for s, lst in op[2].items():
            o.lists[s] = list(lst)
    elif op[0] == "merge":
        m = KvOracle.merged([o] + [_shard(o, l) for l in op[1]])
        o.cm, o.totals, o.lists = m.cm, m.totals, m.lists
    elif op[0] == "total":
        o.totals[op[1]] = np.uint64(op[2])
    return o


def _assert_kv_equal(ref, o, where):
    for k in (ref.cand, 1):
        rk, re_, rc = ref.topk_all(k)
        ok_, oe, oc = o.topk_all(k)
        assert np.array_equal(rc, oc), where
        assert np.array_equal(rk, ok_) and np.array_equal(re_, oe.astype(np.uint64)), where
    assert [int(t) for t in o.totals] == ref.totals, where
    for s in range(ref.S):
        assert np.array_equal(ref.counters(s), o.cm[s]), where


@pytest.mark.parametrize("case", R.kv_cases(), ids=lambda c: c["name"])
def test_kv_reference_equals_the_oracle(case):
    for weighted in (True, False):
        ops = case["ops"] if weighted else [_shrunk(op) for op in case["ops"]]
        if not weighted and not any(op[0] == "state" for op in ops):
            continue  # no weighted state to re-express
        ref = R.run_kv_ref({**case, "ops": []})
        o = _oracle_for(ref)
        for i, op in enumerate(ops):
            if not weighted and op[0] == "total":
                continue
            R.apply_kv_ref(ref, op)
            _apply_oracle(o, op, weighted)
            _assert_kv_equal(ref, o, f"{case['name']} op {i} weighted={weighted}")


@pytest.mark.parametrize("case", [c for c in R.kv_cases() if [op[0] for op in c["ops"]] == ["acc"]
                                  and len(c["ops"][0][1]) <= 80_000], ids=lambda c: c["name"])
def test_kv_reference_equals_the_c_port(case):
    cfg = case["cfg"]
    ref = R.run_kv_ref(case)
    p = kv_port(case["ops"][0][1], case["ops"][0][2], cfg["S"], cfg["width"], cfg["depth"], cfg["candidates"],
                seed=cfg["seed"], threads=2)
    for s in range(cfg["S"]):
        assert np.array_equal(ref.counters(s), p.cm[s].astype(np.uint64))
    assert [int(t) for t in p.totals] == ref.totals
    rk, re_, rc = ref.topk_all(cfg["candidates"])
    pk, pe, pc = p.topk_all(cfg["candidates"])
    assert np.array_equal(rc, pc) and np.array_equal(rk, pk) and np.array_equal(re_, pe.astype(np.uint64))


def test_kv_lds_copies_equal_the_oracle():
    """The tiled copies the device runs with the rows in LDS: same reference, same oracle."""
    for name in ("special_at_cut", "special_through_compactions", "chain_top_0x3ff_with_special", "hot_two_keys_32_32"):
        case = R.tiled_for_lds(R.kv_case(name))
        ref = R.run_kv_ref(case)
        o = _oracle_for(ref)
        for op in case["ops"]:
            _apply_oracle(o, op, True)
        _assert_kv_equal(ref, o, case["name"])


# ------------------------------------------------------- the reference against oracle/realtime.py
def single_span_columns(svc, tid, dur) -> SpanColumns:
    """Every item as a trace of one server span: what a bound DepsContext (K1's emit path) and
    oracle.realtime.rt_port take. duration = last - first, so -1 and 2^40 arrive as they are."""
    from tests.test_gpu_parity import SERVER

    n = len(svc)
    c = SpanColumns.empty(n)
    c.trace_id[:] = tid
    c.span_id[:] = np.arange(1, n + 1, dtype=np.uint64)
    c.first_ts[:] = 1 << 50
    c.last_ts[:] = (1 << 50) + np.asarray(dur, np.int64)
    c.service_id[:] = svc
    c.flags[:] = SERVER
    return c


def _apply_rt_oracle(o, op):
    if op[0] == "acc":
        o.accumulate_merged(op[1], op[2], op[3])
    elif op[0] == "regs":
        o.regs[op[1], :] = op[2]
    elif op[0] == "bins":
        for b, c in op[2].items():
            o.hist[op[1], b] = c


def _assert_rt_equal(ref, regs, hist, where):
    assert np.array_equal(np.array(ref.regs, np.uint8), regs), where
    assert np.array_equal(np.array(ref.bins, np.uint64), np.asarray(hist).astype(np.uint64)), where


@pytest.mark.parametrize("case", R.rt_cases(), ids=lambda c: c["name"])
def test_rt_reference_equals_the_oracle(case):
    cfg = case["cfg"]
    ref = R.RtRef(**cfg)
    o = RtOracle(cfg["S"], p=cfg["p"], m=cfg["m"], seed=cfg["seed"])
    for op in case["ops"]:
        R.apply_rt_ref(ref, op)
        _apply_rt_oracle(o, op)
    _assert_rt_equal(ref, o.regs, o.hist, case["name"])
    assert (ref.dropped_service, ref.dropped_duration) == (o.dropped_service, o.dropped_duration)
    assert ref.distinct() == o.distinct().tolist()
    for s in range(cfg["S"]):
        assert ref.quantiles(s, R.QS) == o.quantile_bins(s, R.QS)
        assert oracle_tdigest(o.hist[s], cfg["m"], 100.0)[3] == ref.count(s)


@pytest.mark.parametrize("case", [c for c in R.rt_cases() if c["ops"][0][0] == "acc"], ids=lambda c: c["name"])
def test_rt_reference_equals_the_c_port(case):
    """The items as single-span traces (clustered by traceId) through oracle/zk_rt_port.c."""
    cfg = case["cfg"]
    ref = R.run_rt_ref(case)
    cols = SpanColumns.concat([single_span_columns(*op[1:]) for op in case["ops"]])
    cols.span_id[:] = np.arange(1, len(cols) + 1, dtype=np.uint64)
    cols = cols.take(np.argsort(cols.trace_id, kind="stable"))
    svc, tid, dur, dropped = merged_span_items(cols, cfg["S"])
    assert len(svc) == sum(ref.count(s) for s in range(cfg["S"])) and dropped == ref.dropped_duration
    r = rt_port(cols, cfg["S"], p=cfg["p"], m=cfg["m"], seed=cfg["seed"], threads=2)
    _assert_rt_equal(ref, r.regs, r.hist, case["name"])
    assert r.dropped_duration == ref.dropped_duration
    assert r.distinct().tolist() == ref.distinct()
