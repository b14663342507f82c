"""TEST INFRASTRUCTURE ONLY -- an independent reference for the two per-service sketches at the bounds
of their domain, and the crafted cases that reach them.

Python integers only, written from the definitions in include/zksketch.h and
zipkin_amd/csrc/zk_sketch_internal.h: nothing here imports oracle/ or zipkin_amd, so it is independent
of both (tests/test_sketch_cases.py holds the three against each other). It plays for the count-min +
top-K sketch (zk_kv) and the HyperLogLog + duration-histogram sketch (zk_rt) the role tests/exactref.py
plays for the link table: `classify_kv` / `classify_rt` say from the inputs alone which rare branch of
the kernels a case must take, so the case lists below can be required to reach every one of them.

splitmix64's finalizer is a bijection (`unmix64` is its inverse), so a case chooses HASHES -- the
empty-slot word of the candidate hash set, a probe chain, a register index and rank -- and turns
them back into keys and traceIds with `key_with_hash` / `trace_with_hash`."""
from __future__ import annotations

import bisect
import functools
import math
import random
from collections import Counter

import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
GOLDEN = 0x9E3779B97F4A7C15
RT_SALT = 0xD6E8FEB86659FD93  # kRtSalt
EMPTY = M64                   # kEmptyKey: the empty-slot word of the candidate hash set
SET_BITS = 10                 # kSetBits: the hash set has 2^10 slots, a key's first slot = its hash's top bits
SORT_CAP = 512                # kSortCap: entries the set holds before it is compacted
KV_WG, KV_U = 512, 4          # k_kv_sketch: threads, keys per thread; a block = 2048 keys
KV_BLOCK = KV_WG * KV_U       # also k_kv_candidates' block (J = 4 keys per thread)
KV_UNIT = 65536               # kKvUnitItems
KV_SMALL = 8192               # kKvSmallPerService: below S * 8192 keys the counters stay in global memory
RT_UNIT = 65536               # kRtUnitItems
RT_QUERY_WG = 256             # k_rt_query: threads, each a contiguous chunk of bins
DMAX = (1 << 40) - 1          # the largest accepted duration


def mix64(z: int) -> int:
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def unmix64(z: int) -> int:
    """Inverse of mix64 (sk_unmix64): x ^= x >> k is undone by x ^= x >> k ^ x >> 2k ..., the
    multiplications by the constants' inverses mod 2^64."""
    z &= M64
    z = (z ^ (z >> 31) ^ (z >> 62)) & M64
    z = (z * 0x319642B2D24D8EC3) & M64
    z = (z ^ (z >> 27) ^ (z >> 54)) & M64
    z = (z * 0x96DE1B173F119089) & M64
    return (z ^ (z >> 30) ^ (z >> 60)) & M64


def kv_seed0(seed: int) -> int:
    """seeds[0] of zk_kv_create: the one seed every row index derives from."""
    return mix64((seed + GOLDEN) & M64)


def key_with_hash(h: int, seed0: int) -> int:
    """The key whose count-min hash mix64(key ^ seed0) is h."""
    return unmix64(h) ^ seed0


def trace_with_hash(h: int, seed: int) -> int:
    """The traceId whose register hash mix64(traceId ^ seed ^ kRtSalt) is h."""
    return unmix64(h) ^ (seed & M64) ^ RT_SALT


# ------------------------------------------------------------------------------ count-min + top-K
class KvRef:
    """Per service: counters as a dict {(row, index): sum}, the total, and the candidate list
    [(key, estimate)] best first. A batch is a multiset {key: count} per service."""

    def __init__(self, S: int, width: int, depth: int = 4, candidates: int = 64, seed: int = 0):
        assert width & (width - 1) == 0
        self.S, self.width, self.depth, self.cand = S, width, depth, candidates
        self.wbits = width.bit_length() - 1
        self.seed, self.seed0 = seed, kv_seed0(seed)
        self.cm = [Counter() for _ in range(S)]
        self.totals = [0] * S
        self.lists: list[list[tuple[int, int]]] = [[] for _ in range(S)]
        self.dropped = 0

    def hash(self, key: int) -> int:
        return mix64(key ^ self.seed0)

    def rows(self, key: int) -> list[int]:
        """Row r: the top log2(width) bits of (h1 + r * h2) mod 2^32, h1 / h2 the halves of ONE hash."""
        h = self.hash(key)
        h1, h2 = h & M32, (h >> 32) | 1
        return [((h1 + r * h2) & M32) >> (32 - self.wbits) for r in range(self.depth)]

    def estimate(self, s: int, key: int) -> int:
        cm = self.cm[s]
        return min(cm.get((r, i), 0) for r, i in enumerate(self.rows(key)))

    def add(self, s: int, counts: dict) -> None:
        cm = self.cm[s]
        for key, c in counts.items():
            for r, i in enumerate(self.rows(key)):
                cm[(r, i)] += c
            self.totals[s] += c

    def relist(self, s: int, offered) -> None:
        """Top `candidates` of (previous list U offered) by (estimate desc, key asc), estimate 0 dropped."""
        keys = {k for k, _ in self.lists[s]} | set(offered)
        est = sorted(((self.estimate(s, k), k) for k in keys), key=lambda t: (-t[0], t[1]))
        self.lists[s] = [(k, e) for e, k in est if e > 0][: self.cand]

    def accumulate(self, batch: dict) -> None:
        """batch = {service: {key: count}}; every service's list is re-made, as k_kv_merge does."""
        for s, counts in batch.items():
            self.add(s, counts)
        for s in range(self.S):
            self.relist(s, batch.get(s, {}).keys())

    def accumulate_items(self, svc, keys) -> None:
        batch: dict = {}
        for s, k in zip(np.asarray(svc).tolist(), np.asarray(keys, dtype=np.uint64).tolist()):
            if s >= self.S:
                self.dropped += 1
            else:
                batch.setdefault(s, Counter())[k] += 1
        self.accumulate(batch)

    def merge_candidates(self, lists) -> None:
        """zk_kv_merge_candidates: lists = [{service: [(key, stored estimate)]}]; an entry is offered
        when its stored estimate is non-zero, and ranked by the CURRENT counters."""
        for s in range(self.S):
            self.relist(s, [k for lst in lists for k, e in lst.get(s, []) if e])

    def counters(self, s: int) -> np.ndarray:
        out = np.zeros((self.depth, self.width), np.uint64)
        for (r, i), c in self.cm[s].items():
            out[r, i] = c
        return out

    def topk_all(self, k: int):
        keys = np.zeros((self.S, k), np.uint64)
        est = np.zeros((self.S, k), np.uint64)
        cnt = np.zeros(self.S, np.uint32)
        for s in range(self.S):
            lst = self.lists[s][:k]
            cnt[s] = len(lst)
            for i, (kk, e) in enumerate(lst):
                keys[s, i], est[s, i] = kk, e
        return keys, est, cnt


# ------------------------------------------------------------------ HyperLogLog + duration histogram
def rt_nbins(m: int) -> int:
    return (41 - m) << m


def bin_bounds(b: int, m: int) -> tuple[int, int]:
    """[lo, hi] of bin b: below 2^m a bin is one value; above, group g = b >> m holds the values with
    exponent e = g + m - 1, cut by their top m mantissa bits into 2^m bins of 2^(e - m) values."""
    if b < (1 << m):
        return b, b
    g, mant = b >> m, b & ((1 << m) - 1)
    e = g + m - 1
    lo = ((1 << m) + mant) << (e - m)
    return lo, lo + (1 << (e - m)) - 1


@functools.lru_cache(maxsize=None)
def _bin_los(m: int) -> tuple:
    los, nxt = [], 0
    for b in range(rt_nbins(m)):
        lo, hi = bin_bounds(b, m)
        assert lo == nxt and hi >= lo, "the bins do not tile the integers"
        los.append(lo)
        nxt = hi + 1
    assert nxt == 1 << 40, "the bins do not end at 2^40 - 1"
    return tuple(los)


def bin_of(d: int, m: int) -> int:
    """The bin whose [lo, hi] holds d, found by searching the tiling (not by restating rt_bin)."""
    assert 0 <= d <= DMAX
    return bisect.bisect_right(_bin_los(m), d) - 1


def hll_fields(trace_id: int, p: int, seed: int) -> tuple[int, int]:
    h = mix64(trace_id ^ (seed & M64) ^ RT_SALT)
    w = (h << p) & M64
    return h >> (64 - p), (64 - w.bit_length() + 1) if w else 64 - p + 1


def nearest_rank(q: float, n: int) -> int:
    return min(max(math.ceil(q * float(n)), 1), n)


def hll_estimate(regs, p: int) -> float:
    """hll_estimate of zk_rt_api.cpp on the exact integer z = sum 2^(64 - M[j]): one rounding to
    double, scaled by 2^-64; linear counting when the raw estimate is <= 2.5 m and a register is 0."""
    mm = 1 << p
    z = sum(1 << (64 - int(r)) for r in regs)
    zeros = sum(1 for r in regs if int(r) == 0)
    Z = math.ldexp(float(z), -64)
    m = float(mm)
    alpha = {16: 0.673, 32: 0.697, 64: 0.709}.get(mm, 0.7213 / (1.0 + 1.079 / m))
    e = alpha * m * m / Z
    if e <= 2.5 * m and zeros > 0:
        e = m * math.log(m / float(zeros))
    return e


class RtRef:
    def __init__(self, S: int, p: int = 14, m: int = 7, seed: int = 0):
        self.S, self.p, self.m, self.seed = S, p, m, seed
        self.nbins = rt_nbins(m)
        self.regs = [[0] * (1 << p) for _ in range(S)]
        self.bins = [[0] * self.nbins for _ in range(S)]
        self.dropped_service = self.dropped_duration = 0

    def accumulate(self, svc, tid, dur) -> None:
        for s, t, d in zip(np.asarray(svc).tolist(), np.asarray(tid, dtype=np.uint64).tolist(),
                           np.asarray(dur, dtype=np.int64).tolist()):
            if s >= self.S:
                self.dropped_service += 1
            elif d < 0 or d > DMAX:
                self.dropped_duration += 1
            else:
                i, rho = hll_fields(t, self.p, self.seed)
                if rho > self.regs[s][i]:
                    self.regs[s][i] = rho
                self.bins[s][bin_of(d, self.m)] += 1

    def count(self, s: int) -> int:
        return sum(self.bins[s])

    def quantiles(self, s: int, qs):
        """([(lo, hi)] of the bin holding each nearest rank, N); all 0 when N = 0."""
        n = self.count(s)
        out = []
        for q in qs:
            if n == 0:
                out.append((0, 0))
                continue
            rank, cum = nearest_rank(q, n), 0
            for b, c in enumerate(self.bins[s]):
                cum += c
                if cum >= rank:
                    out.append(bin_bounds(b, self.m))
                    break
        return out, n

    def distinct(self) -> list[float]:
        return [hll_estimate(self.regs[s], self.p) for s in range(self.S)]


# ------------------------------------------------------------------------------------ the KV cases
# A case: name, cfg (S, width, depth, candidates, seed) and ops, run in order:
#   ("acc", svc u32[n], keys u64[n])        one zk_kv_accumulate
#   ("state", {s: {key: count}}, {s: [(key, est)]})
#                                           weighted state: the counts are ADDED to the counters and
#                                           totals and the candidate lists are REPLACED by the given
#                                           (possibly stale, unordered) ones -- on the device through
#                                           shards.kv_views, no kernel runs
#   ("merge", [{s: [(key, est)]}, ...])     zk_kv_merge_candidates with these gathered lists
#   ("total", s, value)                     a total overwritten (the capacity rule)
def _kv_case(name, S, width, depth, cand, seed, ops):
    return {"name": name, "cfg": dict(S=S, width=width, depth=depth, candidates=cand, seed=seed), "ops": ops}


def _items(batch: dict, rng: random.Random | None = None):
    """{service: {key: count}} -> (svc, keys) arrays, shuffled when an rng is given."""
    rows = [(s, k) for s, counts in batch.items() for k, c in counts.items() for _ in range(c)]
    if rng is not None:
        rng.shuffle(rows)
    return (np.array([r[0] for r in rows], np.uint32), np.array([r[1] for r in rows], np.uint64))


def _chain_keys(top: int, n: int, seed0: int) -> list[int]:
    """n keys whose hashes share the top SET_BITS bits `top`: one probe chain of the hash set."""
    low = 64 - SET_BITS
    return [key_with_hash((top << low) | ((i * 0x2545F4914F6CDD1D + 0x1B873593) & ((1 << low) - 1)), seed0)
            for i in range(n)]


SPECIAL_SEED = 11


def special_key(seed: int = SPECIAL_SEED) -> int:
    """The key whose hash is the hash set's empty-slot word (TopSet::special)."""
    return key_with_hash(EMPTY, kv_seed0(seed))


def _special_cases():
    sd, C = SPECIAL_SEED, 8
    sp = special_key(sd)
    lo1, lo2, hi1, hi2 = 3, 5, sp + 1, sp + 2  # keys on both sides of the special key in key order
    assert lo2 < sp < hi1 < hi2 <= M64
    heavy = {100 + i: 40 - i for i in range(6)}
    out = [
        _kv_case("special_alone", 1, 64, 4, C, sd, [("acc", *_items({0: {sp: 1}}))]),
        _kv_case("special_best", 2, 64, 4, C, sd,
                 [("acc", *_items({1: {sp: 10, 7: 9, 8: 3, 9: 3}}, random.Random(1)))]),
        # six heavier keys, then a four-way tie of which the list takes two: a smaller key and the
        # special key (the last entry); the two larger keys stay outside
        _kv_case("special_at_cut", 1, 4096, 4, C, sd,
                 [("acc", *_items({0: {**heavy, lo1: 3, sp: 3, hi1: 3, hi2: 3}}, random.Random(2)))]),
        _kv_case("special_inside_tie", 1, 4096, 4, C, sd,
                 [("acc", *_items({0: {**heavy, sp: 3, hi1: 3, hi2: 3, lo1: 2}}, random.Random(3)))]),
        _kv_case("special_below_cut", 1, 4096, 4, C, sd,
                 [("acc", *_items({0: {**heavy, lo1: 5, lo2: 5, hi1: 4, sp: 1}}, random.Random(4)))]),
        _kv_case("special_only_in_previous_list", 2, 4096, 4, C, sd,
                 [("acc", *_items({0: {sp: 4, 7: 2}, 1: {sp: 1}})), ("acc", *_items({0: {7: 1, 9: 9}, 1: {12: 2}}))]),
        # 1500 distinct keys, each once: the first block's survivors are inserted in steps with a
        # compaction between them, the special key (3 times, every block) among them
        _kv_case("special_through_compactions", 1, 4096, 4, C, sd,
                 [("acc", *_items({0: {**{mix64(i + 77): 1 for i in range(1500)}, sp: 3}}, random.Random(5)))]),
        # counted, but in no list of this handle: a gathered list offers it with a stale estimate
        _kv_case("special_from_gathered_list", 2, 4096, 4, C, sd,
                 [("state", {0: {sp: 9, 7: 12, 8: 2}, 1: {8: 1}}, {0: [(8, 1), (7, 5)], 1: []}),
                  ("merge", [{0: [(7, 3)]}, {0: [(sp, 1), (55, 4)], 1: [(sp, 7)]}])]),
    ]
    return out


def _chain_cases():
    sd, C = SPECIAL_SEED, 8
    s0 = kv_seed0(sd)
    sp = special_key(sd)
    out = []
    for top in ((1 << SET_BITS) - 1, 0):
        keys = _chain_keys(top, 300, s0)
        counts = {k: 1 + (i * 7) % 37 for i, k in enumerate(keys)}
        out.append(_kv_case(f"chain_top_{top:#x}", 1, 64, 4, C, sd, [("acc", *_items({0: counts}, random.Random(top + 6)))]))
        with_sp = {**counts, sp: 30, 0: 30}
        out.append(_kv_case(f"chain_top_{top:#x}_with_special", 1, 64, 4, C, sd,
                            [("acc", *_items({0: with_sp}, random.Random(top + 7)))]))
    return out


def _tie_cases():
    keys = [mix64(i + 1) for i in range(5000)]
    svc, arr = np.zeros(5000, np.uint32), np.array(keys, np.uint64)
    out = []
    for C in (256, 255, 1):
        ops = [("acc", svc, arr)]
        if C == 256:  # a second batch lifts exactly one key of the tie at the cut over it
            ref = KvRef(1, 4096, 4, C, 3)
            ref.accumulate_items(svc, arr)
            cut = ref.lists[0][-1][1]
            outside = sorted(k for k in keys if ref.estimate(0, k) == cut and k not in dict(ref.lists[0]))
            ops.append(("acc", np.zeros(1, np.uint32), np.array([outside[-1]], np.uint64)))
        out.append(_kv_case(f"tie_wider_than_list_c{C}", 1, 4096, 4, C, 3, ops))
    return out


def _hot_cases():
    sd = SPECIAL_SEED
    sp = special_key(sd)
    a, b = 0xA11CE, 0xB0B
    blocks = {
        "hot_one_key_every_lane": [a] * KV_BLOCK,
        "hot_two_keys_32_32": ([a] * 32 + [b] * 32) * (KV_BLOCK // 64),
        # key i of a block is read by thread i mod 512 in instruction i div 512, so wave w's
        # instruction e reads the 64 keys from (e * 8 + w) * 64: the majority alternates with e
        "hot_majority_changes": [k for g in range(KV_BLOCK // 64)
                                 for k in (([a] * 40 + [b] * 24) if (g // 8) % 2 == 0 else ([a] * 24 + [b] * 40))],
        "hot_special_majority": ([sp] * 48 + [a] * 16) * (KV_BLOCK // 64),
    }
    return [_kv_case(n, 1, 256, 4, 4, sd, [("acc", np.zeros(len(k), np.uint32), np.array(k, np.uint64))])
            for n, k in blocks.items()]


EDGE_RUNS = (1, 2047, 2048, 2049, 4096, 4097, 65536, 65537, 131073)


def _run_keys(n: int, salt: int) -> np.ndarray:
    """n keys drawn from five, in a fixed irregular order: every counter has a known value."""
    pool = np.array([mix64(salt * 8 + j) for j in range(5)], np.uint64)
    return pool[((np.arange(n, dtype=np.uint64) * np.uint64(2654435761) >> np.uint64(7)) % np.uint64(5)).astype(np.int64)]


def _edge_cases():
    out = []
    # counters in global memory: S = 17, n < 17 * 8192, runs beside empty and one-key services, the
    # last service among the non-empty ones
    for name, runs in (("edge_runs_small_a", {0: 2047, 2: 1, 3: 2048, 5: 2049, 6: 1, 8: 4096, 11: 4097, 12: 65536, 16: 1}),
                       ("edge_runs_small_b", {1: 65537, 2: 1, 16: 2049}),
                       ("edge_runs_small_c", {4: 1, 7: 131073, 16: 1})):
        svc = np.concatenate([np.full(n, s, np.uint32) for s, n in runs.items()])
        keys = np.concatenate([_run_keys(n, s) for s, n in runs.items()])
        perm = np.random.default_rng(len(svc)).permutation(len(svc))
        assert len(svc) < 17 * KV_SMALL
        out.append(_kv_case(name, 17, 256, 4, 4, 2, [("acc", svc[perm], keys[perm])]))
    for n in EDGE_RUNS:  # S = 1: rows in LDS from 8192 keys on
        out.append(_kv_case(f"edge_run_{n}", 1, 256, 4, 4, 2, [("acc", np.zeros(n, np.uint32), _run_keys(n, n))]))
    return out


def _u32_cases():
    A, B, D, E, F, G, H = 21, 22, 23, 24, 25, 26, 27
    state = {0: {A: (1 << 31) - 1, B: 1 << 31},       # total 2^32 - 1; unsigned order: B, A
             1: {D: (1 << 32) - 2, E: 1},             # total 2^32 - 1
             2: {F: (1 << 32) - 1},                   # the value estimate_rh starts from
             3: {G: (1 << 31) - 1, H: (1 << 31) - 1}}  # total 2^32 - 2: one more G crosses 2^31
    stale = {0: [(A, 7), (B, 3)], 1: [(E, 9), (D, 1)], 2: [(F, 1)], 3: [(H, 2), (G, 1)]}
    top = [("state", state, stale), ("merge", []),
           ("acc", np.array([3], np.uint32), np.array([G], np.uint64))]
    return [
        _kv_case("u32_estimates_at_the_bound", 4, 4096, 4, 4, 5, top),
        _kv_case("u32_total_2^32-1_answers", 2, 64, 2, 2, 5, [("state", {0: {A: 5}}, {0: [(A, 5)]}), ("total", 0, (1 << 32) - 1)]),
        _kv_case("u32_total_2^32_is_capacity", 2, 64, 2, 2, 5, [("state", {0: {A: 5}}, {0: [(A, 5)]}), ("total", 1, 1 << 32)]),
    ]


MERGE_LISTS = 8


def _merge_cases():
    sd, C = SPECIAL_SEED, 128
    sp = special_key(sd)
    counted = [mix64(i + 9000) for i in range(900)]
    batch = {0: {**{k: 1 + i % 11 for i, k in enumerate(counted)}, sp: 6}, 1: {counted[0]: 2}}
    never = [mix64(i + 50_000) for i in range(40)]
    lists = []
    for l in range(MERGE_LISTS):
        # 100 counted keys per list, overlapping the next list's by 30 (duplicates across lists),
        # with stale estimates; never-counted keys with non-zero estimates; the special key twice
        ks = counted[l * 70: l * 70 + 100] + never[l * 5: l * 5 + 5] + ([sp] if l in (2, 6) else [])
        lists.append({0: [(k, 1 + (i * 13 + l) % 50) for i, k in enumerate(ks)], 1: [(never[l], 3)]})
    return [_kv_case("merge_eight_lists", 2, 4096, 4, C, sd, [("acc", *_items(batch, random.Random(8))), ("merge", lists)])]


@functools.lru_cache(maxsize=None)
def kv_cases() -> tuple:
    return tuple(_special_cases() + _chain_cases() + _tie_cases() + _hot_cases() + _edge_cases() + _u32_cases()
                 + _merge_cases())


def kv_case(name: str) -> dict:
    return next(c for c in kv_cases() if c["name"] == name)


def tiled_for_lds(case: dict) -> dict:
    """The same case with every batch repeated until it holds >= 8192 keys, S = 1 only: zk_kv_accumulate
    then keeps the rows in LDS. Every count is multiplied, so ties and order stay as they are."""
    assert case["cfg"]["S"] == 1
    ops = []
    for op in case["ops"]:
        if op[0] == "acc" and len(op[1]) < KV_SMALL:
            rep = -(-KV_SMALL // len(op[1]))
            op = ("acc", np.tile(op[1], rep), np.tile(op[2], rep))
        ops.append(op)
    return {"name": case["name"] + "_lds", "cfg": case["cfg"], "ops": ops}


def run_kv_ref(case: dict, upto: int | None = None):
    """The reference after the case's ops (or its first `upto`); "total" ops only set the total."""
    ref = KvRef(case["cfg"]["S"], case["cfg"]["width"], case["cfg"]["depth"], case["cfg"]["candidates"], case["cfg"]["seed"])
    for op in case["ops"][:upto]:
        apply_kv_ref(ref, op)
    return ref


def apply_kv_ref(ref: KvRef, op) -> None:
    if op[0] == "acc":
        ref.accumulate_items(op[1], op[2])
    elif op[0] == "state":
        for s, counts in op[1].items():
            ref.add(s, counts)
        for s, lst in op[2].items():
            ref.lists[s] = list(lst)
    elif op[0] == "merge":
        ref.merge_candidates(op[1])
    elif op[0] == "total":
        ref.totals[op[1]] = op[2]
    else:
        raise ValueError(op[0])


def offered_keys(case: dict) -> list[int]:
    """Every key a case counts or offers (the keys whose point estimates a test compares)."""
    keys: set = set()
    for op in case["ops"]:
        if op[0] == "acc":
            keys.update(np.unique(op[2]).tolist())
        elif op[0] == "state":
            keys.update(k for c in op[1].values() for k in c)
            keys.update(k for lst in op[2].values() for k, _ in lst)
        elif op[0] == "merge":
            keys.update(k for l in op[1] for lst in l.values() for k, _ in lst)
    return sorted(keys)


def classify_kv(case: dict) -> set:
    """The rare paths a KV case must take, named from its inputs and the reference's arithmetic alone."""
    cfg = case["cfg"]
    ref = KvRef(cfg["S"], cfg["width"], cfg["depth"], cfg["candidates"], cfg["seed"])
    out: set = set()
    for op in case["ops"]:
        offered: dict = {}  # service -> keys the op offers beside the previous list
        if op[0] == "acc":
            svc, keys = np.asarray(op[1]), np.asarray(op[2])
            n = len(svc)
            out.add("rows_in_lds" if n >= cfg["S"] * KV_SMALL else "rows_in_global")
            for s in np.unique(svc).tolist():
                ks = keys[svc == s].tolist()
                offered[s] = set(ks)
                run = len(ks)
                for name, v in (("run==1", 1), ("run==block-1", KV_BLOCK - 1), ("run==block", KV_BLOCK),
                                ("run==block+1", KV_BLOCK + 1), ("run==2blocks", 2 * KV_BLOCK),
                                ("run==2blocks+1", 2 * KV_BLOCK + 1), ("run==unit", KV_UNIT),
                                ("run==unit+1", KV_UNIT + 1), ("run==2units+1", 2 * KV_UNIT + 1)):
                    if run == v:
                        out.add(name)
                distinct = offered[s]
                if len(distinct) >= 2 * SORT_CAP:
                    out.add("compactions>=2")
                # probe chains: every distinct key of a run that fits the set uncompacted is inserted;
                # keys that repeat in a later block are then looked up past their first two slots
                if len(distinct) <= SORT_CAP and run > 2 * KV_BLOCK:
                    slots = Counter(ref.hash(k) >> (64 - SET_BITS) for k in distinct if ref.hash(k) != EMPTY)
                    for slot, c in slots.items():
                        if c >= 3:
                            out.add("chain_len>=3")
                        if slot + c > (1 << SET_BITS):
                            out.add("chain_wraps")
                if cfg["S"] == 1:  # the wave layout survives the partition only in whole 64-key groups
                    groups = [Counter(ks[g: g + 64]) for g in range(0, run - run % 64, 64)]
                    major = [c.most_common(1)[0] for c in groups]
                    if any(m[1] == 64 for m in major):
                        out.add("hot_wave_full")
                    if any(len(c) == 2 and m[1] == 32 for c, m in zip(groups, major)):
                        out.add("hot_wave_split")
                    if any(x[0] != y[0] and x[1] > 32 and y[1] > 32 for x, y in zip(major, major[8:])):
                        out.add("hot_key_changes")
                    if any(ref.hash(m[0]) == EMPTY and m[1] > 32 for m in major):
                        out.add("hot_key_special")
        elif op[0] == "merge":
            out.add(f"merge_lists=={len(op[1])}")
            for s in range(cfg["S"]):
                entries = [(k, e) for l in op[1] for k, e in l.get(s, [])]
                offered[s] = {k for k, e in entries if e}
                if len(entries) > len({k for k, _ in entries}):
                    out.add("merge_duplicates")
                if len(offered[s] | {k for k, _ in ref.lists[s]}) > SORT_CAP:
                    out.add("merge_compacts")
        before = [dict(l) for l in ref.lists]
        apply_kv_ref(ref, op)
        if op[0] == "total":
            out.add("total>=2^32" if op[2] >> 32 else "total==2^32-1" if op[2] == M32 else "total_written")
            continue
        if op[0] == "state":
            continue
        for s in range(cfg["S"]):
            pool = set(before[s]) | offered.get(s, set())
            if any(ref.hash(k) == EMPTY for k in pool):
                out.add("special_key")
                if ref.hash(next(iter(pool))) == EMPTY and len(pool) == 1:
                    out.add("special_alone")
                if ref.lists[s] and ref.hash(ref.lists[s][0][0]) == EMPTY:
                    out.add("special_best")
                if op[0] == "merge":
                    out.add("special_in_merge")
                elif not any(ref.hash(k) == EMPTY for k in offered.get(s, ())):
                    out.add("special_only_in_previous_list")
            if op[0] == "merge" and any(ref.estimate(s, k) == 0 for k in offered.get(s, ())):
                out.add("merge_stale_entry")
            lst = ref.lists[s]
            if len(lst) == ref.cand:
                cut = lst[-1][1]
                inside = dict(lst)
                tied_out = [k for k in pool if k not in inside and ref.estimate(s, k) == cut]
                if tied_out:
                    out.add("tie_at_cut")
                    if ref.hash(lst[-1][0]) == EMPTY and any(e == cut for _, e in lst[:-1]):
                        out.add("special_at_cut")
                    if any(ref.hash(k) == EMPTY for k in tied_out):
                        out.add("special_tied_outside")
                if any(ref.hash(k) == EMPTY and k not in inside and ref.estimate(s, k) < cut for k in pool):
                    out.add("special_below_cut")
            if any(e >= 1 << 31 for _, e in lst):
                out.add("est>=2^31")
            if any(e == M32 for _, e in lst):
                out.add("est==2^32-1")
    return out


KV_CLASSES = (
    "special_key", "special_alone", "special_best", "special_at_cut", "special_below_cut",
    "special_only_in_previous_list", "special_in_merge", "chain_len>=3", "chain_wraps", "tie_at_cut",
    "est>=2^31", "est==2^32-1", "total==2^32-1", "total>=2^32", "hot_wave_full", "hot_wave_split",
    "hot_key_changes", "hot_key_special", "compactions>=2", "rows_in_global", "rows_in_lds", "run==1",
    "run==block-1", "run==block", "run==block+1", "run==2blocks", "run==2blocks+1", "run==unit", "run==unit+1",
    "run==2units+1", f"merge_lists=={MERGE_LISTS}", "merge_lists==0", "merge_duplicates", "merge_stale_entry",
    "merge_compacts",
)


# ------------------------------------------------------------------------------------ the RT cases
# A case: name, cfg (S, p, m, seed), ops and the quantiles to ask:
#   ("acc", svc u32[n], tid u64[n], dur i64[n])   one zk_rt_accumulate_merged
#   ("regs", s, value)                            every register of service s written (rt_views)
#   ("bins", s, {bin: count})                     bins of service s written (rt_views)
QS = (0.0, 1e-300, 0.07, 0.5, 1.0 - 2.0 ** -53, 1.0)


def _rt_case(name, S, p, m, seed, ops):
    return {"name": name, "cfg": dict(S=S, p=p, m=m, seed=seed), "ops": ops}


def _tid(idx: int, rho: int, p: int, seed: int, low: int = 0) -> int:
    """A traceId with register index idx and rank rho (rho = 64 - p + 1: every remaining bit zero)."""
    rest = 64 - p
    assert 1 <= rho <= rest + 1 and 0 <= idx < 1 << p
    w = 0 if rho == rest + 1 else (1 << (rest - rho)) | (low & ((1 << (rest - rho)) - 1))
    t = trace_with_hash((idx << rest) | w, seed)
    assert hll_fields(t, p, seed) == (idx, rho)
    return t


def _register_case(p: int):
    seed, m, R, rest = 17 + p, 7, 1 << p, 64 - p
    rng = random.Random(p)
    b1: list = []  # (service, traceId, duration)
    for idx in (0, R - 1):
        for rho in (1, rest, rest + 1):
            b1.append((0, _tid(idx, rho, p, seed), 10 * rho))
    b1 += [(0, _tid(4 + k, 2 + k, p, seed, rng.getrandbits(60)), k) for k in range(4)]  # one word, four values
    for n, base in ((64, 8), (256, 8)):  # one LDS word from every lane of a wave, of a workgroup
        b1 += [(1 if n == 64 else 2, _tid(base + rng.randrange(4), rng.randint(1, rest + 1), p, seed, rng.getrandbits(60)), i)
               for i in range(n)]
    # byte 0 of word 3 ends higher than anything the second batch brings; its byte 1 is raised
    b1 += [(3, _tid(12, 9, p, seed, 5), 1), (3, _tid(13, 2, p, seed, 6), 2)]
    b2 = [(3, _tid(12, 3, p, seed, 7), 3), (3, _tid(13, 5, p, seed, 8), 4)]
    # 65537 items, rank below the maximum everywhere but in the last one: the second unit's flush
    n5 = RT_UNIT + 1
    t5 = [trace_with_hash(mix64(i + (p << 20)) | (1 << 20), seed) for i in range(n5 - 1)] + [_tid(R // 2, rest + 1, p, seed)]
    b1 += [(4, t, 1000 + i % 977) for i, t in enumerate(t5)]

    def arrays(rows):
        return (np.array([r[0] for r in rows], np.uint32), np.array([r[1] for r in rows], np.uint64),
                np.array([r[2] for r in rows], np.int64))

    return _rt_case(f"registers_p{p}", 5, p, m, seed, [("acc", *arrays(b1)), ("acc", *arrays(b2))])


def edge_durations(m: int) -> list[int]:
    d = [0, (1 << m) - 1, 1 << m, (1 << m) + 1, DMAX]
    for k in range(1, 40):
        d += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    return d


def _duration_case(m: int):
    d = edge_durations(m) + [1 << 40, -1]  # the last two are only counted as dropped
    n = len(d)
    return _rt_case(f"durations_m{m}", 2, 8, m, 3, [("acc", np.ones(n, np.uint32), np.arange(1, n + 1, dtype=np.uint64) * np.uint64(GOLDEN),
                                                     np.array(d, np.int64))])


def _query_case(m: int):
    nb = rt_nbins(m)
    chunk = -(-nb // RT_QUERY_WG)
    c0 = 37 * chunk  # the first bin of thread 37's chunk
    ops = [("bins", 0, {0: 10}), ("bins", 1, {0: 7}), ("bins", 2, {nb - 1: 10}), ("bins", 3, {nb - 1: 7})]
    for s, N in ((4, 100), (5, 101)):
        r07, r50 = nearest_rank(0.07, N), nearest_rank(0.5, N)
        # ranks 1..r07-1 end with thread 36's chunk (its last bin), so rank r07 = excl + 1 of thread
        # 37's; thread 37's first bin ends at rank r50 = excl + local (empty chunks follow); the rest
        # is the last bin
        ops.append(("bins", s, {c0 - 1: r07 - 1, c0: r50 - (r07 - 1), nb - 1: N - r50}))
    # N = 6: the median, rank 3, is the last rank of thread 5's chunk; N = 7: rank 4 = excl + 1 of thread 6's
    ops.append(("bins", 6, {5 * chunk + chunk - 1: 3, 6 * chunk: 3}))
    ops.append(("bins", 7, {5 * chunk + chunk - 1: 3, 6 * chunk: 4}))
    ops.append(("bins", 8, {2 * chunk: M32, 100: M32, nb - 2: M32}))  # N = 3 (2^32 - 1)
    return _rt_case(f"queries_m{m}", 9, 4, m, 1, ops)


def _register_sum_cases():
    out = []
    for p in (4, 14, 16):
        out.append(_rt_case(f"register_sum_p{p}", 2, p, 7, 0, [("regs", 0, 0), ("regs", 1, 64 - p + 1)]))
    return out


@functools.lru_cache(maxsize=None)
def rt_cases() -> tuple:
    return tuple([_register_case(p) for p in (4, 14, 16)] + [_duration_case(m) for m in (2, 7, 8)]
                 + [_query_case(m) for m in (2, 7, 8)] + _register_sum_cases())


def rt_case(name: str) -> dict:
    return next(c for c in rt_cases() if c["name"] == name)


def apply_rt_ref(ref: RtRef, op) -> None:
    if op[0] == "acc":
        ref.accumulate(op[1], op[2], op[3])
    elif op[0] == "regs":
        ref.regs[op[1]] = [op[2]] * (1 << ref.p)
    elif op[0] == "bins":
        for b, c in op[2].items():
            ref.bins[op[1]][b] = c
    else:
        raise ValueError(op[0])


def run_rt_ref(case: dict) -> RtRef:
    ref = RtRef(**case["cfg"])
    for op in case["ops"]:
        apply_rt_ref(ref, op)
    return ref


def chunk_edge_ranks(bins, qs=QS) -> int:
    """How many of the ranks asked for lie on an edge of a k_rt_query thread's chunk of bins: the first
    rank of a chunk after other mass (excl + 1, excl > 0) or the last of a chunk (excl + local)."""
    nb, n = len(bins), sum(bins)
    if n == 0:
        return 0
    chunk = -(-nb // RT_QUERY_WG)
    firsts, lasts, cum = set(), set(), 0
    for t in range(0, nb, chunk):
        local = sum(bins[t: t + chunk])
        if local:
            if cum:
                firsts.add(cum + 1)
            lasts.add(cum + local)
        cum += local
    lasts.discard(n)  # the last rank of all is on no inner edge
    return sum(1 for q in qs if nearest_rank(q, n) in firsts | lasts)


def classify_rt(case: dict) -> set:
    cfg = case["cfg"]
    p, m, R, nb = cfg["p"], cfg["m"], 1 << cfg["p"], rt_nbins(cfg["m"])
    ref = RtRef(**cfg)
    out: set = set()
    for op in case["ops"]:
        before = [list(r) for r in ref.regs] if op[0] == "acc" else None
        if op[0] == "acc":
            per_word: dict = {}
            runs = Counter()
            for s, t, d in zip(op[1].tolist(), op[2].tolist(), op[3].tolist()):
                if s >= cfg["S"]:
                    continue
                if d < 0 or d > DMAX:
                    out.add("duration_dropped")
                    continue
                runs[s] += 1
                i, rho = hll_fields(t, p, cfg["seed"])
                per_word.setdefault((s, i >> 2), []).append((i & 3, rho))
                out.update(n for n, c in (("rho_max", rho == 64 - p + 1), ("rho==64-p", rho == 64 - p), ("rho==1", rho == 1),
                                          ("idx_first", i == 0), ("idx_last", i == R - 1)) if c)
                b = bin_of(d, m)
                out.update(n for n, c in (("bin_first", b == 0), ("bin_last", b == nb - 1), ("duration_max", d == DMAX),
                                          ("duration>=2^24", d >= 1 << 24)) if c)
                if d >= 1 << 24 and any((d + x) & (d + x - 1) == 0 for x in (-1, 0, 1)):
                    out.add("duration_at_power_of_two>=2^24")
            for (s, w), hits in per_word.items():
                top = {}
                for byte, rho in hits:
                    top[byte] = max(top.get(byte, 0), rho)
                if len(top) == 4 and len(set(top.values())) == 4:
                    out.add("word_four_values")
                if len(hits) >= 64:
                    out.add("word_hit_by_a_wave")
                if len(hits) >= 256:
                    out.add("word_hit_by_a_workgroup")
                old = before[s][4 * w: 4 * w + 4]
                raised = [b for b, r in top.items() if r > old[b]]
                kept = [b for b, r in top.items() if 0 < r <= old[b]]
                if any(old) and raised and kept:
                    out.add("word_one_byte_raised")
            if any(n == RT_UNIT + 1 for n in runs.values()):
                out.add("run==unit+1")
        apply_rt_ref(ref, op)
        if op[0] == "regs":
            out.add("regs_all_zero" if op[2] == 0 else "regs_all_max" if op[2] == 64 - p + 1 else "regs_written")
        if op[0] == "bins":
            bins = ref.bins[op[1]]
            n = sum(bins)
            if n and bins[0] == n:
                out.add("all_in_first_bin")
            if n and bins[-1] == n:
                out.add("all_in_last_bin")
            if n >> 32:
                out.add("count>2^32")
            out.add("count_odd" if n & 1 else "count_even")
            if chunk_edge_ranks(bins):
                out.add("rank_on_chunk_edge")
            out.add(f"bins_per_thread=={-(-nb // RT_QUERY_WG)}")
            if nb < RT_QUERY_WG:
                out.add("threads_without_bins")
    return out


RT_CLASSES = (
    "rho_max", "rho==64-p", "rho==1", "idx_first", "idx_last", "word_four_values", "word_hit_by_a_wave",
    "word_hit_by_a_workgroup", "word_one_byte_raised", "run==unit+1", "bin_first", "bin_last", "duration_max",
    "duration>=2^24", "duration_at_power_of_two>=2^24", "duration_dropped", "regs_all_zero", "regs_all_max",
    "all_in_first_bin", "all_in_last_bin", "count>2^32", "count_odd", "count_even", "rank_on_chunk_edge",
    "bins_per_thread==1", "bins_per_thread==33", "threads_without_bins",
)
