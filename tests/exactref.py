"""TEST INFRASTRUCTURE ONLY -- an exact reference for the link table at the bounds of its domain.

Python integers and fractions.Fraction only: nothing here imports zipkin_amd or calls the C oracle,
so it is independent of both. A cell's content is a multiset of durations, a list of
(duration, count) pairs; its power sums are exact ints, its expected moments are
oracle.moments.moments_from_power_sums (Fraction -> float, correctly rounded), and `classify` says
from the mathematics of the inputs alone which rounding path of k_finalize's div_round
(zipkin_amd/csrc/zk_finalize.hip) a moment must take."""
from __future__ import annotations

import random

from oracle.moments import moments_from_power_sums
from tests.test_reduce_bounds import flush, rows_of

DMAX = (1 << 40) - 1  # the largest accepted duration (kMaxDuration - 1)
NMAX = (1 << 32) - 1  # the most records since reset (kMaxRecordsSinceReset)

# every reducer and emitter case carries these durations: both sides of 2^21 (the wide kernel's
# packed-word branch), of 2^32 (RunSums::add_small / add) and the top of the range
EDGE_DURATIONS = (0, 1, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 7, DMAX - 1, DMAX)


def power_sums(ms):
    """(n, S1, S2, S3, S4) of a multiset [(duration, count), ...] as exact ints."""
    n = sum(c for _, c in ms)
    return (n, *(sum(c * d ** k for d, c in ms) for k in (1, 2, 3, 4)))


def moments(ms):
    """(m0, m1..m4): the exact moments rounded once."""
    return tuple(moments_from_power_sums(*power_sums(ms)))


def numerators(ms):
    """[(A, D)] of m1..m4 exactly as k_finalize forms them (not reduced to lowest terms)."""
    n, s1, s2, s3, s4 = power_sums(ms)
    return [(s1, n),
            (n * s2 - s1 * s1, n),
            (n * n * s3 - 3 * n * s1 * s2 + 2 * s1 ** 3, n * n),
            (n ** 3 * s4 - 4 * n * n * s1 * s3 + 6 * n * s1 * s1 * s2 - 3 * s1 ** 4, n ** 3)]


def classify(A: int, D: int):
    """-> (class, negative, right_shift) of the quotient A / D (D > 0).

    |A| / D is scaled to a 53-bit mantissa plus a fraction f in [0, 1), in integers. class is one
    of zero, exact (f = 0), tie_even / tie_odd (f = 1/2, by the mantissa's last bit),
    just_above_tie (0 < f - 1/2 <= 2^-10), just_below_tie (0 < 1/2 - f <= 2^-10), carry (f > 1/2
    with mantissa 2^53 - 1: rounding up carries into the exponent) or plain. right_shift says
    bitlen(|A|) - bitlen(D) > 58: the scaling shift of div_round is negative there."""
    assert D > 0
    neg, a = A < 0, abs(A)
    if a == 0:
        return "zero", False, False
    right = a.bit_length() - D.bit_length() > 58
    e = a.bit_length() - D.bit_length() - 53
    while True:
        num, den = (a, D << e) if e >= 0 else (a << -e, D)
        mant, rem = divmod(num, den)
        if mant >> 53:
            e += 1
        elif not mant >> 52:
            e -= 1
        else:
            break
    if rem == 0:
        cls = "exact"
    elif 2 * rem == den:
        cls = "tie_odd" if mant & 1 else "tie_even"
    elif 0 < 2 * rem - den and (2 * rem - den) * 512 <= den:
        cls = "just_above_tie"
    elif 0 < den - 2 * rem and (den - 2 * rem) * 512 <= den:
        cls = "just_below_tie"
    elif 2 * rem > den and mant == (1 << 53) - 1:
        cls = "carry"
    else:
        cls = "plain"
    return cls, neg, right


def classes(ms):
    """classify() of m1..m4."""
    return [classify(A, D) for A, D in numerators(ms)]


CONSTRUCTED = (
    ("tie_even_m1", [(1 << 33, (1 << 20) - 1), ((1 << 33) + 1, 1)]),
    ("tie_odd_m1", [(1 << 33, (1 << 20) - 3), ((1 << 33) + 1, 3)]),
    ("carry_m1", [(1 << 39, (1 << 20) - 1), ((1 << 39) - 1, 1)]),
    ("cancel_at_top", [(DMAX, NMAX)]),
    ("largest_numerators", [(0, 1 << 31), (DMAX, (1 << 31) - 1)]),
    ("tiny_spread_huge_mean", [(DMAX - 1, 1), (DMAX, 2)]),
    ("one_at_zero", [(0, 1)]),
    ("one_at_top", [(DMAX, 1)]),
    ("left_skewed", [(5, 1), (DMAX - 3, 1000), (DMAX, 999)]),  # m3 < 0
    ("symmetric", [(1 << 32, 7), ((1 << 32) + 1000, 11), ((1 << 32) + 2000, 7)]),  # m3 = 0
)
RANDOM_SEED = 20261
TABLE_CELLS = 64 * 64


def _random_multiset(rng):
    while True:
        ms = []
        for _ in range(rng.randint(1, 4)):
            d = rng.randrange(1 << rng.choice((21, 32, 40)))
            kind = rng.randrange(7)
            if kind < 3:
                c = kind + 1
            elif kind == 3:
                c = rng.randrange(1, 1 << 10)
            elif kind == 4:
                c = rng.randrange(1, 1 << 20)
            elif kind == 5:
                c = 1 << rng.randrange(0, 31)
            else:
                c = rng.randrange(1, 1 << 30)
            ms.append((d, c))
        if sum(c for _, c in ms) <= NMAX:
            return ms


_CASES = None


def finalize_cases():
    """[(name, multiset)]: the constructed cases, then a seeded random family that fills a
    64 x 64 table (4096 cells in all). Every value is < 2^40, every total < 2^32."""
    global _CASES
    if _CASES is None:
        rng = random.Random(RANDOM_SEED)
        cases = list(CONSTRUCTED)
        while len(cases) < TABLE_CELLS:
            cases.append((f"random_{len(cases)}", _random_multiset(rng)))
        _CASES = cases
    return _CASES


def multiset(durations):
    """[(duration, count)] of an iterable (or numpy array) of durations."""
    if hasattr(durations, "dtype"):
        import numpy as np

        values, counts = np.unique(durations, return_counts=True)
        return [(int(v), int(c)) for v, c in zip(values, counts)]
    out = {}
    for d in durations:
        out[int(d)] = out.get(int(d), 0) + 1
    return sorted(out.items())


def assert_moments(got, cells, S):
    """A finalized table (arrays m0..m4 and present over S * S cells) equals the correctly rounded
    moments of `cells` = {(parent, child): multiset} bit for bit, and every other cell is absent. A
    failure names the cell, the class of the moment that differs and both values."""
    import numpy as np

    m0 = np.asarray(got.m0).astype(np.uint64)
    ms = [np.asarray(getattr(got, k)).view(np.uint64) for k in ("m1", "m2", "m3", "m4")]
    present = np.asarray(got.present)
    want_present = np.zeros(S * S, np.uint8)
    for (p, c), m in cells.items():
        i = p * S + c
        want = moments(m)
        want_present[i] = 1
        assert int(m0[i]) == want[0], f"cell ({p}, {c}): m0 {int(m0[i])} != {want[0]}"
        for k in range(4):
            w = np.float64(want[k + 1]).view(np.uint64)
            if ms[k][i] != w:
                A, D = numerators(m)[k]
                raise AssertionError(f"cell ({p}, {c}) m{k + 1}: class {classify(A, D)}, device "
                                     f"{ms[k][i].view(np.float64)!r} != exact {want[k + 1]!r} (multiset {m})")
    assert np.array_equal(present, want_present), "the set of present cells differs"
    empty = want_present == 0
    assert not m0[empty].any() and not any(a[empty].any() for a in ms), "an absent cell holds a value"


def worst_flush_cell():
    """(16 limbs, (n, S1..S4)): the accumulator cell after 2^32 - 1 links of 2^40 - 1, each in a
    flush of its own -- every limb of a sum but its top one is (a 32-bit chunk) x (2^32 - 1), near
    2^64, the largest state the carry-free layout has to hold."""
    _, _, one = flush(rows_of([DMAX]))
    limbs = [x * NMAX for x in one] + [0]
    assert all(x < 1 << 64 for x in limbs)
    return limbs, power_sums([(DMAX, NMAX)])
