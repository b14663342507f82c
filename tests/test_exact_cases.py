"""The case list of tests/exactref.py reaches what the device tests need it to reach -- every
rounding class of k_finalize's div_round, negative numerators, its right-shift path, numerators up
to the width the 384-bit arithmetic was chosen for -- and the host views of the table
(zipkin_amd/table.py) agree with the exact sums on every case. All of it from the reference alone:
no device, no oracle."""
from collections import Counter
from fractions import Fraction

import numpy as np

from tests import exactref
from tests.exactref import CONSTRUCTED, DMAX, NMAX, classes, classify, finalize_cases, numerators, power_sums
from zipkin_amd import table

S = 64


def test_classify_on_hand_made_quotients():
    assert classify(0, 7) == ("zero", False, False)
    assert classify(-3, 1) == ("exact", True, False)
    assert classify((1 << 54) + 2, 1)[0] == "tie_even"  # mantissa 2^52, f = 1/2
    assert classify((1 << 54) + 6, 1)[0] == "tie_odd"
    assert classify(((1 << 53) + 1) * 3, 3 << 1)[0] == "tie_even"
    assert classify((1 << 64) + (1 << 11) + 1, 1)[0] == "just_above_tie"
    assert classify((1 << 64) + (1 << 11) - 1, 1)[0] == "just_below_tie"
    assert classify((1 << 64) - 1, 1)[0] == "carry"
    assert classify(1, 3)[0] == "plain"
    assert classify(1 << 200, 3) == ("plain", False, True)
    assert classify(-(1 << 60), 3) == ("plain", True, True)  # 61 - 2 = 59 > 58
    assert classify(-(1 << 59), 3)[2] is False  # 60 - 2 = 58: the left-shift path (s = 0)


def test_constructed_cases_hit_their_class():
    by = dict(CONSTRUCTED)
    assert classes(by["tie_even_m1"])[0][0] == "tie_even"
    assert classes(by["tie_odd_m1"])[0][0] == "tie_odd"
    assert classes(by["carry_m1"])[0][0] == "carry"
    assert exactref.moments(by["cancel_at_top"]) == (NMAX, float(DMAX), 0.0, 0.0, 0.0)
    assert [c[0] for c in classes(by["cancel_at_top"])[1:]] == ["zero"] * 3
    assert [abs(A).bit_length() for A, _ in numerators(by["largest_numerators"])] == [71, 142, 182, 284]
    assert numerators(by["left_skewed"])[2][0] < 0
    assert numerators(by["symmetric"])[2][0] == 0 and numerators(by["symmetric"])[1][0] > 0
    assert exactref.moments(by["one_at_zero"]) == (1, 0.0, 0.0, 0.0, 0.0)
    assert exactref.moments(by["one_at_top"]) == (1, float(DMAX), 0.0, 0.0, 0.0)
    # the rounded moments are those of the ties' definitions
    n, s1 = power_sums(by["tie_even_m1"])[:2]
    assert Fraction(s1, n) == (1 << 33) + Fraction(1, 1 << 20) and float(Fraction(s1, n)) == float(1 << 33)
    n, s1 = power_sums(by["tie_odd_m1"])[:2]
    assert float(Fraction(s1, n)) == float((1 << 33) + 4 * 2.0 ** -20)  # 3 ulps (2^-20) rounds to 4


def test_case_list_reaches_every_finalize_path():
    cases = finalize_cases()
    assert len(cases) == S * S
    seen = Counter()
    negative = right = largest = 0
    for _, ms in cases:
        assert all(0 <= d <= DMAX and c >= 1 for d, c in ms) and sum(c for _, c in ms) <= NMAX
        for (cls, neg, rs), (A, _) in zip(classes(ms), numerators(ms)):
            seen[cls] += 1
            negative += neg
            right += rs
            largest = max(largest, abs(A).bit_length())
    print(dict(seen), "negative", negative, "right_shift", right, "largest numerator bits", largest)
    for cls in ("tie_even", "tie_odd", "carry", "zero"):
        assert seen[cls] >= 1, cls
    assert seen["just_above_tie"] >= 5 and seen["just_below_tie"] >= 5
    assert negative >= 500 and right >= 1000
    assert 280 <= largest < 300


def test_host_table_views_agree_with_the_exact_sums():
    cases = finalize_cases()
    want = {(i // S, i % S): power_sums(ms) for i, (_, ms) in enumerate(cases)}
    acc = table.encode(want, S)
    assert table.decode(acc, S) == want
    x = table.pack(acc, S)
    assert table.decode_exchange(x, S) == want
    assert np.array_equal(x, table.encode_exchange(want, S))
    assert np.array_equal(table.unpack(x, S), acc)


def test_worst_flush_cell_decodes_and_packs_exactly():
    limbs, sums = exactref.worst_flush_cell()
    assert sums[0] == NMAX and sums[4] == NMAX * DMAX ** 4
    # every limb of a sum but its top one holds (a 32-bit chunk) x (2^32 - 1)
    for off, k in table.POWER_LIMBS:
        assert all(limbs[off + i] % NMAX == 0 and limbs[off + i] // NMAX < 1 << 32 for i in range(k))
    assert max(limbs) > (1 << 64) - (1 << 34)
    assert table.decode_cell(limbs) == sums
    acc = np.zeros(2 * 2 * table.LIMBS + table.TAIL, np.uint64)
    acc[3 * table.LIMBS: 4 * table.LIMBS] = np.array(limbs, np.uint64)
    acc = acc.view(np.int64)
    assert table.decode(acc, 2) == {(1, 1): sums}
    x = table.pack(acc, 2)
    assert table.decode_exchange(x, 2) == {(1, 1): sums}
    assert np.array_equal(x, table.encode_exchange({(1, 1): sums}, 2))
    # the exchange limbs leave room for 256 ranks
    assert all(int(v) <= (1 << 56) - 1 for v in x.view(np.uint64))
    assert table.decode(table.unpack(x, 2), 2) == {(1, 1): sums}
