"""CPU checks of what the large-offset and special-value GPU tests stand on (tests/test_gpu_table_large.py,
tests/test_gpu_table_acc.py): the closed form that homes an mbits at a given slot, the slots chosen around
bytes 2^31 and 2^32 of a table's buffer, the wrap cluster's predicted slots, and the any-order expectation of
the double accumulate on NaN, infinities, overflowing sums and subnormals -- checked against exact arithmetic
and against random sequential and tree orders of the additions.  No GPU, no library call."""
import math
import random
from fractions import Fraction

import numpy as np
import pytest

pytest.importorskip("torch")
import table_iter_ref as IT  # noqa: E402
import table_ref as R  # noqa: E402
import test_gpu_table_acc as ACC  # noqa: E402
import test_gpu_table_large as L  # noqa: E402


# ------------------------------------------------------------ homes ---
@pytest.mark.parametrize("C", [64, 1 << 20, 1 << 31])
def test_mbits_for_slot_is_home_high_inverted(C):
    rng = random.Random(C)
    k = R.log2_capacity(C)
    slots = [0, 1, 2, C // 2, C - 2, C - 1] + [rng.randrange(C) for _ in range(300)]
    if C == L.LARGE_C:
        for B in L.LARGE_B:
            named, spread = L.chosen_homes(C, B)
            slots += named + spread + [s for w in range(3) for s in L.created_homes(C, B, w)]
    seen = set()
    for s in slots:
        for low in (0, 1, 0x7777, (1 << (64 - k)) - 1, rng.randrange(1 << (64 - k))):
            mb = L.mbits_for_slot(s, C, low)
            assert 0 <= mb < 1 << 64 and R.home_high(mb, C) == s
            assert (mb * R.MIX) & L.M64 == (s << (64 - k)) | low
            seen.add((s, low, mb))
    assert len({mb for _, _, mb in seen}) == len({(s, low) for s, low, _ in seen})  # a bijection


@pytest.mark.parametrize("B", L.LARGE_B)
def test_chosen_slots_hold_bytes_2_31_and_2_32(B):
    C = L.LARGE_C
    tags, win, rows, end = IT.layout(C, B)
    assert end == 64 + (C + 1) * (16 + B) and end > 1 << 33
    named, spread = L.chosen_homes(C, B)
    for byte, s in ((1 << 31, named[2]), (1 << 32, named[5])):
        assert rows + s * B <= byte < rows + (s + 1) * B
        assert named[named.index(s) - 1] == s - 1 and named[named.index(s) + 1] == s + 1
    assert rows + (named[5] + 1) * B > 1 << 32 and rows + named[4] * B < 1 << 32  # one neighbour on either side
    assert named[0] == 0 and named[-1] == C - 2 and all(s >= C // 2 for s in spread) and len(spread) >= 30
    assert rows + C * B > 2 * (1 << 32)  # mbits 0's private slot: the highest offset of all, past 8 GiB


@pytest.mark.parametrize("B", L.LARGE_B)
def test_predicted_slots_equal_probe_model(B):
    """The slot the GPU test expects of every mbits, against sequential linear probing in the order of its calls:
    the first batch (any order inside it: its homes are distinct and apart), the three wrap mbits one by one,
    then the entries the inserting calls create."""
    C = L.LARGE_C
    main, wrap, slot_of = L.large_keys(C, B)
    created = [L.mbits_for_slot(s, C, low) for w, low in ((0, 0x2000), (1, 0x2001), (2, 0x3000))
               for s in L.created_homes(C, B, w)]
    want = {k: s for k, s in zip(created, [s for w in range(3) for s in L.created_homes(C, B, w)])}
    want.update(slot_of)
    for seed in range(3):
        order = np.random.default_rng(seed).permutation(len(main))
        seq = [int(k) for k in main[order]] + [int(k) for k in wrap] + created
        slots, cost = R.probe_model(seq, C)
        assert {k: int(s) for k, s in zip(seq, slots)} == want
        assert [int(s) for s in slots[len(main):len(main) + 3]] == [C - 1, 1, 2]
        assert [int(c) for c in cost[len(main):len(main) + 3]] == [1, 3, 4]
    assert len(set(want.values())) == len(want) == len(main) + 3 + 12
    below = L.below(want, C)
    assert not set(below.tolist()) & set(want) and len(set(below.tolist())) == len(want) - 1  # 0 and C share C - 1
    assert {R.home_high(int(k), C) for k in below} == {(s - 1) % C for s in want.values()}


# --------------------------------------------------- special values ---
def reduce_in_order(xs, rng, tree):
    """xs added up as IEEE doubles: in a random sequential order, or as a random binary tree."""
    xs = [np.float64(x) for x in xs]
    rng.shuffle(xs)
    with np.errstate(all="ignore"):
        if not tree:
            s = xs[0]
            for x in xs[1:]:
                s = s + x
            return float(s)
        while len(xs) > 1:
            a = xs.pop(rng.randrange(len(xs)))
            b = xs.pop(rng.randrange(len(xs)))
            xs.append(a + b)
    return float(xs[0])


def same(a, b):
    return math.isnan(b) if math.isnan(a) else np.float64(a).tobytes() == np.float64(b).tobytes()


@pytest.mark.parametrize("rule", ACC.SPECIAL_RULES)
def test_special_expectations_hold_in_any_order(rule):
    """special_expect on every input set of the GPU test: equal to the exact sum (fractions) where that is
    finite and the rule says "exact", and to three random sequential and three random tree orders of IEEE
    additions everywhere -- the expectations do not depend on the order."""
    rng = random.Random(ACC.SPECIAL_RULES.index(rule))
    seen = {"nan": 0, "inf": 0, "zero": 0, "normal_from_sub": 0, "sub": 0, "ordinary": 0}
    for B, vo, elems in ACC.SPECIAL_REGIONS:
        for shape in ACC.SPECIAL_SHAPES:
            for insert in (False, True):
                held, old, absent, mb, add, rule_of = ACC.special_batch(rule, shape, elems, insert)
                words = ACC.special_words(held, old, mb, add, insert)
                assert set(words) == set(rule_of)
                assert len(add) == len(mb) and add.shape[1] == elems and held[0] == 0
                for key, xs in words.items():
                    want = ACC.special_expect(xs)
                    if all(math.isfinite(x) for x in xs) and math.isfinite(want):
                        exact = sum(Fraction(x) for x in xs)
                        assert Fraction(want) == exact and (want != 0 or math.copysign(1.0, want) > 0)
                    for tree in (False, True):
                        for _ in range(3):
                            got = reduce_in_order(xs, rng, tree)
                            assert same(want, got), (rule, shape, insert, key, xs[:4], want, got)
                    if rule_of[key] == "ordinary":
                        assert math.isfinite(want) and float(want).is_integer() and abs(want) < 2 ** 53
                        seen["ordinary"] += 1
                    else:
                        tiny = all(abs(x) < 2.0 ** -1000 for x in xs)
                        seen["nan"] += math.isnan(want)
                        seen["inf"] += math.isinf(want)
                        seen["zero"] += tiny and want == 0 and len(xs) > 1 and any(x != 0 for x in xs)
                        seen["normal_from_sub"] += tiny and want >= 2.0 ** -1022 and xs[1] < 2.0 ** -1022
                        seen["sub"] += tiny and 0 < abs(want) < 2.0 ** -1022
    assert seen["ordinary"] > 100
    need = {"nan": ["nan"], "pinf": ["inf"], "ninf": ["inf"], "both": ["nan", "inf"], "overflow": ["inf"],
            "sub": ["sub"], "sub_zero": ["zero", "sub"], "sub_cross": ["normal_from_sub"]}[rule]
    assert all(seen[k] > 10 for k in need), seen


def test_special_expect_refuses_what_depends_on_the_order():
    for xs in ([1e308, 1e308, -1e308], [1.0, 2.0 ** -60, -1.0], [-0.0, -0.0], [0.1, 0.2, 0.3],
               [1.7e308, 1e292]):  # cancels or not; rounds; the sign of zero; rounds; overflows or not
        with pytest.raises(ValueError):
            ACC.special_expect(xs)
    assert ACC.special_expect([0.0, 1e308]) == 1e308 and ACC.special_expect([1e308] * 2) == math.inf
    assert ACC.special_expect([-1e308] * 3) == -math.inf and ACC.special_expect([0.0, 0.0]) == 0.0
    assert ACC.special_expect([5e-324, -5e-324]) == 0.0 and math.copysign(1.0, ACC.special_expect([5e-324, -5e-324])) > 0
    assert ACC.special_expect([2.0 ** -1023, 2.0 ** -1023]) == 2.0 ** -1022
    assert math.isnan(ACC.special_expect([math.inf, 1.0, -math.inf])) and math.isnan(ACC.special_expect([math.nan, math.inf]))
