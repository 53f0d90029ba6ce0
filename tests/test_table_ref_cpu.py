"""The references of tests/table_ref.py, proved on the CPU before tests/test_gpu_table_edges.py relies on
them: the probe model against a plain slot-by-slot walk, what of it depends on the insertion order (which
a GPU's schedule decides) and what does not, the vectorised last-writer table against the dict model of
tests/test_gpu_table.py, and that a home taken from the wrong bits would show in the counts."""
import numpy as np
import pytest

import table_ref as R
from test_gpu_table import ALL_ONES, Model, distinct_mbits, rows_for, splitmix64


def structured_mbits(kind, n=32768):
    """The mbits of test_structured_mbits_keep_probes_short: keys that share their low bits."""
    i = np.arange(n, dtype=np.uint64)
    if kind == "low16":
        mb = (splitmix64(i) << np.uint64(16)) | np.uint64(0x1234)
    else:
        mb = (splitmix64(i) >> np.uint64(12)) * np.uint64(1024) + np.uint64(5)
    assert len(np.unique(mb)) == n
    return mb


def test_home_is_the_high_bits_of_the_mix():
    for mb in (1, 2, 0x1234567890ABCDEF, ALL_ONES):
        for k in (6, 16, 31):
            want = int(((np.array([mb], np.uint64) * np.uint64(R.MIX)) >> np.uint64(64 - k))[0])  # wraps mod 2^64
            assert R.home_high(mb, 1 << k) == want < 1 << k


@pytest.mark.parametrize("C,n", [(64, 64), (64, 50), (4096, 3000)])
def test_probe_model_is_the_plain_walk(C, n):
    mb = distinct_mbits(n, 40)
    rng = np.random.default_rng(C + n)
    seq = np.concatenate([mb, rng.choice(mb, 100), np.zeros(3, np.uint64)])[rng.permutation(n + 103)]
    for home in (R.home_high, R.home_low):
        s0, c0 = R.probe_walk(seq, C, home)
        s1, c1 = R.probe_model(seq, C, home)
        assert (s0 == s1).all() and (c0 == c1).all()
        zero = seq == 0
        assert (s1[zero] == C).all() and (c1[zero] == 1).all() and (s1[~zero] < C).all()
        # an entry sits at home + displacement on the ring, with no free slot in between
        homes = np.array([home(int(x), C) for x in seq[~zero]])
        assert (((homes + c1[~zero] - 1) & (C - 1)) == s1[~zero]).all()
        occ = np.zeros(C, bool)
        occ[s1[~zero]] = True
        for h, c in zip(homes, c1[~zero]):
            assert occ[(h + np.arange(c)) & (C - 1)].all()


@pytest.mark.parametrize("C,n", [(64, 64), (64, 50), (4096, 3000), (65536, 32768)])
def test_order_independence(C, n):
    """Whatever order the keys arrive in -- on the GPU the schedule decides it -- linear probing occupies the
    same slots and inspects the same total number of them, cluster by cluster.  Where inside its cluster
    one key lands is NOT independent of the order (asserted too: it is why the exact-count GPU test sends
    whole clusters)."""
    mb = distinct_mbits(n, 40)
    seen = []
    for seed in range(4):
        order = np.arange(n) if seed == 0 else np.random.default_rng(seed).permutation(n)
        slots, cost = R.probe_model(mb[order], C)
        back = np.empty(n, np.int64)
        back[order] = np.arange(n)
        slots, cost = slots[back], cost[back]  # per key, in mb's order
        lab, ncl = R.clusters(slots, C)
        # name a cluster by its smallest key index: labels depend on nothing but the occupied set anyway
        per_cluster = np.bincount(lab, weights=cost, minlength=ncl).astype(np.int64)
        seen.append((int(cost.sum()), np.sort(slots), lab, per_cluster, slots))
    print(f"C {C} n {n}: {seen[0][0]} slots inspected in all, {len(seen[0][3])} clusters")
    for total, occ, lab, per_cluster, _ in seen[1:]:
        assert total == seen[0][0]
        assert (occ == seen[0][1]).all()
        assert (lab == seen[0][2]).all()  # the same keys share a cluster
        assert (per_cluster == seen[0][3]).all()
    assert any((s[4] != seen[0][4]).any() for s in seen[1:])  # single keys do move


def test_clusters():
    lab, n = R.clusters([62, 63, 0, 1, 5, 9, 10, 64], 64)  # the run 62..1 wraps; 64 is mbits 0's slot
    assert n == 3 and lab[7] == -1
    assert lab[0] == lab[1] == lab[2] == lab[3] and lab[5] == lab[6]
    assert len({lab[0], lab[4], lab[5]}) == 3
    lab, n = R.clusters(np.arange(64), 64)
    assert n == 1 and (lab == 0).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_put_ref_agrees_with_the_dict_model(seed):
    rng = np.random.default_rng(70 + seed)
    B = (8, 40, 16)[seed]
    pool = np.concatenate([np.array([0, 1, ALL_ONES], np.uint64), distinct_mbits(60, 70 + seed)])
    absent = distinct_mbits(20, 80)
    model, state = Model(1024), None
    for rnd, m in enumerate((1, 0, 300, 63, 4097, 2)):
        mb = rng.choice(pool[:3 + 10 * (rnd + 1)], m)
        if m >= 63:
            mb[:3] = pool[:3]  # the mark values are in
        rows = rows_for(m, B, 90 + rnd + seed)
        status, state = R.put_ref(mb, rows, state)
        assert (status == model.put(mb, rows)).all()
        assert (state[0][1:] > state[0][:-1]).all() and len(state[0]) == len(model.d)
        q = np.concatenate([pool, absent, rng.choice(pool, 50)])
        for head in (1, 8):
            assert (R.replies_ref(state, q, head, B) == model.replies(q, head, B)).all()
    assert {0, 1, ALL_ONES} <= set(model.d)


@pytest.mark.parametrize("kind", ["low16", "mod1024"])
def test_home_from_the_high_bits(kind):
    """At load 0.5 the mix's high bits inspect fewer than 2 slots per record for keys that share their low
    bits; homes from the low bits inspect more than 100.  So the equality that the GPU test asserts on the
    table's counter tells the two apart."""
    mb = structured_mbits(kind)
    high = R.probe_model(mb, 65536)[1].mean()
    low = R.probe_model(mb, 65536, R.home_low)[1].mean()
    print(f"{kind}: {high:.3f} slots per record from the high bits, {low:.1f} from the low bits")
    assert high < 2
    assert low > 100
