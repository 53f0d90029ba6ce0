"""GPU checks of the table's update, insert-if-absent and compare-and-swap by key
(include/pdht_hip_table_keys_rmw.h).  The oracle is the record route at one rank on a twin table, which this
project's other suites pin -- bucket_put_records(nranks=1) -> update_records / add_records, bucket_records
(nranks=1) -> cswap -- beside the sequential models update_ref, cswap_ref and add_ref on a dict state and the
oracle's CityHash64.  Tables are compared by their entries (mbits -> row), never by storage image: the slot
order inside a cluster may differ between two inserting runs.  Every comparison is byte for byte."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

import table_add_ref as A  # noqa: E402
import table_rmw_ref as M  # noqa: E402
from test_gpu_table import to_dev  # noqa: E402
from test_gpu_table_keys import (KEYSIZES, NS, SENTINEL, entries_of, keys_at, keys_with_repeats, rows_of,  # noqa: E402
                                 rows_only, rowbytes_of, slot_of, u64, values_at, values_for, walk_cost)

pytestmark = pytest.mark.gpu

UPDATE = "k_table_locate_keys<last>+k_table_write_keys<{}>"
ADD = "k_table_add_claim_keys+k_table_add_write_keys<{}>"
CSWAP = "k_table_locate_keys<first>+k_table_cswap"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------- helpers ---
def piece(B):
    return 16 if B % 16 == 0 else 8


def put_records_of(kd, vd, key_slot=0):
    """The put records of the record route at one rank: record position = key index."""
    rec, offs = P.bucket_put_records(kd.contiguous(), vd, 1, key_slot=key_slot)
    assert offs.cpu().tolist() == [0, kd.shape[0]]
    return rec


def state_rows(tab):
    return rows_only(entries_of(tab))


def state_bytes(state):
    return {k: np.asarray(r, np.uint8).tobytes() for k, r in state.items()}


def twins(dev, C, B, keys, vals, key_slot=0):
    """Two tables filled alike through the record route, and the dict state of the models."""
    ta, tb = P.DeviceTable(C, B, dev), P.DeviceTable(C, B, dev)
    state = {}
    if len(keys):
        rec = put_records_of(keys_at(keys, dev), to_dev(vals, dev), key_slot)
        assert (ta.put_records(rec) != 2).all() and (tb.put_records(rec) != 2).all()
        state = {k: np.frombuffer(r, np.uint8).copy() for k, r in state_rows(ta).items()}
    return ta, tb, state


def word_of(row, offset):
    return int(np.frombuffer(bytes(row[offset:offset + 8]), np.uint64)[0])


def same_tables(ta, tb, state, moved=None):
    """Entries of both tables equal the state; counts()[:3] agree (and [0], [1], [3] stayed when `moved`
    gives the counts before a call that may only take a batch number)."""
    ea = state_rows(ta)
    assert ea == state_rows(tb) == state_bytes(state)
    assert ta.counts()[:3] == tb.counts()[:3]
    if moved is not None:
        now = ta.counts()
        assert (now[0], now[1], now[3]) == (moved[0], moved[1], moved[3]) and now[2] == moved[2] + 1


# ------------------------------------------------- 1. parity with the record route ---
@pytest.mark.parametrize("E", [1, 8, 24])
@pytest.mark.parametrize("L", KEYSIZES)
def test_keyed_writes_equal_the_record_route(dev, oracle, L, E):
    """Table A by the keyed calls, table B by the record route, both pre-filled with every second key of the
    batch, so that a not-found (update, cswap) and an exists (add) stand in every wave: update_keys, then
    cswap_keys on the first word of the value, then add_keys on what is now a half-filled table, and add_keys
    on an empty pair.  Status, replies, mbits_out, counts()[:3], the entries and the kernel's name are
    checked, the entries and status also against the sequential models.  Keys from an aligned base (the
    vector classes of 8 / 16 / 32 / 64 bytes), from byte offset 1 and from byte offset 8; values in the three
    layouts."""
    C = 2048
    for key_slot in (0, 32, 64):
        if key_slot and key_slot < L:
            continue
        B, slot = rowbytes_of(L, E, key_slot), slot_of(L, key_slot)
        for n in NS:
            for off, layout in ((0, "packed"), (1, "odd"), (8, "slice")):
                if n in (63, 65) and off == 8:
                    continue
                keys, vals = keys_with_repeats(n, L, key_slot + off), values_for(n, E, off)
                vals2, vals3 = values_for(n, E, off + 50), values_for(n, E, off + 60)
                kd = keys_at(keys, dev, off)
                want_mb = oracle.city64_fixed(keys)
                ta, tb, state = twins(dev, C, B, keys[::2], vals[::2], key_slot)
                # update
                vd = values_at(vals2, dev, layout)
                before = ta.counts()
                st_a, mb = ta.update_keys(kd, vd, key_slot=key_slot, mbits=True)
                assert P.last_kernel() == UPDATE.format(piece(B))
                st_b = tb.update_records(put_records_of(kd, vd, key_slot))
                assert torch.equal(st_a, st_b) and (u64(mb) == want_mb).all()
                want_st = M.update_ref(state, want_mb, rows_of(keys, vals2, key_slot))
                assert (st_a.cpu().numpy() == want_st).all()
                assert L == 1 or n < 4 or (want_st == 3).any()
                same_tables(ta, tb, state, before)
                # cswap: the word of the first key's row, present after the update
                compare = word_of(state[int(want_mb[0])], slot)
                before = ta.counts()
                ra, mb = ta.cswap_keys(kd, slot, compare, 0x0123456789ABCDEF, mbits=True)
                assert P.last_kernel() == CSWAP
                rb = tb.cswap(P.bucket_records(kd.contiguous(), 1)[0], slot, compare, 0x0123456789ABCDEF)
                assert torch.equal(ra, rb) and (u64(mb) == want_mb).all()
                assert (ra.cpu().numpy() == M.cswap_ref(state, want_mb, slot, compare, 0x0123456789ABCDEF)).all()
                same_tables(ta, tb, state, before)
                # add on the half-filled tables, then on empty ones
                for xa, xb, xstate in ((ta, tb, state), twins(dev, C, B, keys[:0], vals[:0], key_slot)):
                    vd = values_at(vals3, dev, layout)
                    nb = xa.counts()[2]
                    st_a, mb = xa.add_keys(kd, vd, key_slot=key_slot, mbits=True)
                    assert P.last_kernel() == ADD.format(piece(B))
                    st_b = xb.add_records(put_records_of(kd, vd, key_slot))
                    assert torch.equal(st_a, st_b) and (u64(mb) == want_mb).all()
                    want_st, _ = A.add_ref(xstate, want_mb, rows_of(keys, vals3, key_slot), capacity=C)
                    assert (st_a.cpu().numpy() == want_st).all()
                    same_tables(xa, xb, xstate)
                    assert xa.counts()[:3] == (len(xstate), 0, nb + 1)


# ------------------------------------------------------------ 2. order ---
def _order_batches(L):
    rng = np.random.default_rng(L)
    a, b = rng.integers(0, 256, (2, L), dtype=np.uint8)
    one = np.tile(a, (4097, 1))
    two = np.tile(np.stack([a, b]), (700, 1))[:1399]
    tail = rng.integers(0, 256, (128, L), dtype=np.uint8)  # a repeat in the last two lanes of both waves
    tail[62], tail[63], tail[127] = a, a, tail[126]
    return [("one key", one), ("two keys", two), ("wave tail", tail)]


@pytest.mark.parametrize("L", [8, 13])
def test_order_inside_a_batch(dev, oracle, L):
    """One key 4097 times, two keys alternating, and a repeat in a wave's last two lanes: update_keys leaves
    the LAST value of an mbits, add_keys the FIRST, and of cswap_keys' requests the first alone sees
    `compare`; a second cswap_keys with the same pair sees `desired` wherever the first swapped."""
    E, C = 8, 256
    B, slot = rowbytes_of(L, E), slot_of(L)
    for name, keys in _order_batches(L):
        n = len(keys)
        mbits = oracle.city64_fixed(keys)
        first = {int(k): n - 1 - p for p, k in enumerate(mbits[::-1])}
        last = {int(k): p for p, k in enumerate(mbits)}
        vals = np.arange(1, n + 1, dtype=np.uint64).view(np.uint8).reshape(n, 8)  # value = position + 1
        kd, vd = keys_at(keys, dev, 1), to_dev(vals, dev)
        rows = rows_of(keys, vals)
        # add on an empty table: the first
        ta = P.DeviceTable(C, B, dev)
        st = ta.add_keys(kd, vd).cpu().numpy()
        assert sorted(np.flatnonzero(st == 0).tolist()) == sorted(first.values()), name
        assert (st[st != 0] == 4).all()
        assert state_rows(ta) == {k: rows[p].tobytes() for k, p in first.items()}
        state = {k: rows[p].copy() for k, p in first.items()}
        # cswap on the value word with compare = the word of keys[0]'s entry: its first request alone sees it
        compare, desired = first[int(mbits[0])] + 1, 1 << 63
        rep = ta.cswap_keys(kd, slot, compare, desired).cpu().numpy()
        assert (rep == M.cswap_ref(state, mbits, slot, compare, desired)).all(), name
        old = rep[:, 8:].copy().view(np.uint64)[:, 0]
        assert np.flatnonzero(old == compare).tolist() == [first[int(mbits[0])]]
        assert (old[mbits == mbits[0]][1:] == desired).all()
        rep2 = ta.cswap_keys(kd, slot, compare, desired).cpu().numpy()
        assert (rep2 == M.cswap_ref(state, mbits, slot, compare, desired)).all()
        assert (rep2[:, 8:].copy().view(np.uint64)[:, 0][mbits == mbits[0]] == desired).all()
        assert rep2[:, 0].all() and state_rows(ta) == state_bytes(state)
        # update: the last
        st = ta.update_keys(kd, vd).cpu().numpy()
        assert (st == M.update_ref(state, mbits, rows)).all(), name
        assert sorted(np.flatnonzero(st == 0).tolist()) == sorted(last.values()) and (st[st != 0] == 1).all()
        assert state_rows(ta) == {k: rows[p].tobytes() for k, p in last.items()}
        assert ta.counts()[:3] == (len(last), 0, 4)


# ------------------------------------------------------------ 3. counters ---
def test_counters(dev, oracle):
    """update_keys and cswap_keys only take a batch number; an add_keys of keys that are all present inspects
    for each key exactly its displacement + 1, a number no schedule changes."""
    L, E, n, C = 13, 8, 900, 1024
    B = rowbytes_of(L, E)
    keys, vals = keys_with_repeats(n, L, 3), values_for(n, E, 3)
    kd, vd = keys_at(keys, dev, 1), to_dev(vals, dev)
    mbits = oracle.city64_fixed(keys)
    tab = P.DeviceTable(C, B, dev)
    tab.add_keys(kd, vd)
    ent = entries_of(tab)
    c0 = tab.counts()
    assert c0[:3] == (len(set(mbits.tolist())), 0, 1) and c0[3] >= n
    more = np.concatenate([keys, values_for(50, L, 4)])
    tab.update_keys(keys_at(more, dev), to_dev(values_for(n + 50, E, 5), dev))
    c1 = tab.counts()
    assert c1 == (c0[0], c0[1], c0[2] + 1, c0[3])
    tab.cswap_keys(keys_at(more, dev), slot_of(L), 0, 1)
    c2 = tab.counts()
    assert c2 == (c0[0], c0[1], c0[2] + 2, c0[3])
    st = tab.add_keys(kd, vd)
    assert st.eq(4).all()
    c3 = tab.counts()
    assert c3[:3] == (c0[0], c0[1], c0[2] + 3)
    assert c3[3] - c2[3] == walk_cost(ent, mbits, C)


# ------------------------------------------------------------ 4. overflow ---
@pytest.mark.parametrize("L,E", [(13, 8), (32, 24)])
def test_add_keys_overflow(dev, oracle, L, E):
    """Capacity 64: 20 present keys, then a batch of 200 new keys, the present ones and repeats of both: 220
    distinct keys into 64 slots."""
    C, B = 64, rowbytes_of(L, E)
    rng = np.random.default_rng(L)
    pool = np.unique(rng.integers(0, 256, (400, L), dtype=np.uint8), axis=0)
    pool = pool[rng.permutation(len(pool))]
    present, new = pool[:20], pool[20:220]
    tab, _, state = twins(dev, C, B, present, values_for(20, E, 1))
    keys = np.concatenate([new, present, new[:50], present[:10]])
    keys = keys[rng.permutation(len(keys))]
    n = len(keys)
    vals = values_for(n, E, 2)
    mbits = oracle.city64_fixed(keys)
    assert len(np.unique(mbits)) == 220  # no collision among the test's keys
    before = tab.counts()
    st, mb = tab.add_keys(keys_at(keys, dev, 1), to_dev(vals, dev), mbits=True)
    st = st.cpu().numpy()
    assert (u64(mb) == mbits).all()
    after = tab.counts()
    assert set(np.unique(st).tolist()) <= {0, 2, 4}
    was_present = np.isin(mbits, oracle.city64_fixed(present))
    assert (st[was_present] == 4).all()                             # a present key is never dropped
    lost = set(mbits[st == 2].tolist())
    assert not lost & set(mbits[st != 2].tolist())                  # all repeats of a key share its fate
    assert int((st == 0).sum()) + len(lost) == 200                  # created + dropped = distinct new keys
    assert int((st == 2).sum()) == after[1] - before[1] > 0
    assert after[0] == 64 and after[2] == before[2] + 1
    want, _ = A.add_ref(state, mbits, rows_of(keys, vals), capacity=C, dropped=lost)
    assert (st == want).all()
    ent = state_rows(tab)
    assert len(ent) == 64 and ent == state_bytes(state)


# ------------------------------------------------------------ 5. wide rows ---
@pytest.mark.parametrize("words", [63, 64, 65, 129])
def test_wide_rows(dev, oracle, words):
    """Rows of more pieces than a wave has lanes: the sweep loops of both row writers (eight-byte pieces for an
    odd number of words; 129 words are 65 + 64)."""
    L, n, C = 8, 130, 256
    B = 8 * words
    E = B - slot_of(L)
    keys = keys_with_repeats(n, L, words)
    mbits = oracle.city64_fixed(keys)
    for off, layout in ((0, "packed"), (1, "odd")):
        kd = keys_at(keys, dev, off)
        ta, tb, state = twins(dev, C, B, keys[::2], values_for(len(keys[::2]), E, 1))
        vals = values_for(n, E, words + off)
        vd = values_at(vals, dev, layout)
        st_a = ta.update_keys(kd, vd)
        assert P.last_kernel() == UPDATE.format(piece(B))
        assert torch.equal(st_a, tb.update_records(put_records_of(kd, vd)))
        assert (st_a.cpu().numpy() == M.update_ref(state, mbits, rows_of(keys, vals))).all()
        same_tables(ta, tb, state)
        vals = values_for(n, E, words + off + 7)
        vd = values_at(vals, dev, layout)
        st_a = ta.add_keys(kd, vd)
        assert P.last_kernel() == ADD.format(piece(B))
        assert torch.equal(st_a, tb.add_records(put_records_of(kd, vd)))
        assert (st_a.cpu().numpy() == A.add_ref(state, mbits, rows_of(keys, vals), capacity=C)[0]).all()
        assert (st_a == 0).any() and (st_a == 4).any()
        same_tables(ta, tb, state)


# ------------------------------------------------------------ 6. grid-stride ---
def test_grid_stride(dev, oracle):
    """One batch past the reach of every launch (table_grid caps a grid at 8 workgroups of 256 lanes per CU):
    with 13-byte keys and 8-byte values one round covers cus * 8 * 256 keys of k_table_locate_keys,
    k_table_add_claim_keys and k_table_cswap, and cus * 8 * 4 * 64 of the two row writers.  The models here
    are numpy: first and last occurrence of every mbits."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    m = cus * 8 * 1024 + 4097
    assert m % 64 != 0 and m < 1 << 24
    L, E, C, nd = 13, 8, 1 << 20, 300000
    B, slot = rowbytes_of(L, E), slot_of(L)
    rng = np.random.default_rng(5)
    distinct = np.unique(rng.integers(0, 256, (nd + 64, L), dtype=np.uint8), axis=0)[:nd]
    dmb = oracle.city64_fixed(distinct)
    assert len(distinct) == nd == len(np.unique(dmb))
    pick = rng.integers(0, nd, m)
    keys, mbits = distinct[pick], dmb[pick]
    kd = keys_at(keys, dev, 1)
    uniq, first = np.unique(mbits, return_index=True)
    # add into a table that holds the first 1000 distinct keys
    held = np.isin(mbits, dmb[:1000])
    tab, _, _ = twins(dev, C, B, distinct[:1000], values_for(1000, E, 1))
    before = rows_only(entries_of(tab))
    vals = rng.integers(0, 256, (m, E), dtype=np.uint8)
    st, mb = tab.add_keys(kd, to_dev(vals, dev), mbits=True)
    assert P.last_kernel() == ADD.format(8)
    assert (u64(mb) == mbits).all()
    want = np.full(m, 4, np.uint8)
    want[first] = 0
    want[held] = 4
    assert (st.cpu().numpy() == want).all()
    rows = rows_of(keys, vals)
    emb, erows, _ = tab.entries()
    order = np.argsort(u64(emb))
    semb, srows = u64(emb)[order], erows.cpu().numpy()[order]
    assert (semb == np.union1d(uniq, dmb[:1000])).all()
    at = np.searchsorted(semb, uniq)
    new = ~np.isin(uniq, dmb[:1000])
    assert (srows[at][new] == rows[first][new]).all()
    assert all(srows[i].tobytes() == before[int(semb[i])] for i in np.flatnonzero(np.isin(semb, dmb[:1000])))
    # update: the batch and 4097 absent keys behind it
    absent = rng.integers(0, 256, (4097, L), dtype=np.uint8)
    absent = absent[~np.isin(oracle.city64_fixed(absent), dmb)]
    more = np.concatenate([keys[:m - len(absent)], absent])
    mmb = np.concatenate([mbits[:m - len(absent)], oracle.city64_fixed(absent)])
    md = keys_at(more, dev, 1)
    vals = rng.integers(0, 256, (m, E), dtype=np.uint8)
    st = tab.update_keys(md, to_dev(vals, dev))
    assert P.last_kernel() == UPDATE.format(8)
    ulast = m - 1 - np.unique(mmb[::-1], return_index=True)[1]
    want = np.ones(m, np.uint8)
    want[ulast] = 0
    want[m - len(absent):] = 3
    assert (st.cpu().numpy() == want).all()
    rows = rows_of(more, vals)
    emb, erows, _ = tab.entries()
    order = np.argsort(u64(emb))
    srows2 = erows.cpu().numpy()[order]
    assert (u64(emb)[order] == semb).all()
    touched = np.unique(mmb[:m - len(absent)])
    tl = (m - len(absent)) - 1 - np.unique(mmb[:m - len(absent)][::-1], return_index=True)[1]
    at = np.searchsorted(semb, touched)
    assert (srows2[at] == rows[tl]).all()
    rest = np.ones(len(semb), bool)
    rest[at] = False
    assert (srows2[rest] == srows[rest]).all()
    # cswap against the record route on a copy of the table
    twin = P.DeviceTable(C, B, dev)
    twin.storage.copy_(tab.storage)
    compare = word_of(rows[tl[0]], slot)
    ra = tab.cswap_keys(md, slot, compare, 7)
    assert P.last_kernel() == CSWAP
    rb = twin.cswap(P.bucket_records(md.contiguous(), 1)[0], slot, compare, 7)
    assert torch.equal(ra, rb)
    assert torch.equal(tab.storage, twin.storage)  # nothing was inserted: the images stay equal
    assert ra[m - len(absent):, 0].eq(0).all() and ra[:m - len(absent), 0].eq(1).all()


# ------------------------------------------------------------ 7. mixing ---
def test_keyed_and_record_calls_mix_on_one_table(dev, oracle):
    """On table A keyed and record calls of every kind take turns; its twin B is driven by records only.
    After every call the entries and counts()[:3] agree: the batch numbers run on across the kinds.  Two
    rounds of eight calls, a clear() between them.  The capacity holds every key of a round: which new mbits
    an overflow drops is left to the schedule, and two tables need not agree on it."""
    L, E, n, C = 13, 16, 500, 4096
    B, slot = rowbytes_of(L, E), slot_of(L)
    ta, tb = P.DeviceTable(C, B, dev), P.DeviceTable(C, B, dev)
    calls = 0
    for rnd in (0, 1):
        def batch(k, count=n):
            keys = keys_with_repeats(count, L, 10 * rnd + k)
            vals = values_for(count, E, 10 * rnd + k)
            kd, vd = keys_at(keys, dev, k % 2), to_dev(vals, dev)
            return kd, vd, put_records_of(kd, vd)

        def check(nb):
            assert state_rows(ta) == state_rows(tb)
            assert ta.counts()[:3] == tb.counts()[:3] and ta.counts()[2] == nb

        kd0, vd0, rec0 = batch(0)
        assert torch.equal(ta.add_keys(kd0, vd0), tb.add_records(rec0))                       # keyed add
        check(1)
        kd1, vd1, rec1 = batch(1)
        assert torch.equal(ta.put_records(rec1), tb.put_records(rec1))                        # record put
        check(2)
        both = torch.cat([kd0, kd1])
        vals = to_dev(values_for(2 * n, E, 30 + rnd), dev)
        st_a, mb = ta.update_keys(both, vals, mbits=True)                                     # keyed update
        assert torch.equal(st_a, tb.update_records(put_records_of(both, vals))) and st_a.ne(3).all()
        check(3)
        word = word_of(vals[-1].cpu().numpy(), 0)
        assert torch.equal(ta.cswap(mb, slot, word, 5), tb.cswap(mb, slot, word, 5))          # cswap by mbits
        check(4)
        kd2, vd2, rec2 = batch(2)
        assert torch.equal(ta.acc_records(rec2, torch.int64, slot, 2, insert=True),           # inserting accumulate
                           tb.acc_records(rec2, torch.int64, slot, 2, insert=True))
        check(5)
        ask = torch.cat([kd2, kd0[:100]])
        assert torch.equal(ta.cswap_keys(ask, slot + 8, 0, 9),                                # keyed cswap
                           tb.cswap(P.bucket_records(ask.contiguous(), 1)[0], slot + 8, 0, 9))
        check(6)
        assert torch.equal(ta.put_keys(kd1, vd0), tb.put_records(put_records_of(kd1, vd0)))   # keyed put
        check(7)
        kd3, vd3, rec3 = batch(3)
        assert torch.equal(ta.add_records(rec3), tb.add_records(rec3))                        # record add
        check(8)
        va, sa = ta.get_keys(both, E)
        vb, sb = tb.get_keys(both, E)
        assert torch.equal(va, vb) and torch.equal(sa, sb) and sa.eq(0).all()
        calls += 8
        if rnd == 0:
            ta.clear()
            tb.clear()
            assert ta.counts() == (0, 0, 0, 0) and state_rows(ta) == {}
    assert calls == 16


# ------------------------------------------------------------ 8. workspace, guards, streams, graphs ---
@pytest.mark.parametrize("fill", [0x00, 0xFF, "leftovers"])
def test_workspace_of_the_queried_size_with_any_contents(dev, oracle, fill):
    """A workspace of exactly the queried size whose bytes on entry are zeros, ones or what another call
    left; status and replies between guard bytes."""
    L, E, n, C = 13, 8, 777, 2048
    B, slot = rowbytes_of(L, E), slot_of(L)
    keys, vals = keys_with_repeats(n, L, 11), values_for(n, E, 11)
    kd, vd = keys_at(keys, dev, 1), to_dev(vals, dev)
    mbits = oracle.city64_fixed(keys)
    ta, tb, state = twins(dev, C, B, keys[::2], values_for(len(keys[::2]), E, 12))

    def ws_of(need, want):
        assert need == want
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        if fill == "leftovers":
            c = (need - 3) // 5  # an add_keys of c keys fills 4 * c + c rounded up to 4 bytes of it
            P.DeviceTable(C, B, dev).add_keys(kd[:c], vd[:c], workspace=ws)
        else:
            ws.fill_(fill)
        return ws

    guard = torch.full((n + 16,), SENTINEL, dtype=torch.uint8, device=dev)
    st = guard[8:8 + n]
    ta.update_keys(kd, vd, status=st, workspace=ws_of(P.table_update_keys_workspace_bytes(n), 4 * n))
    assert (st.cpu().numpy() == M.update_ref(state, mbits, rows_of(keys, vals))).all()
    assert guard[:8].eq(SENTINEL).all() and guard[8 + n:].eq(SENTINEL).all()
    tb.update_records(put_records_of(kd, vd))
    same_tables(ta, tb, state)
    wide = torch.full((n + 2, 24), SENTINEL, dtype=torch.uint8, device=dev)
    rep = wide[1:n + 1, :16]
    compare = word_of(state[int(mbits[0])], slot)
    ta.cswap_keys(kd, slot, compare, 3, out=rep, workspace=ws_of(P.table_cswap_keys_workspace_bytes(n), 4 * n))
    assert (rep.cpu().numpy() == M.cswap_ref(state, mbits, slot, compare, 3)).all()
    assert wide[0].eq(SENTINEL).all() and wide[-1].eq(SENTINEL).all() and wide[:, 16:].eq(SENTINEL).all()
    tb.cswap(P.bucket_records(kd.contiguous(), 1)[0], slot, compare, 3)
    same_tables(ta, tb, state)
    guard.fill_(SENTINEL)
    ta.add_keys(kd, vd, status=st, workspace=ws_of(P.table_add_keys_workspace_bytes(n), 4 * n + (n + 3) // 4 * 4))
    assert (st.cpu().numpy() == A.add_ref(state, mbits, rows_of(keys, vals), capacity=C)[0]).all()
    assert guard[:8].eq(SENTINEL).all() and guard[8 + n:].eq(SENTINEL).all()
    tb.add_records(put_records_of(kd, vd))
    same_tables(ta, tb, state)


def test_on_a_side_stream(dev, oracle):
    L, E, n, C = 16, 8, 700, 1024
    B, slot = rowbytes_of(L, E), slot_of(L)
    keys, vals = keys_with_repeats(n, L, 13), values_for(n, E, 13)
    kd, vd = keys_at(keys, dev), to_dev(vals, dev)
    mbits = oracle.city64_fixed(keys)
    tab, _, state = twins(dev, C, B, keys[::2], values_for(len(keys[::2]), E, 14))
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    st_u = tab.update_keys(kd, vd, stream=s)
    rep = tab.cswap_keys(kd, slot, 0, 1, stream=s)
    st_a = tab.add_keys(kd, vd, stream=s)
    s.synchronize()
    rows = rows_of(keys, vals)
    assert (st_u.cpu().numpy() == M.update_ref(state, mbits, rows)).all()
    assert (rep.cpu().numpy() == M.cswap_ref(state, mbits, slot, 0, 1)).all()
    assert (st_a.cpu().numpy() == A.add_ref(state, mbits, rows, capacity=C)[0]).all()
    assert state_rows(tab) == state_bytes(state) and tab.counts()[2] == 4


def test_the_keyed_calls_capture_into_one_graph(dev, oracle):
    """add_keys -> update_keys -> cswap_keys -> get_keys captured on a side stream as one linear chain and
    replayed twice: the replays see the entries the eager run created, so both leave the same bytes."""
    L, E, n, C = 13, 8, 300, 1024
    B, slot = rowbytes_of(L, E), slot_of(L)
    keys, vals = keys_with_repeats(n, L, 6), values_for(n, E, 6)
    vals2 = values_for(n, E, 16)
    kd, vd, vd2 = keys_at(keys, dev, 1), to_dev(vals, dev), to_dev(vals2, dev)
    mbits = oracle.city64_fixed(keys)
    tab = P.DeviceTable(C, B, dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    st_a, st_u, gst = torch.empty(n, **u8), torch.empty(n, **u8), torch.empty(n, **u8)
    ws = torch.empty(P.table_add_keys_workspace_bytes(n), **u8)
    mb = torch.empty(n, dtype=torch.int64, device=dev)
    rep, out = torch.empty((n, 16), **u8), torch.empty((n, E), **u8)
    compare = word_of(vals2[n - 1], 0)  # the last key's value word: its entry holds it after the update

    def chain():
        tab.add_keys(kd, vd, status=st_a, workspace=ws)
        tab.update_keys(kd, vd2, status=st_u, mbits=mb, workspace=ws)
        tab.cswap_keys(kd, slot, compare, 0x55, out=rep, workspace=ws)
        tab.get_keys(kd, E, values=out, status=gst)

    chain()  # eager
    torch.cuda.synchronize(dev)
    state = {}
    want_a, _ = A.add_ref(state, mbits, rows_of(keys, vals), capacity=C)
    assert (st_a.cpu().numpy() == want_a).all() and tab.counts()[:3] == (len(state), 0, 3)
    want_u = M.update_ref(state, mbits, rows_of(keys, vals2))
    want_rep = M.cswap_ref(state, mbits, slot, compare, 0x55)
    assert (st_u.cpu().numpy() == want_u).all() and (rep.cpu().numpy() == want_rep).all() and gst.eq(0).all()
    s = torch.cuda.Stream(device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain()
    assert tab.counts()[2] == 3  # capture runs nothing
    seen = []
    for k in (1, 2):
        for t in (st_a, st_u, gst, rep, out):
            t.fill_(9)
        mb.fill_(9)
        g.replay()
        torch.cuda.synchronize(dev)
        seen.append([t.clone() for t in (st_a, st_u, gst, rep, out, mb)])
        assert tab.counts()[:3] == (len(state), 0, 3 + 3 * k)
    for a, b in zip(*seen):
        assert torch.equal(a, b)
    st_a2, st_u2, gst2, rep2, out2, mb2 = seen[1]
    # every key is present now: the add changes nothing, the update restores the rows, the swap sees them again
    assert st_a2.eq(4).all() and (st_u2.cpu().numpy() == want_u).all() and (rep2.cpu().numpy() == want_rep).all()
    assert (u64(mb2) == mbits).all() and gst2.eq(0).all()
    assert state_rows(tab) == state_bytes(state)
    want_out = np.stack([state[int(k)][slot:slot + E] for k in mbits])
    assert (out2.cpu().numpy() == want_out).all()
