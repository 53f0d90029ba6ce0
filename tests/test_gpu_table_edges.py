"""GPU checks of the device-resident table where tests/test_gpu_table.py stops: rows and values of more
pieces than a wave has lanes, a batch that overflows part-way, the exact number of slots a put inspects,
batches past the grid's reach (every grid-stride loop takes a second round), long sequences of batches on
one table with a clear() in between, and caller-owned storage with guard bytes around it.  Every
comparison is byte-exact against a CPU model (Model of test_gpu_table.py, tests/table_ref.py), inside the
documented contract of include/pdht_hip_table.h."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

import table_ref as R  # noqa: E402
from test_gpu_table import (ALL_ONES, Model, check_get, distinct_mbits, forge, forged_replies,  # noqa: E402
                            np_resolve, rec_to_dev, rows_for, splitmix64, to_dev)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rec16_to_dev(rec, dev):
    """Records at base = 8 mod 16, so that the rows at +24 start 16-byte aligned (k_table_write<16> when the
    stride and rowbytes are multiples of 16 too)."""
    m, S = rec.shape
    buf = torch.empty(m * S // 8 + 2, dtype=torch.int64, device=dev).view(torch.uint8)[8:8 + m * S].view(m, S)
    assert buf.data_ptr() % 16 == 8
    buf.copy_(to_dev(rec, dev))
    return buf


def with_repeats(keys, m, rng):
    """m records over `keys`: every key at least once (when m allows), the rest repeats, shuffled."""
    n = len(keys)
    if m <= n:
        return keys[rng.permutation(n)[:m]]
    return keys[rng.permutation(np.concatenate([np.arange(n), rng.integers(0, n, m - n)]))]


# ------------------------------------------------------------------ 1. wide rows ---
# Pieces of a row (pdht_table.hip):
#   put   np = B/16 (k_table_write<16>) when B, the record stride and the address of the first row are
#         multiples of 16, else np = B/8 (<8>);
#   get   head 8 on aligned replies moves nw = B/8 + 1 words, W = 2 of them per lane (k_table_get<16>)
#         when nw is even and replies and stride are 16-byte aligned, else W = 1 (<8>): np = nw / W;
#         anything else moves np = head + B bytes (k_table_get_bytes).
# A wave's 64 lanes take pieces 0..63 at once; pieces 64.. are the tail loops under test.
WIDE = (496, 504, 512, 520, 1000, 1008, 1016, 1024, 1032, 1040, 2056, 2064)
WIDE_MS = (1, 65, 4097)


def get_pieces(B):
    nw = B // 8 + 1
    W = 2 if nw % 2 == 0 else 1
    return W, nw // W


def test_wide_rowbytes_straddle_one_wave():
    """The parameter table itself: each kernel sees 63, 64, 65 and 129 pieces (k_table_get<8> moves an odd
    number of words, so never 64)."""
    put8 = {B // 8 for B in WIDE}
    put16 = {B // 16 for B in WIDE if B % 16 == 0}
    get8 = {get_pieces(B)[1] for B in WIDE if get_pieces(B)[0] == 1}
    get16 = {get_pieces(B)[1] for B in WIDE if get_pieces(B)[0] == 2}
    assert {63, 64, 65, 129} <= put8 and {63, 64, 65, 129} <= put16 and {63, 64, 65, 129} <= get16
    assert {63, 65, 129} <= get8
    assert {504, 512, 520, 1016, 1024, 1032, 1040, 2056} <= set(WIDE)


@pytest.mark.parametrize("m", WIDE_MS)
@pytest.mark.parametrize("B", WIDE)
def test_wide_rows_put_get(dev, B, m):
    rng = np.random.default_rng(B * 7 + m)
    keys = distinct_mbits({1: 1, 65: 20, 4097: 1500}[m], 100)
    mb = with_repeats(keys, m, rng)
    assert len(np.unique(mb)) == len(keys)  # repeats: superseded wide rows must write nothing
    absent = distinct_mbits(37, 101)
    q = np.concatenate([keys, absent, rng.choice(keys, 64)])[rng.permutation(len(keys) + 37 + 64)]
    layouts = [(8, 24 + B, rec_to_dev)]
    if B % 16 == 0:
        layouts.append((16, 24 + B + 8, rec16_to_dev))
    for piece, S, place in layouts:
        tab, model = P.DeviceTable(16384, B, dev), Model(16384)
        rows = rows_for(m, B, 100 + piece)
        rec = place(forge(mb, rows, S), dev)
        st = tab.put_records(rec)
        assert P.last_kernel() == f"k_table_claim+k_table_write<{piece}>"
        assert (st.cpu().numpy() == model.put_fast(mb, rows)).all()
        assert tab.counts()[:3] == (len(keys), 0, 1)
        W, _ = get_pieces(B)
        assert tab.get(to_dev(q.view(np.int64), dev)).shape == (len(q), 8 + B)
        assert P.last_kernel() == ("k_table_get<16>" if W == 2 else "k_table_get<8>")
        check_get(tab, model, q, dev)  # stored, absent and repeated requests
        check_get(tab, model, mb, dev, records=rec)  # read in place


# ------------------------------------------------------------- 2. wide values ---
def resolve_piece(replies, head, slot, values, E):
    """The rule of get_resolve in pdht_table.hip: the widest of 16 / 8 / 4 / 1 bytes that divides the address
    of the value in the reply, the reply stride, the values address and stride, and E."""
    rstride = replies.stride(0) if replies.shape[0] > 1 else replies.shape[1]
    vstride = values.stride(0) if values.shape[0] > 1 else values.shape[1]
    bits = (replies.data_ptr() + head + slot) | rstride | values.data_ptr() | vstride | E
    return 16 if bits % 16 == 0 else 8 if bits % 8 == 0 else 4 if bits % 4 == 0 else 1


RESOLVE_E = (260, 520, 1024, 1040)
RESOLVE_L = (8, 300)


def static_resolve_piece(E, L, head):
    """resolve_piece for dense, 16-byte aligned replies and values (what the allocator returns)."""
    slot = (L + 7) // 8 * 8
    bits = (head + slot) | (head + slot + E) | E
    return 16 if bits % 16 == 0 else 8 if bits % 8 == 0 else 4 if bits % 4 == 0 else 1


def test_wide_values_cover_every_piece_width():
    """The parameter table itself: <1>, <4>, <8> and <16> each move a value of more than 64 pieces."""
    seen = {}
    for E in RESOLVE_E:
        for L in RESOLVE_L:
            for head in (1, 8):
                p = static_resolve_piece(E, L, head)
                seen[p] = max(seen.get(p, 0), E // p)
    assert set(seen) == {1, 4, 8, 16} and all(n > 64 for n in seen.values()), seen


@pytest.mark.parametrize("head", [1, 8])
@pytest.mark.parametrize("L", RESOLVE_L)
@pytest.mark.parametrize("E", RESOLVE_E)
def test_wide_values_resolve(dev, E, L, head):
    slot = (L + 7) // 8 * 8
    for m in (1, 65, 4097):
        n = m + 9
        keys, index, rep = forged_replies(m, n, L, E, slot, head, 0, L * E + m + head)
        # some replies that carry another key differ from it in the LAST key byte only: with L = 300 that
        # byte is compared in the fifth pass of a 64-lane group
        found = np.flatnonzero(rep[:, 0] == 1)
        tail = found[::3]
        rep[tail, head:head + L] = keys[index[tail]]
        rep[tail, head + L - 1] ^= 0x80
        want_v = np.full((n, E), 0x5A, np.uint8)
        want_s = np.full(n, 0xEE, np.uint8)
        np_resolve(rep, head, slot, keys, index, E, want_v, want_s)
        if m >= 65:
            assert (want_s[index[tail]] == 3).all() and len(tail) > 0
            assert (want_s == 0).any() and (want_s == 2).any() and (want_s == 3).sum() > len(tail)
        kd, rd = to_dev(keys, dev), to_dev(rep, dev)
        # a dense index
        vals = torch.full((n, E), 0x5A, dtype=torch.uint8, device=dev)
        stat = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        v, s = P.get_resolve(rd, kd, E, head=head, index=to_dev(index.view(np.int32), dev), values=vals,
                             status=stat)
        piece = resolve_piece(rd, head, slot, vals, E)
        assert P.last_kernel() == f"k_get_resolve<{piece}>"
        if m > 1:
            assert piece == static_resolve_piece(E, L, head)
        assert (s.cpu().numpy() == want_s).all()
        assert (v.cpu().numpy() == want_v).all()  # rows whose status is not 0 keep the pattern
        # the index in place at +12 of a record batch, values row-strided
        recs = np.zeros((m, 32), np.uint8)
        recs[:, 12:16] = index.view(np.uint8).reshape(m, 4)
        ix = to_dev(recs, dev).view(torch.int32).view(m, 8)[:, 3]
        wide = torch.full((n, E + 24), 0x5A, dtype=torch.uint8, device=dev)
        stat.fill_(0xEE)
        v, s = P.get_resolve(rd, kd, E, head=head, index=ix, values=wide[:, 8:8 + E], status=stat)
        assert P.last_kernel() == f"k_get_resolve<{resolve_piece(rd, head, slot, wide[:, 8:8 + E], E)}>"
        assert (s.cpu().numpy() == want_s).all()
        w = wide.cpu().numpy()
        assert (w[:, 8:8 + E] == want_v).all() and (w[:, :8] == 0x5A).all() and (w[:, 8 + E:] == 0x5A).all()


# --------------------------------------------------------- 3. part-way overflow ---
@pytest.mark.parametrize("B", [8, 40, 520])
def test_overflow_part_way(dev, B):
    """More new mbits than free slots, each with many records (pdht_hip_table.h: a present mbits is never
    dropped, the schedule picks the losers, all records of one mbits share the fate).  Which new mbits won
    is the one thing read from the device, and it is capped: exactly as many as there were free slots."""
    C, S = 64, 24 + B
    rng = np.random.default_rng(300 + B)
    tab, model = P.DeviceTable(C, B, dev), Model(C)
    old = distinct_mbits(40, 300)
    rows = rows_for(40, B, 300)
    st = tab.put_records(rec_to_dev(forge(old, rows, S), dev))
    assert (st.cpu().numpy() == model.put(old, rows)).all() and tab.counts()[:3] == (40, 0, 1)
    new = np.concatenate([distinct_mbits(100, 301), np.array([1], np.uint64)])  # mbits 1 competes like any key
    assert len(np.unique(np.concatenate([old, new]))) == 141
    mb = with_repeats(np.concatenate([old, new, np.zeros(1, np.uint64)]), 4097, rng)
    assert np.bincount(np.unique(mb, return_inverse=True)[1]).min() >= 10  # every mbits many times
    winners, dropped = None, 0
    for rnd in (0, 1):  # the same batch again with new rows: tags are final
        rows = rows_for(4097, B, 310 + rnd)
        rec = rec_to_dev(forge(mb, rows, S), dev)
        st = tab.put_records(rec).cpu().numpy()
        lost = st == 2
        # all records of one mbits share the fate
        lost_keys, kept_keys = set(mb[lost].tolist()), set(mb[~lost].tolist())
        assert not (lost_keys & kept_keys)
        assert set(old.tolist()) <= kept_keys and 0 in kept_keys  # present mbits and mbits 0 are never dropped
        won = kept_keys - set(old.tolist()) - {0}
        assert won <= set(new.tolist()) and len(won) == C - 40
        if rnd == 0:
            winners = won
        assert won == winners
        # from here on the model decides: the sub-batch of the stored mbits, applied one after the other
        keep = np.isin(mb, np.array(sorted(kept_keys), np.uint64))
        assert (keep == ~lost).all()
        want = np.full(4097, 2, np.uint8)
        want[keep] = model.put_fast(mb[keep], rows[keep])
        assert (st == want).all()  # exactly the last record of a stored mbits has 0, the rest 1
        dropped += int((want == 2).sum())
        assert dropped == (rnd + 1) * int(np.isin(mb, np.array(sorted(set(new.tolist()) - winners),
                                                               np.uint64)).sum())
        assert tab.counts()[:3] == (C + 1, dropped, 2 + rnd)
        assert len(model.d) == C + 1
        q = np.concatenate([old, new, np.zeros(1, np.uint64), distinct_mbits(5, 302)])
        check_get(tab, model, q, dev)  # losers and absent mbits: all-zero replies
        check_get(tab, model, mb, dev, records=rec)
        losers = np.array(sorted(set(new.tolist()) - winners), np.uint64)
        assert len(losers) == 101 - (C - 40)
        assert int(tab.get(to_dev(losers.view(np.int64), dev)).count_nonzero()) == 0


# ------------------------------------------------------ 4. exact slots inspected ---
def structured_mbits(kind):
    i = np.arange(32768, dtype=np.uint64)
    if kind == "low16":
        return (splitmix64(i) << np.uint64(16)) | np.uint64(0x1234)
    return (splitmix64(i) >> np.uint64(12)) * np.uint64(1024) + np.uint64(5)


@pytest.fixture(scope="module")
def probe_cases():
    """Per case: capacity, the keys, probe_model's cost of each and its cluster (made once, never written)."""
    out = {}
    for kind, C in (("low16", 65536), ("mod1024", 65536), ("full", 64)):
        keys = distinct_mbits(64, 40) if kind == "full" else structured_mbits(kind)
        assert len(np.unique(keys)) == len(keys)
        slots, cost = R.probe_model(keys, C)
        lab, ncl = R.clusters(slots, C)
        out[kind] = (C, keys, cost, lab, ncl)
    return out


@pytest.mark.parametrize("kind", ["low16", "mod1024", "full"])
def test_exact_slots_inspected(dev, probe_cases, kind):
    """counts()[3] against the probe model, exactly.  A put of a PRESENT mbits inspects 1 + its displacement
    from home = (mbits * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - log2 C) and claims nothing, so a batch of
    present mbits adds a number that no race can change.  The order in which the first batch's waves
    claimed decides where inside its cluster (run of occupied slots) a key sits, but not the sum over a
    whole cluster (tests/test_table_ref_cpu.py::test_order_independence), so the second batch draws whole
    clusters, with repeats, 4097 records in all with mbits 0 filling up.  This pins the home bits, the
    wrap (the full table is one cluster around the ring), the step and the counter."""
    C, keys, cost, lab, ncl = probe_cases[kind]
    n, B = len(keys), 8
    rng = np.random.default_rng(400 + n)
    tab, model = P.DeviceTable(C, B, dev), Model(C)
    rows = rows_for(n, B, 400)
    st = tab.put_records(rec_to_dev(forge(keys, rows, 24 + B), dev))
    assert (st.cpu().numpy() == model.put_fast(keys, rows)).all()
    entries, dropped, nb, first = tab.counts()
    assert (entries, dropped, nb) == (n, 0, 1)
    total = int(cost.sum())
    print(f"{kind}: first batch {first / n:.4f} slots inspected per record, the model {total / n:.4f}")
    assert first >= total  # a lost compare-and-swap race can only add slots

    by_cluster = [np.flatnonzero(lab == c) for c in range(ncl)]
    pick, left = [], 4096
    for c in rng.integers(0, ncl, 100000):  # clusters drawn with repeats until 4096 records are taken
        if len(by_cluster[c]) <= left:
            pick.append(by_cluster[c])
            left -= len(by_cluster[c])
        if left == 0:
            break
    pick = np.concatenate(pick)
    assert len(pick) == 4096 and len(np.unique(pick)) < 4096  # with repeats
    mb = np.concatenate([keys[pick], np.zeros(1, np.uint64)])  # mbits 0 inspects its one private slot
    want = int(cost[pick].sum()) + 1
    mb = mb[rng.permutation(4097)]
    rows2 = rows_for(4097, B, 401)
    st = tab.put_records(rec_to_dev(forge(mb, rows2, 24 + B), dev))
    assert (st.cpu().numpy() == model.put_fast(mb, rows2)).all()
    entries, dropped, nb, second = tab.counts()
    print(f"{kind}: second batch {(second - first) / 4097:.4f} slots inspected per record, "
          f"the model {want / 4097:.4f}")
    assert (entries, dropped, nb) == (n + 1, 0, 2)
    assert second - first == want

    # every key once more, in another order: the whole model total, whatever the first batch's schedule was
    order = rng.permutation(n)
    rows3 = rows_for(n, B, 402)
    rec = rec_to_dev(forge(keys[order], rows3, 24 + B), dev)
    st = tab.put_records(rec)
    assert (st.cpu().numpy() == model.put_fast(keys[order], rows3)).all()
    entries, dropped, nb, third = tab.counts()
    assert (entries, dropped, nb) == (n + 1, 0, 3)
    assert third - second == total
    q = np.concatenate([keys, np.zeros(1, np.uint64)])
    got = tab.get(to_dev(q.view(np.int64), dev)).cpu().numpy()
    assert (got == model.replies(q, 8, B)).all()
    assert (tab.get(rec).cpu().numpy() == model.replies(keys[order], 8, B)).all()


# ---------------------------------------------------------------- 5. grid-stride ---
@pytest.fixture(scope="module")
def grid_keys():
    """300000 distinct mbits and what probe_model says a put of all of them inspects in 2^20 slots (made once,
    never written)."""
    keys = distinct_mbits(300000, 500)
    return keys, int(R.probe_model(keys, 1 << 20)[1].sum())


@pytest.mark.parametrize("B,S,piece", [(8, 32, 8), (16, 48, 16)])
def test_grid_stride(dev, grid_keys, B, S, piece):
    """One batch past the reach of every launch, so that each grid-stride loop runs a second round, the last
    one with part of a wave past the end.  table_grid (pdht_table.hip) caps a grid at 8 workgroups per CU
    of kBlock = 256 lanes = 4 waves; one round of the whole grid covers
      k_table_claim   one record per lane                                   cus * 8 * 256
      k_table_write   np = 1: 64 records per wave x kRowsInFlight = 4       cus * 8 * 4 * 256 = cus * 8 * 1024
      k_table_get     at most 64 requests per wave (np = 1)                 cus * 8 * 4 * 64  = cus * 8 * 256
    records.  Every ordinary mbits occurs equally often (mbits 0 fills up), so that the slots a second put
    of the same records inspects are a number no schedule changes: each key's whole cluster as often."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    m = cus * 8 * 1024 + 4097
    assert m > cus * 8 * 256 and m > cus * 8 * 4 * 256 and m > cus * 8 * 4 * 64
    assert m % 64 != 0 and m < 1 << 24
    C = 1 << 20
    t0 = time.perf_counter()
    rng = np.random.default_rng(500 + B)
    keys, total = grid_keys
    times = m // len(keys)
    zeros = m - times * len(keys)
    assert times >= 2 and zeros >= 1
    mb = np.concatenate([np.tile(keys, times), np.zeros(zeros, np.uint64)])[rng.permutation(m)]
    rows = rng.integers(0, 256, (m, B), dtype=np.uint8)
    rec = np.empty((m, S), np.uint8)  # forge() without its noise: 100 MB of it is this test's time
    rec[:, :16] = 0xC7
    rec[:, 16:24] = mb.view(np.uint8).reshape(m, 8)
    rec[:, 24:24 + B] = rows
    rec[:, 24 + B:] = 0x3C
    place = rec16_to_dev if piece == 16 else rec_to_dev
    recd = place(rec, dev)
    tab = P.DeviceTable(C, B, dev)
    want_st, state = R.put_ref(mb, rows)
    probes = 0
    for rnd in (1, 2):  # the second time every mbits is present
        st = tab.put_records(recd)
        assert P.last_kernel() == f"k_table_claim+k_table_write<{piece}>"
        assert torch.equal(st.cpu(), torch.from_numpy(want_st))
        entries, dropped, nb, seen = tab.counts()
        assert (entries, dropped, nb) == (300001, 0, rnd)
        assert seen - probes >= times * total + zeros  # lost races only add
        if rnd == 2:
            assert seen - probes == times * total + zeros
        probes = seen
    absent = distinct_mbits(4097, 501)
    for head in (8, 1):
        got = tab.get(recd, head=head)  # all records in place
        assert torch.equal(got.cpu(), torch.from_numpy(R.replies_ref(state, mb, head, B)))
        got = tab.get(to_dev(absent.view(np.int64), dev), head=head)
        assert int(got.count_nonzero()) == 0 and tuple(got.shape) == (4097, head + B)
    # a small batch over the same table: updates, new mbits, and the winner words of the big batches lose
    mb2 = np.concatenate([keys[:40], absent[:24], np.zeros(1, np.uint64)])[rng.permutation(65)]
    rows2 = rows_for(65, B, 502)
    st = tab.put_records(place(forge(mb2, rows2, S), dev))
    want_st, state = R.put_ref(mb2, rows2, state)
    assert (st.cpu().numpy() == want_st).all()
    assert tab.counts()[:3] == (300025, 0, 3)
    q = np.concatenate([mb2, keys[40:4000], absent[24:]])
    got = tab.get(to_dev(q.view(np.int64), dev))
    assert (got.cpu().numpy() == R.replies_ref(state, q, 8, B)).all()
    print(f"grid-stride rowbytes {B}: m {m} on {cus} CUs, {time.perf_counter() - t0:.2f} s wall")


# -------------------------------------------------------------- 6. long sequences ---
@pytest.mark.parametrize("B", [8, 40])
def test_sixteen_batches_and_a_clear(dev, B):
    """Winner words are never cleared between batches; (batch << 32) | position must order them.  16 batches
    on one table of 256 slots over a pool of 180 mbits (it never overflows, so the dict model is exact),
    clear() after the eighth with the same object going on."""
    rng = np.random.default_rng(600 + B)
    pool = np.concatenate([np.array([0, 1, ALL_ONES], np.uint64), distinct_mbits(177, 600)])
    absent = distinct_mbits(9, 601)
    x, y = pool[5], pool[6]
    sizes = [4097, 63, 300, 4097, 63, 300, 1, 63, 300, 4097, 1, 63] + [int(s) for s in rng.choice([1, 63, 300, 4097], 4)]
    assert len(sizes) == 16
    tab, model = P.DeviceTable(256, B, dev), Model(256)
    batches = 0
    for k, m in enumerate(sizes):
        mb = rng.choice(pool, m)
        if k == 3:  # x wins at a high position ...
            mb[mb == x] = pool[7]
            mb[4000] = x
        if k == 4:  # ... and in the next batch at a lower one than the winner word still holds
            mb[mb == x] = pool[7]
            mb[2] = x
            assert np.flatnonzero(mb == x).max() == 2 < 4000
        if k in (5, 9):  # position 0 is the only writer of its mbits (after clear() too: the word is 0 | 0)
            mb[mb == y] = pool[7]
            mb[0] = y
            assert (mb == y).sum() == 1
        rows = rows_for(m, B, 610 + k)
        rec = rec_to_dev(forge(mb, rows, 24 + B + (8 if k % 2 else 0)), dev)
        st = tab.put_records(rec)
        assert (st.cpu().numpy() == model.put_fast(mb, rows)).all()
        batches += 1
        n0 = 1 if 0 in model.d else 0
        assert tab.counts()[:3] == (len(model.d), 0, batches)
        assert len(model.d) - n0 <= 179
        check_get(tab, model, np.concatenate([pool, absent]), dev)
        check_get(tab, model, mb, dev, records=rec)
        if k == 7:
            tab.clear()
            model, batches = Model(256), 0
            assert tab.counts() == (0, 0, 0, 0)
            check_get(tab, model, np.concatenate([pool, absent]), dev)  # nothing is found


# ------------------------------------------------------- 7. caller-owned storage ---
@pytest.mark.parametrize("B", [8, 1040])
def test_caller_owned_storage(dev, B):
    """DeviceTable(storage=...): nothing is written outside the table_bytes the caller handed over, and
    mbits 0's private slot C is the last row of the buffer."""
    C, S = 64, 24 + B
    nbytes = P.table_bytes(C, B)
    assert nbytes == 64 + (C + 1) * (16 + B)
    buf = torch.full((nbytes + 2 * 4096,), 0xA5, dtype=torch.uint8, device=dev)
    off = 4096 + (-(buf.data_ptr() + 4096)) % 16
    storage = buf[off:off + nbytes]
    tab, model = P.DeviceTable(C, B, dev, storage=storage), Model(C)
    assert tab.storage.data_ptr() == buf.data_ptr() + off and tab.nbytes == nbytes

    def guards_intact():
        d = buf.cpu().numpy()
        return (d[:off] == 0xA5).all() and (d[off + nbytes:] == 0xA5).all()

    assert guards_intact()
    mb = np.concatenate([distinct_mbits(64, 40), np.zeros(1, np.uint64)])
    rows = rows_for(65, B, 700)
    st = tab.put_records(rec_to_dev(forge(mb, rows, S), dev))  # every slot and the private one
    assert (st.cpu().numpy() == model.put(mb, rows)).all() and (st == 0).all()
    assert tab.counts()[:3] == (65, 0, 1) and guards_intact()
    over = np.concatenate([distinct_mbits(30, 701), mb])[np.random.default_rng(7).permutation(95)]
    orows = rows_for(95, B, 701)
    rec = rec_to_dev(forge(over, orows, S), dev)
    st = tab.put_records(rec)  # 30 new mbits and no free slot
    want = model.put(over, orows)
    assert (st.cpu().numpy() == want).all() and (want == 2).sum() == 30
    assert tab.counts()[:3] == (65, 30, 2) and guards_intact()
    check_get(tab, model, over, dev, records=rec)  # both heads
    assert guards_intact()
    zero = tab.get(to_dev(np.zeros(1, np.int64), dev)).cpu().numpy()[0]
    zrow = orows[np.flatnonzero(over == 0)[-1]]
    assert zero[0] == 1 and (zero[8:] == zrow).all()
    assert (buf[off + nbytes - B:off + nbytes].cpu().numpy() == zrow).all()  # slot C: the last thing written


# ------------------------------------------------------- 8. high batch numbers ---
# "A table takes 2^32 batches between two inits" (include/pdht_hip_table.h): the winner word is
# (counters[2] << 32) | position under an unsigned 64-bit atomicMax, in five claim / locate kernels and four second
# kernels.  counters[2] is the u64 at byte 16 of the table's buffer (tests/table_iter_ref.py has the layout); a
# test may move it FORWARD, which leaves the older winner words with smaller numbers -- the state of a long-lived
# table.
import table_acc_ref as ACCR  # noqa: E402
import table_add_ref as ADDR  # noqa: E402
import table_rmw_ref as RMWR  # noqa: E402
from test_gpu_table_add import check_table, rec_at, replies8, run_add  # noqa: E402

EVERY_KIND = ["add", "put", "update", "cswap", "acc", "add", "put", "add", "cswap",
              "add", "update", "add", "acc", "cswap", "add", "put", "add"]  # seventeen batches, no clear


def set_batch_number(tab, v):
    assert tab.counts()[2] <= v < 1 << 32  # forward only, inside the contract
    tab.storage[16:24].view(torch.int64).fill_(v)
    assert tab.counts()[2] == v


def one_batch(tab, state, what, mb, rows, dev):
    """One batch of the kind `what` on the device and on the dict model: status / replies compared."""
    B, m = tab.rowbytes, len(mb)
    rec = rec_at(forge(mb, rows, 24 + B), dev)
    if what == "add":
        run_add(tab, state, mb, rows, dev)
    elif what == "put":
        st = tab.put_records(rec).cpu().numpy()
        last = m - 1 - np.unique(mb[::-1], return_index=True)[1]
        want = np.ones(m, np.uint8)
        want[last] = 0
        assert (st == want).all()
        for p in last:
            state[int(mb[p])] = rows[p].copy()
    elif what == "update":
        assert (tab.update_records(rec).cpu().numpy() == RMWR.update_ref(state, mb, rows)).all()
    elif what == "cswap":
        held = [k for k in mb.tolist() if k in state]
        word = int(state[held[0]][8:16].view(np.uint64)[0])  # what one of the entries holds: it swaps
        got = tab.cswap(rec, 8, word, 77).cpu().numpy()
        assert (got == RMWR.cswap_ref(state, mb, 8, word, 77)).all()
    else:
        assert what == "acc"
        st = tab.acc_records(rec, torch.int64, 16, insert=True).cpu().numpy()
        assert (st == ACCR.acc_ref(state, mb, rows, np.int64, 16, 1, True, capacity=tab.capacity)[0]).all()


@pytest.mark.parametrize("start", [(1 << 31) - 9, (1 << 32) - 17], ids=["across_bit_31", "up_to_2_32"])
def test_seventeen_batches_of_every_kind_at_high_batch_numbers(dev, start):
    """A 256-slot table that took one batch of every kind at small numbers, then counters[2] moved to 2^31 - 9
    (bit 31 of the batch number is set from the tenth batch on) or to 2^32 - 17 (the last batch carries number
    2^32 - 1 and leaves counts()[2] == 2^32, where the contract ends): add / put / update / cswap / inserting
    accumulate in turn over one pool of mbits with heavy repeats and mbits 0.  After every batch the status, the
    replies, the three counters and the whole table (get and export) against the dict models."""
    B, C = 24, 256
    pool = np.concatenate([np.zeros(1, np.uint64), distinct_mbits(130, 8300)])
    rng = np.random.default_rng(8301)
    tab, state, batches = P.DeviceTable(C, B, dev), {}, 0
    for t, what in enumerate(["add", "put", "update", "cswap", "acc"]):
        mb = pool[rng.integers(0, 40, 300)]
        one_batch(tab, state, what, mb, rows_for(300, B, 8302 + t), dev)
        batches += 1
        assert tab.counts()[:3] == (len(state), 0, batches)
    set_batch_number(tab, start)
    batches = start
    for t, what in enumerate(EVERY_KIND):
        m = int(rng.integers(300, 600))
        mb = pool[rng.integers(0, 60 + 4 * t, m)]
        mb[rng.integers(0, m, 3)] = 0
        assert (mb == 0).any() and len(np.unique(mb)) < m // 2  # mbits 0, heavy repeats
        one_batch(tab, state, what, mb, rows_for(m, B, 8310 + t), dev)
        batches += 1
        entries, dropped, nb = tab.counts()[:3]
        assert (entries, dropped) == (len(state), 0) and isinstance(nb, int) and nb == batches
        check_table(tab, state, pool, dev)
    assert len(EVERY_KIND) == 17 and batches == start + 17
    assert (start < 1 << 31 < batches) or batches == 1 << 32


def test_put_cswap_add_in_a_graph_across_bit_31(dev):
    """One captured graph of put(a) -> cswap -> add(c), captured with counters[2] at 2^31 - 2 and replayed three
    times: the nine batches carry the numbers 2^31 - 2 .. 2^31 + 6, and the model is stepped along."""
    B, m, C = 40, 900, 1024
    keys = distinct_mbits(400, 8400)
    rng = np.random.default_rng(8401)
    batch = {x: keys[rng.integers(lo, hi, m)] for x, (lo, hi) in dict(a=(0, 250), b=(100, 300), c=(150, 400)).items()}
    rows = {x: rows_for(m, B, 8402 + i) for i, x in enumerate("abc")}
    rec = {x: rec_at(forge(batch[x], rows[x], 24 + B), dev) for x in "abc"}
    both = next(k for k in batch["b"].tolist() if k in set(batch["a"].tolist()))
    last_a = int(np.flatnonzero(batch["a"] == np.uint64(both)).max())  # the record of a whose row stays, and b asks
    compare = int(rows["a"][last_a][8:16].view(np.uint64)[0])           # for its mbits: the cswap swaps on every replay
    tab, state = P.DeviceTable(C, B, dev), {}
    ws = torch.empty(P.table_add_workspace_bytes(m), dtype=torch.uint8, device=dev)
    st = {x: torch.empty(m, dtype=torch.uint8, device=dev) for x in "ac"}
    swapped = torch.empty((m, 16), dtype=torch.uint8, device=dev)
    rep = torch.empty((m, 8 + B), dtype=torch.uint8, device=dev)

    def step():
        tab.put_records(rec["a"], status=st["a"], workspace=ws[:4 * m])
        tab.cswap(rec["b"], 8, compare, 0x5555, out=swapped, workspace=ws[:4 * m])
        tab.add_records(rec["c"], status=st["c"], replies=rep, workspace=ws)

    def model_step():
        want = {}
        last = m - 1 - np.unique(batch["a"][::-1], return_index=True)[1]
        want["a"] = np.ones(m, np.uint8)
        want["a"][last] = 0
        for p in last:
            state[int(batch["a"][p])] = rows["a"][p].copy()
        want["b"] = RMWR.cswap_ref(state, batch["b"], 8, compare, 0x5555)
        assert (want["b"][:, 8:16] == np.frombuffer(np.uint64(compare).tobytes(), np.uint8)).all(1).any()
        want["c"] = ADDR.add_ref(state, batch["c"], rows["c"], capacity=C)
        return want

    def compare_all(want):
        assert (st["a"].cpu().numpy() == want["a"]).all() and (swapped.cpu().numpy() == want["b"]).all()
        assert (st["c"].cpu().numpy() == want["c"][0]).all() and (rep.cpu().numpy() == want["c"][1]).all()
        check_table(tab, state, keys, dev)

    step()  # eager, at small numbers
    compare_all(model_step())
    first = (1 << 31) - 2
    set_batch_number(tab, first)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    assert tab.counts()[2] == first  # capture runs nothing
    for k in (1, 2, 3):
        for t in list(st.values()) + [swapped, rep]:
            t.fill_(9)
        g.replay()
        torch.cuda.synchronize(dev)
        compare_all(model_step())
        assert tab.counts()[:3] == (len(state), 0, first + 3 * k)
    assert first + 9 > 1 << 31


def test_rehash_renews_the_batch_numbers(dev):
    """With counters[2] at 2^32 - 1 the table can take one more batch; rehash (same capacity, and twice it) gives
    tables with the same entries whose counts()[2] is the number of chunks that held an entry, and which take a
    put / update / cswap batch with repeats as any young table does.  The old table is left untouched."""
    B, C = 24, 256
    pool = np.concatenate([np.zeros(1, np.uint64), distinct_mbits(170, 8500)])
    rng = np.random.default_rng(8501)
    tab, state = P.DeviceTable(C, B, dev), {}
    for t, what in enumerate(["add", "put", "acc"]):
        one_batch(tab, state, what, pool[rng.integers(0, 150, 500)], rows_for(500, B, 8502 + t), dev)
    set_batch_number(tab, (1 << 32) - 1)
    old_counts = tab.counts()
    slots = tab.entries()[2].cpu().numpy().view(np.uint32).astype(np.int64)
    assert len(slots) == len(state) > 100
    S = 24 + B
    for capacity, chunk_slots in ((C, None), (2 * C, 64), (C, 1)):
        kw = {} if chunk_slots is None else dict(chunk_bytes=chunk_slots * S)
        new = tab.rehash(capacity, **kw)
        chunks = 1 if chunk_slots is None else len(np.unique(slots // chunk_slots))
        assert new.counts()[:3] == (len(state), 0, chunks) and new.capacity == capacity
        model = {k: v.copy() for k, v in state.items()}
        check_table(new, model, pool, dev)
        for t, what in enumerate(["put", "update", "cswap"]):
            mb = pool[rng.integers(0, 171, 400)]
            one_batch(new, model, what, mb, rows_for(400, B, 8510 + t), dev)
            assert new.counts()[:3] == (len(model), 0, chunks + t + 1)
            check_table(new, model, pool, dev)
    assert tab.counts() == old_counts
    check_table(tab, state, pool, dev)
