"""GPU checks of the table's put and get by key (include/pdht_hip_table_keys.h).  The oracle is the record
route at one rank, which this project's other suites pin: bucket_put_records(nranks=1) -> put_records for
the put, bucket_records(nranks=1) -> get -> get_resolve for the get.  Every comparison is byte for byte."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

import table_ref as R  # noqa: E402
from test_gpu_table import forge, rec_to_dev, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xC3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------- helpers ---
def slot_of(L, key_slot=0):
    return key_slot if key_slot else (L + 7) // 8 * 8


def rowbytes_of(L, E, key_slot=0):
    return (slot_of(L, key_slot) + E + 7) // 8 * 8


def rows_of(keys, values, key_slot=0):
    """The rows the contract names: the key, zeros up to the slot, the value, zeros up to 8."""
    n, L = keys.shape
    E = values.shape[1]
    slot = slot_of(L, key_slot)
    rows = np.zeros((n, rowbytes_of(L, E, key_slot)), np.uint8)
    rows[:, :L] = keys
    rows[:, slot:slot + E] = values
    return rows


def keys_with_repeats(n, L, seed):
    """n keys of L bytes, about a quarter of them repeats of earlier ones (more where L = 1 has no room)."""
    rng = np.random.default_rng(seed * 1009 + n * 31 + L)
    nd = max(1, n - n // 4)
    distinct = rng.integers(0, 256, (nd, L), dtype=np.uint8)
    pick = np.concatenate([np.arange(nd), rng.integers(0, nd, n - nd)])
    return distinct[pick[rng.permutation(n)]]


def values_for(n, E, seed):
    return np.random.default_rng(seed * 7919 + n * 13 + E).integers(0, 256, (n, E), dtype=np.uint8)


def keys_at(keys, dev, off=0):
    """Packed keys on the device, `off` bytes past a 16-byte aligned address."""
    n, L = keys.shape
    buf = torch.zeros(n * L + off + 16, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    out = buf[off:off + n * L].view(n, L)
    out.copy_(to_dev(keys, dev))
    return out


LAYOUTS = ("packed", "slice", "odd")


def values_at(values, dev, layout):
    """[n, E] on the device: packed on an aligned base, a column slice of a wider tensor (the row stride is
    E + 11), or packed from a base at byte offset 1.  The bytes around the rows are SENTINEL."""
    n, E = values.shape
    if layout == "packed":
        out = torch.full((n, E), SENTINEL, dtype=torch.uint8, device=dev)
    elif layout == "slice":
        out = torch.full((n, E + 11), SENTINEL, dtype=torch.uint8, device=dev)[:, 5:5 + E]
    else:
        buf = torch.full((n * E + 17,), SENTINEL, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 16 == 0
        out = buf[1:1 + n * E].view(n, E)
    out.copy_(to_dev(values, dev))
    return out


def record_put(tab, keys_d, values_d, key_slot=0):
    """The oracle of put_keys: the record route at one rank."""
    rec, offs = P.bucket_put_records(keys_d.contiguous(), values_d, 1, key_slot=key_slot)
    assert offs.cpu().tolist() == [0, keys_d.shape[0]]
    return tab.put_records(rec), rec


def record_get(tab, keys_d, E, key_slot=0, values=None, status=None):
    """The oracle of get_keys: bucket_records -> get (head 8) -> get_resolve."""
    L = keys_d.shape[1]
    rec, _ = P.bucket_records(keys_d, 1)
    rep = tab.get(rec, head=8)
    return P.get_resolve(rep, keys_d, E, head=8, key_slot=key_slot, index=P.record_fields(rec, L)[3], values=values,
                         status=status)


def entries_of(tab):
    """mbits -> (row bytes, slot): slot order may differ between two inserting runs, the map may not."""
    mb, rows, slots = tab.entries()
    mb, rows, slots = mb.cpu().numpy().view(np.uint64), rows.cpu().numpy(), slots.cpu().numpy()
    out = {int(k): (r.tobytes(), int(s)) for k, r, s in zip(mb, rows, slots)}
    assert len(out) == len(mb)
    return out


def rows_only(entries):
    return {k: v[0] for k, v in entries.items()}


def walk_cost(entries, mbits, capacity):
    """The slots a put of `mbits`, all present, inspects: for each its displacement from home + 1."""
    return sum(1 + ((entries[int(k)][1] - R.home_high(int(k), capacity)) & (capacity - 1)) for k in mbits)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


# ------------------------------------------------- 1. parity with the record route ---
KEYSIZES = (1, 7, 8, 13, 16, 17, 32, 33, 64)  # both sides of every CityHash64 branch edge, k-mer, madkey_t
NS = (1, 63, 64, 65, 1000)


@pytest.mark.parametrize("E", [1, 8, 24])
@pytest.mark.parametrize("L", KEYSIZES)
def test_put_keys_equals_the_record_route(dev, oracle, L, E):
    """Table A by put_keys, table B by bucket_put_records(nranks=1) -> put_records: status, counts()[:3] and
    the entries (mbits -> row) are equal, mbits_out is the oracle's CityHash64, the state is table_ref's.  The
    keys come from an aligned base (the vector classes of 8 / 16 / 32 / 64 bytes), from byte offset 1 and from
    byte offset 8, the values in the three layouts.
    A second put of the same keys finds every mbits present, so it inspects for each key exactly its
    displacement + 1, a number no schedule changes: on table A a put_keys and a put_records of the same
    records add the same to counts()[3], and on each table that sum is the one its own slots give (between
    the two tables the slots inside a cluster may differ, which is why the exact comparison is made on
    one)."""
    C = 2048
    for key_slot in (0, 32, 64):
        if key_slot and key_slot < L:
            continue
        B = rowbytes_of(L, E, key_slot)
        for n in NS:
            for off, layout in ((0, "packed"), (1, "odd"), (8, "slice")):
                if n in (63, 65) and off == 8:
                    continue
                keys, vals = keys_with_repeats(n, L, key_slot + off), values_for(n, E, off)
                kd, vd = keys_at(keys, dev, off), values_at(vals, dev, layout)
                ta, tb = P.DeviceTable(C, B, dev), P.DeviceTable(C, B, dev)
                st_a, mb = ta.put_keys(kd, vd, key_slot=key_slot, mbits=True)
                assert P.last_kernel() == f"k_table_claim_keys+k_table_write_keys<{16 if B % 16 == 0 else 8}>"
                st_b, rec = record_put(tb, kd, vd, key_slot)
                assert torch.equal(st_a, st_b)
                assert ta.counts()[:3] == tb.counts()[:3]
                ea, eb = entries_of(ta), entries_of(tb)
                assert rows_only(ea) == rows_only(eb)
                want_mb = oracle.city64_fixed(keys)
                assert (u64(mb) == want_mb).all()
                want_st, (sk, sr) = R.put_ref(want_mb, rows_of(keys, vals, key_slot))
                assert (st_a.cpu().numpy() == want_st).all()
                assert rows_only(ea) == {int(k): r.tobytes() for k, r in zip(sk, sr)}
                assert ta.counts()[:3] == (len(sk), 0, 1)
                # the second put: every mbits is present
                seen = ta.counts()[3]
                assert torch.equal(ta.put_keys(kd, vd, key_slot=key_slot), st_a)
                by_keys = ta.counts()[3] - seen
                ta.put_records(rec)
                by_records = ta.counts()[3] - seen - by_keys
                assert by_keys == by_records == walk_cost(ea, want_mb, C)
                seen = tb.counts()[3]
                tb.put_records(rec)
                assert tb.counts()[3] - seen == walk_cost(eb, want_mb, C)
                assert rows_only(entries_of(ta)) == rows_only(ea) and ta.counts()[:3] == (len(sk), 0, 3)


# ------------------------------------------------- 2. get_keys against get -> get_resolve ---
@pytest.mark.parametrize("E", [1, 4, 8, 16])
@pytest.mark.parametrize("L", [1, 8, 13, 16, 32, 64])
def test_get_keys_equals_get_and_resolve(dev, oracle, L, E):
    """On one table: present keys, absent keys, repeats of both and a planted collision -- a record put under
    CityHash64(keyA) whose key slot holds another key, so that get_keys(keyA) answers 3.  values start as
    SENTINEL: rows with status 2 or 3 keep it, and so do the bytes between the rows of a slice."""
    rng = np.random.default_rng(L * 100 + E)
    n_have = 150 if L > 1 else 100
    pool = np.unique(rng.integers(0, 256, (400, L), dtype=np.uint8), axis=0)
    pool = pool[rng.permutation(len(pool))]
    have, key_a, other, absent = pool[:n_have], pool[n_have], pool[n_have + 1], pool[n_have + 2:n_have + 40]
    B = rowbytes_of(L, E)
    tab = P.DeviceTable(512, B, dev)
    vals = values_for(n_have, E, 3)
    st = tab.put_keys(keys_at(have, dev), to_dev(vals, dev))
    assert (st == 0).all()
    mb_a = oracle.city64_fixed(key_a[None])
    planted = rows_of(other[None], values_for(1, E, 4))
    assert (tab.put_records(rec_to_dev(forge(mb_a, planted, 24 + B), dev)) == 0).all()
    ask = np.concatenate([have, absent, key_a[None], have[:40], absent[:5], key_a[None]])
    ask = ask[rng.permutation(len(ask))]
    n = len(ask)
    is_a = (ask == key_a).all(axis=1)
    where = {k.tobytes(): i for i, k in enumerate(have)}
    want_st = np.array([3 if a else 0 if k.tobytes() in where else 2 for k, a in zip(ask, is_a)], np.uint8)
    want = np.full((n, E), SENTINEL, np.uint8)
    for i, k in enumerate(ask):
        if want_st[i] == 0:
            want[i] = vals[where[k.tobytes()]]
    for off in (0, 1, 8):
        kd = keys_at(ask, dev, off)
        for layout in LAYOUTS:
            got = values_at(np.full((n, E), SENTINEL, np.uint8), dev, layout)
            ref = values_at(np.full((n, E), SENTINEL, np.uint8), dev, layout)
            whole_got, whole_ref = got._base if got._base is not None else got, ref._base if ref._base is not None else ref
            mb = torch.empty(n, dtype=torch.int64, device=dev)
            v, s = tab.get_keys(kd, E, values=got, status=torch.full((n,), 9, dtype=torch.uint8, device=dev), mbits=mb)
            vstride = got.stride(0) if n > 1 else E
            piece = next(p for p in (16, 8, 4, 1) if (B | slot_of(L) | got.data_ptr() | vstride | E) % p == 0)
            assert P.last_kernel() == f"k_table_get_keys<{piece}>"
            rv, rs = record_get(tab, kd, E, values=ref, status=torch.full((n,), 9, dtype=torch.uint8, device=dev))
            assert torch.equal(s, rs) and torch.equal(v, rv) and torch.equal(whole_got, whole_ref)
            assert (s.cpu().numpy() == want_st).all() and (v.cpu().numpy() == want).all()
            assert (u64(mb) == oracle.city64_fixed(ask)).all()
    # the defaults of get_resolve: new values start as zeros, new status as 2
    v, s = tab.get_keys(keys_at(ask, dev), E)
    assert (s.cpu().numpy() == want_st).all()
    assert (v.cpu().numpy() == np.where((want_st == 0)[:, None], want, 0)).all()
    assert tab.counts()[2] == 2  # a get takes no batch number


# ------------------------------------------------------------ 3. wide rows ---
# (L, eight-byte pieces of the row).  The put moves 16-byte pieces when rowbytes is a multiple of 16, so 130
# words are its 65 pieces; with L = 16 and 132 words the value alone is 65 sixteen-byte pieces for the get.
@pytest.mark.parametrize("L,words", [(8, 63), (8, 64), (8, 65), (8, 129), (16, 130), (16, 132)])
def test_wide_rows(dev, oracle, L, words):
    B = 8 * words
    E = B - slot_of(L)
    n, C = 130, 256
    keys, vals = keys_with_repeats(n, L, words), values_for(n, E, words)
    ask = np.concatenate([keys, np.random.default_rng(words).integers(0, 256, (9, L), dtype=np.uint8)])
    for off, layout in ((0, "packed"), (1, "odd")):
        kd, vd = keys_at(keys, dev, off), values_at(vals, dev, layout)
        ta, tb = P.DeviceTable(C, B, dev), P.DeviceTable(C, B, dev)
        st_a = ta.put_keys(kd, vd)
        assert P.last_kernel() == f"k_table_claim_keys+k_table_write_keys<{16 if words % 2 == 0 else 8}>"
        st_b, _ = record_put(tb, kd, vd)
        assert torch.equal(st_a, st_b) and ta.counts()[:3] == tb.counts()[:3]
        ea = rows_only(entries_of(ta))
        assert ea == rows_only(entries_of(tb))
        want_st, (sk, sr) = R.put_ref(oracle.city64_fixed(keys), rows_of(keys, vals))
        assert (st_a.cpu().numpy() == want_st).all() and ea == {int(k): r.tobytes() for k, r in zip(sk, sr)}
        ad = keys_at(ask, dev, off)
        got = values_at(np.full((len(ask), E), SENTINEL, np.uint8), dev, layout)
        ref = values_at(np.full((len(ask), E), SENTINEL, np.uint8), dev, layout)
        v, s = ta.get_keys(ad, E, values=got)
        piece = next(p for p in (16, 8, 4, 1) if (B | slot_of(L) | got.data_ptr() | E) % p == 0)
        assert P.last_kernel() == f"k_table_get_keys<{piece}>"  # (odd: bytes, 488 .. 1040 pieces a value)
        rv, rs = record_get(tb, ad, E, values=ref)
        assert torch.equal(s, rs) and torch.equal(v, rv)
        assert s[:n].eq(0).all() and s[n:].eq(2).all() and v[n:].eq(SENTINEL).all()


# ------------------------------------------------------------ 4. overflow ---
@pytest.mark.parametrize("L,E", [(13, 8), (32, 24)])
def test_overflow(dev, oracle, L, E):
    """Capacity 64: 20 present keys, then a batch of 200 new keys, the present ones and repeats of both."""
    C, B = 64, rowbytes_of(L, E)
    rng = np.random.default_rng(L)
    pool = np.unique(rng.integers(0, 256, (400, L), dtype=np.uint8), axis=0)
    pool = pool[rng.permutation(len(pool))]
    present, new = pool[:20], pool[20:220]
    tab = P.DeviceTable(C, B, dev)
    assert (tab.put_keys(keys_at(present, dev), to_dev(values_for(20, E, 1), dev)) == 0).all()
    keys = np.concatenate([new, present, new[:50], present[:10]])
    keys = keys[rng.permutation(len(keys))]
    n = len(keys)
    vals = values_for(n, E, 2)
    mbits = oracle.city64_fixed(keys)
    assert len(np.unique(mbits)) == 220  # no collision among the test's keys
    before = tab.counts()
    st, mb = tab.put_keys(keys_at(keys, dev, 1), to_dev(vals, dev), mbits=True)
    st = st.cpu().numpy()
    assert (u64(mb) == mbits).all()
    after = tab.counts()
    was_present = np.isin(mbits, oracle.city64_fixed(present))
    assert not (st[was_present] == 2).any()                       # no present key is dropped
    assert int((st == 2).sum()) == after[1] - before[1] > 0       # the drops are the counter's growth
    assert after[0] == 64 and after[2] == before[2] + 1
    ent = rows_only(entries_of(tab))
    assert len(ent) == 64
    lost = set(mbits[st == 2].tolist())
    assert not lost & set(mbits[st != 2].tolist())                # all records of one mbits share the fate
    assert set(ent) == set(mbits.tolist()) - lost
    rows = rows_of(keys, vals)
    last = {int(k): p for p, k in enumerate(mbits)}               # the last record of every mbits
    for k, row in ent.items():
        assert row == rows[last[k]].tobytes()
    assert sorted(np.flatnonzero(st == 0).tolist()) == sorted(last[k] for k in ent)
    assert ((st == 1) == ~np.isin(np.arange(n), list(last.values())) & (st != 2)).all()
    v, s = tab.get_keys(keys_at(keys, dev), E)
    s = s.cpu().numpy()
    assert ((s == 0) == (st != 2)).all() and ((s == 2) == (st == 2)).all()
    stored = np.array([last[int(k)] for k in mbits])
    assert (v.cpu().numpy()[s == 0] == vals[stored[s == 0]]).all()


# ------------------------------------------------------------ 5. grid-stride ---
def test_grid_stride(dev, oracle):
    """One batch past the reach of every launch, so that each grid-stride loop runs a second round, the last
    one with part of a wave past the end.  table_grid caps a grid at 8 workgroups per CU of kBlock = 256 lanes
    = 4 waves; with 13-byte keys and 8-byte values (slot 16, rowbytes 24) one round of the whole grid covers
      k_table_claim_keys     one key per lane                                             cus * 8 * 256
      k_table_write_keys<8>  np = 3 pieces: groups of 4 lanes, 16 keys per wave
                             x kRowsInFlight = 4                                           cus * 8 * 4 * 64
      k_table_get_keys<8>    np = 1, the 13-byte key at 4 bytes a lane: groups of 4 lanes,
                             16 keys per wave                                              cus * 8 * 4 * 16
    keys."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    m = cus * 8 * 1024 + 4097
    assert m > cus * 8 * 256 and m > cus * 8 * 4 * 64 and m > cus * 8 * 4 * 16
    assert m % 64 != 0 and m < 1 << 24
    L, E, C, nd = 13, 8, 1 << 20, 300000
    B = rowbytes_of(L, E)
    rng = np.random.default_rng(5)
    distinct = np.unique(rng.integers(0, 256, (nd + 64, L), dtype=np.uint8), axis=0)[:nd]
    assert len(distinct) == nd
    dmb = oracle.city64_fixed(distinct)
    assert len(np.unique(dmb)) == nd
    pick = np.concatenate([np.tile(np.arange(nd), m // nd), np.arange(m % nd)])[rng.permutation(m)]
    keys, mbits = distinct[pick], dmb[pick]
    vals = rng.integers(0, 256, (m, E), dtype=np.uint8)
    want_st, (sk, sr) = R.put_ref(mbits, rows_of(keys, vals))
    tab = P.DeviceTable(C, B, dev)
    kd = keys_at(keys, dev, 1)
    st, mb = tab.put_keys(kd, to_dev(vals, dev), mbits=True)
    assert P.last_kernel() == "k_table_claim_keys+k_table_write_keys<8>"
    assert torch.equal(st.cpu(), torch.from_numpy(want_st))
    assert (u64(mb) == mbits).all()
    assert tab.counts()[:3] == (nd, 0, 1)
    emb, erows, _ = tab.entries()
    order = np.argsort(u64(emb))
    assert (u64(emb)[order] == sk).all() and (erows.cpu().numpy()[order] == sr).all()
    absent = rng.integers(0, 256, (4097, L), dtype=np.uint8)
    absent = absent[~np.isin(oracle.city64_fixed(absent), dmb)]
    ask = np.concatenate([keys, absent])
    v, s = tab.get_keys(keys_at(ask, dev, 1), E)
    assert P.last_kernel() == "k_table_get_keys<8>"
    rep = R.replies_ref((sk, sr), np.concatenate([mbits, oracle.city64_fixed(absent)]), 8, B)
    assert (s.cpu().numpy() == np.where(rep[:, 0] == 1, 0, 2)).all()
    assert (v.cpu().numpy() == rep[:, 8 + slot_of(L):8 + slot_of(L) + E]).all()  # zeros where absent: the default


# ------------------------------------------------------------ 6. graph capture ---
def test_put_keys_and_get_keys_capture_into_a_graph(dev, oracle):
    """One put_keys and one get_keys captured on a side stream, one linear chain; replayed twice."""
    L, E, n, C = 13, 8, 300, 1024
    B = rowbytes_of(L, E)
    keys, vals = keys_with_repeats(n, L, 6), values_for(n, E, 6)
    kd, vd = keys_at(keys, dev, 1), to_dev(vals, dev)
    tab = P.DeviceTable(C, B, dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    ws = torch.empty(P.table_put_keys_workspace_bytes(n), dtype=torch.uint8, device=dev)
    mb = torch.empty(n, dtype=torch.int64, device=dev)
    out = torch.empty((n, E), dtype=torch.uint8, device=dev)
    gst = torch.empty(n, dtype=torch.uint8, device=dev)

    def chain():
        tab.put_keys(kd, vd, status=st, mbits=mb, workspace=ws)
        tab.get_keys(kd, E, values=out, status=gst)

    chain()  # eager
    torch.cuda.synchronize(dev)
    base = tab.counts()
    assert base[2] == 1
    want_st, (sk, sr) = R.put_ref(oracle.city64_fixed(keys), rows_of(keys, vals))
    assert (st.cpu().numpy() == want_st).all() and gst.eq(0).all()
    s = torch.cuda.Stream(device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain()
    assert tab.counts()[2] == base[2]  # capture runs nothing
    seen = []
    for k in (1, 2):
        for t in (st, out, gst):
            t.fill_(9)
        mb.fill_(9)
        g.replay()
        torch.cuda.synchronize(dev)
        seen.append((st.clone(), mb.clone(), out.clone(), gst.clone()))
        entries, dropped, nb, _ = tab.counts()
        assert (entries, dropped, nb) == (len(sk), 0, base[2] + k)
    for a, b in zip(*seen):
        assert torch.equal(a, b)
    st2, mb2, out2, gst2 = seen[1]
    assert (st2.cpu().numpy() == want_st).all() and (u64(mb2) == oracle.city64_fixed(keys)).all()
    assert gst2.eq(0).all()
    last = {int(k): p for p, k in enumerate(oracle.city64_fixed(keys))}
    assert (out2.cpu().numpy() == vals[[last[int(k)] for k in oracle.city64_fixed(keys)]]).all()


# ------------------------------------------------------------ 7. mixing ---
def test_keyed_and_record_calls_mix_on_one_table(dev, oracle):
    """A table filled by put_keys answers get, cswap and update_records by mbits_out as the record-filled
    table does; a table filled by put_records answers get_keys."""
    L, E, n, C = 13, 16, 500, 1024
    B = rowbytes_of(L, E)
    slot = slot_of(L)
    keys, vals = keys_with_repeats(n, L, 7), values_for(n, E, 7)
    kd, vd = keys_at(keys, dev, 1), to_dev(vals, dev)
    ta, tb = P.DeviceTable(C, B, dev), P.DeviceTable(C, B, dev)
    st, mb = ta.put_keys(kd, vd, mbits=True)
    st_b, rec = record_put(tb, kd, vd)
    assert torch.equal(st, st_b)
    assert torch.equal(mb, P.put_record_fields(rec, L, E)[4])
    absent = to_dev(np.array([3, 5, 7], np.uint64).view(np.int64), dev)
    ask = torch.cat([mb, absent])
    assert torch.equal(ta.get(ask), tb.get(ask))
    assert torch.equal(ta.get(ask, head=1), tb.get(ask, head=1))
    # cswap on the first word of the value: the first request of an mbits whose word is `compare` wins
    word = int(np.ascontiguousarray(vals[-1]).view(np.uint64)[0])
    ra, rb = ta.cswap(ask, slot, word, 0x1234), tb.cswap(ask, slot, word, 0x1234)
    assert torch.equal(ra, rb) and int(ra[:, 0].sum()) == n
    assert rows_only(entries_of(ta)) == rows_only(entries_of(tb))
    # update by mbits_out: new rows under the digests the keyed put returned, and three absent ones
    umb = np.concatenate([u64(mb)[::3], np.array([3, 5, 7], np.uint64)])
    urec = rec_to_dev(forge(umb, values_for(len(umb), B, 8), 24 + B), dev)
    ua, ub = ta.update_records(urec), tb.update_records(urec)
    assert torch.equal(ua, ub) and ua[-3:].eq(3).all()
    assert rows_only(entries_of(ta)) == rows_only(entries_of(tb))
    assert ta.counts()[:3] == tb.counts()[:3]
    # a record-filled table answers get_keys: the keys it was filled from, and the updated rows' keys collide or not
    tc = P.DeviceTable(C, B, dev)
    record_put(tc, kd, vd)
    more = np.concatenate([keys, values_for(20, L, 9)])
    md = keys_at(more, dev, 1)
    v, s = tc.get_keys(md, E)
    rv, rs = record_get(tc, md, E)
    assert torch.equal(v, rv) and torch.equal(s, rs) and s[:n].eq(0).all()
    last = {int(k): p for p, k in enumerate(u64(mb))}
    assert (v[:n].cpu().numpy() == vals[[last[int(k)] for k in u64(mb)]]).all()
    v, s = tb.get_keys(md, E)  # after the update: whatever key bytes the forged rows hold, both routes agree
    rv, rs = record_get(tb, md, E)
    assert torch.equal(v, rv) and torch.equal(s, rs)
