"""GPU checks of the device-resident table (include/pdht_hip_table.h): batch
put, get and resolve, bit-exact against a Python dict that restates the
reference's server loop --
  put  libmpipdht/init.c:223-241  find by mbits, insert if absent, overwrite the entry;
  get  libmpipdht/init.c:192-220  find by mbits, reply {status, entry} or status 0;
  client libmpipdht/putget.c:50-59  NotFound / Collision / copy the value
-- applied to the records one after the other in batch order.  Records are
forged with numpy (mbits chosen freely; the header words the table must not
read hold noise), except in the end-to-end case."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

pytestmark = pytest.mark.gpu

ROWBYTES = (8, 16, 40, 64, 288)
MS = (0, 1, 63, 65, 4097)
ALL_ONES = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def splitmix64(i):
    z = (np.asarray(i, np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def forge(mbits, rows, stride, seed=0):
    """Put records [m, stride]: noise in type / rank / ht_index / index and in the pad, mbits at +16, the
    row at +24."""
    m, B = rows.shape
    rec = np.random.default_rng(1000 + seed + m).integers(0, 256, (m, stride), dtype=np.uint8)
    rec[:, 16:24] = np.asarray(mbits, np.uint64).view(np.uint8).reshape(m, 8)
    rec[:, 24:24 + B] = rows
    return rec


def rec_to_dev(rec, dev):
    """On the device in int64 storage (8-byte aligned)."""
    m, S = rec.shape
    buf = torch.empty(max(m * S // 8, 1), dtype=torch.int64, device=dev).view(torch.uint8)[:m * S].view(m, S)
    buf.copy_(to_dev(rec, dev))
    return buf


class Model:
    """The reference's table: a dict keyed by mbits.  `capacity` ordinary entries; mbits 0 has the
    implementation's private slot, so it never competes for one."""

    def __init__(self, capacity):
        self.capacity, self.d, self.dropped, self.batches = capacity, {}, 0, 0

    def put(self, mbits, rows):
        m = len(mbits)
        status = np.zeros(m, np.uint8)
        stored = []
        for p in range(m):  # init.c:223-241, one message after the other
            k = int(mbits[p])
            if k not in self.d and k != 0 and sum(1 for x in self.d if x != 0) >= self.capacity:
                status[p] = 2
                self.dropped += 1
                continue
            self.d[k] = (p, rows[p])
            stored.append(p)
        for p in stored:  # superseded by a later record of this batch
            if self.d[int(mbits[p])][0] != p:
                status[p] = 1
        self.d = {k: (-1, v[1]) for k, v in self.d.items()}
        self.batches += 1 if m else 0
        return status

    def put_fast(self, mbits, rows):
        """The same for a batch that cannot overflow."""
        m = len(mbits)
        _, first_rev = np.unique(mbits[::-1], return_index=True)
        last = m - 1 - first_rev
        status = np.ones(m, np.uint8)
        status[last] = 0
        for p in last:
            self.d[int(mbits[p])] = (-1, rows[p])
        self.batches += 1 if m else 0
        return status

    def replies(self, mbits, head, B):
        out = np.zeros((len(mbits), head + B), np.uint8)  # init.c:192-220: status 0 and nothing else
        for p, k in enumerate(mbits):
            e = self.d.get(int(k))
            if e is not None:
                out[p, 0] = 1
                out[p, head:] = e[1]
        return out


def check_get(tab, model, q, dev, records=None):
    """Every reply form for the requests q: head 8 and 1, dense mbits and (when given) records read in place,
    a padded reply stride and, for head 1, a reply buffer at an odd address; pad bytes keep their pattern."""
    B, m = tab.rowbytes, len(q)
    qd = to_dev(np.asarray(q, np.uint64).view(np.int64), dev)
    for head in (8, 1):
        want = model.replies(q, head, B)
        got = tab.get(qd, head=head)
        assert tuple(got.shape) == (m, head + B)
        assert P.last_kernel() == ("k_table_get_bytes" if head == 1 else
                                   "k_table_get<16>" if (B // 8 + 1) % 2 == 0 else "k_table_get<8>")
        assert (got.cpu().numpy() == want).all()
        if records is not None:
            assert (tab.get(records, head=head).cpu().numpy() == want).all()
        pad, off = (8, 0) if head == 8 else (3, 1)
        S = head + B + pad
        buf = torch.full((m * S + 16,), 0xA5, dtype=torch.uint8, device=dev)
        out = buf[off:off + m * S].view(m, S)[:, :head + B]
        tab.get(qd, head=head, out=out)
        d = buf.cpu().numpy()
        body = d[off:off + m * S].reshape(m, S)
        assert (body[:, :head + B] == want).all()
        assert (body[:, head + B:] == 0xA5).all() and (d[:off] == 0xA5).all() and (d[off + m * S:] == 0xA5).all()


def distinct_mbits(n, seed):
    mb = splitmix64(np.arange(n, dtype=np.uint64) + np.uint64(seed << 32))
    assert len(np.unique(mb)) == n and (n == 0 or mb.min() > 0)
    return mb


def rows_for(m, B, seed):
    return np.random.default_rng(seed * 977 + m * 31 + B).integers(0, 256, (m, B), dtype=np.uint8)


# --------------------------------------------------------------- basic put ---
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("B", ROWBYTES)
def test_put_then_get(dev, B, m):
    for extra in (0, 8):
        tab, model = P.DeviceTable(16384, B, dev), Model(16384)
        mb, rows = distinct_mbits(m, 1), rows_for(m, B, 1)
        rec = rec_to_dev(forge(mb, rows, 24 + B + extra), dev)
        st = tab.put_records(rec)
        assert P.last_kernel().startswith("k_table_claim+k_table_write<")
        assert (st.cpu().numpy() == model.put_fast(mb, rows)).all()
        assert tab.counts()[:3] == (m, 0, 1 if m else 0)
        absent = distinct_mbits(37, 2)
        q = np.concatenate([mb, absent])[np.random.default_rng(m).permutation(m + 37)]
        check_get(tab, model, q, dev)
        check_get(tab, model, mb, dev, records=rec)  # in place at +16, the record stride between them


def test_put_moves_16_byte_pieces_when_it_can(dev):
    """Records whose rows start 16-byte aligned (base = 8 mod 16) with a 16-byte stride: k_table_write<16>."""
    B, m, S = 64, 4097, 24 + 64 + 8
    tab, model = P.DeviceTable(16384, B, dev), Model(16384)
    mb, rows = distinct_mbits(m, 3), rows_for(m, B, 3)
    buf = torch.empty(m * S // 8 + 1, dtype=torch.int64, device=dev).view(torch.uint8)[8:8 + m * S].view(m, S)
    buf.copy_(to_dev(forge(mb, rows, S), dev))
    st = tab.put_records(buf)
    assert P.last_kernel() == "k_table_claim+k_table_write<16>"
    assert (st.cpu().numpy() == model.put_fast(mb, rows)).all()
    check_get(tab, model, mb, dev, records=buf)


def test_absent_and_repeated_requests(dev):
    B = 40
    tab, model = P.DeviceTable(16384, B, dev), Model(16384)
    mb, rows = distinct_mbits(500, 4), rows_for(500, B, 4)
    tab.put_records(rec_to_dev(forge(mb, rows, 24 + B), dev), status=False)
    model.put_fast(mb, rows)
    absent = distinct_mbits(300, 5)
    got = tab.get(to_dev(absent.view(np.int64), dev))
    assert int(got.count_nonzero()) == 0  # status 0 and an all-zero reply
    check_get(tab, model, absent, dev)
    rep = np.random.default_rng(6).choice(np.concatenate([mb[:20], absent[:5]]), 4097)  # repeated requests
    check_get(tab, model, rep, dev)
    empty = P.DeviceTable(64, B, dev)  # nothing stored at all
    assert int(empty.get(to_dev(mb.view(np.int64), dev)).count_nonzero()) == 0


@pytest.mark.parametrize("B", ROWBYTES)
def test_mark_values_are_ordinary_keys(dev, B):
    """mbits 0 and 0xFFFF_FFFF_FFFF_FFFF stored, updated and found next to ordinary ones."""
    tab, model = P.DeviceTable(64, B, dev), Model(64)
    marks = np.array([0, ALL_ONES], np.uint64)
    q = np.concatenate([marks, distinct_mbits(10, 7)])
    check_get(tab, model, q, dev)  # absent while the table is empty
    for rnd, mb in enumerate((np.concatenate([distinct_mbits(5, 7), marks]),          # stored
                              np.concatenate([marks, distinct_mbits(7, 7), marks]),    # updated, twice in a batch
                              np.array([0], np.uint64))):
        rows = rows_for(len(mb), B, 10 + rnd)
        st = tab.put_records(rec_to_dev(forge(mb, rows, 24 + B), dev))
        assert (st.cpu().numpy() == model.put(mb, rows)).all()
        check_get(tab, model, q, dev)
    assert tab.counts()[:3] == (9, 0, 3)
    tab.clear()
    assert tab.counts() == (0, 0, 0, 0)
    assert int(tab.get(to_dev(q.view(np.int64), dev)).count_nonzero()) == 0


# --------------------------------------------------------- last writer wins ---
@pytest.mark.parametrize("B", ROWBYTES)
def test_one_mbits_4097_times(dev, B):
    for extra in (0, 8):
        tab = P.DeviceTable(16384, B, dev)
        mb = np.full(4097, 0x1234567890ABCDEF, np.uint64)
        rows = rows_for(4097, B, 20)
        st = tab.put_records(rec_to_dev(forge(mb, rows, 24 + B + extra), dev)).cpu().numpy()
        assert (st[:4096] == 1).all() and st[4096] == 0
        assert tab.counts()[:3] == (1, 0, 1)
        got = tab.get(to_dev(mb[:1].view(np.int64), dev)).cpu().numpy()
        assert got[0, 0] == 1 and (got[0, 1:8] == 0).all() and (got[0, 8:] == rows[4096]).all()


@pytest.fixture(scope="module")
def big_batches():
    """100003 records over 20000 distinct mbits, twice (made once, never written)."""
    out = {}
    keys = distinct_mbits(20000, 30)
    for rnd in (0, 1):
        rng = np.random.default_rng(31 + rnd)
        pick = np.concatenate([np.arange(20000), rng.integers(0, 20000, 80003)])
        out[rnd] = keys[rng.permutation(pick)]
    return keys, out


@pytest.mark.parametrize("B", ROWBYTES)
def test_many_writers_per_mbits(dev, big_batches, B):
    keys, batches = big_batches
    for extra in (0, 8):
        tab, model = P.DeviceTable(32768, B, dev), Model(32768)
        for rnd in (0, 1):  # the second batch overwrites the same mbits
            mb = batches[rnd]
            rows = rows_for(len(mb), B, 32 + rnd)
            st = tab.put_records(rec_to_dev(forge(mb, rows, 24 + B + extra), dev))
            assert (st.cpu().numpy() == model.put_fast(mb, rows)).all()
            entries, dropped, nb, _ = tab.counts()
            assert (entries, dropped, nb) == (20000, 0, rnd + 1)
            got = tab.get(to_dev(keys.view(np.int64), dev)).cpu().numpy()
            assert (got == model.replies(keys, 8, B)).all()


# ------------------------------------------------------------ wrap and full ---
@pytest.mark.parametrize("B", ROWBYTES)
def test_full_table_and_wrapping_probes(dev, B):
    for extra in (0, 8):
        S = 24 + B + extra
        tab, model = P.DeviceTable(64, B, dev), Model(64)
        mb = distinct_mbits(64, 40)
        rows = rows_for(64, B, 40)
        st = tab.put_records(rec_to_dev(forge(mb, rows, S), dev))  # fills every slot: some probes wrap
        assert (st.cpu().numpy() == model.put(mb, rows)).all() and (st == 0).all()
        assert tab.counts()[:3] == (64, 0, 1)
        new = distinct_mbits(10, 41)
        nrows = rows_for(10, B, 41)
        st = tab.put_records(rec_to_dev(forge(new, nrows, S), dev))  # no free slot: ends normally
        assert (st.cpu().numpy() == model.put(new, nrows)).all() and (st == 2).all()
        assert tab.counts()[:3] == (64, 10, 2)
        check_get(tab, model, np.concatenate([new, mb]), dev)  # none of the ten is found, the 64 are
        rows2 = rows_for(64, B, 42)
        order = np.random.default_rng(43).permutation(64)
        st = tab.put_records(rec_to_dev(forge(mb[order], rows2, S), dev))  # present mbits are never dropped
        assert (st.cpu().numpy() == model.put(mb[order], rows2)).all() and (st == 0).all()
        assert tab.counts()[:3] == (64, 10, 3)
        check_get(tab, model, np.concatenate([new, mb]), dev)
        # the private slot of mbits 0 is not one of the 64
        z = np.array([0], np.uint64)
        zr = rows_for(1, B, 44)
        st = tab.put_records(rec_to_dev(forge(z, zr, S), dev))
        assert (st.cpu().numpy() == model.put(z, zr)).all() and (st == 0).all()
        assert tab.counts()[:3] == (65, 10, 4)
        check_get(tab, model, np.concatenate([z, new, mb]), dev)


# -------------------------------------------------------- structured digests ---
@pytest.mark.parametrize("kind", ["low16", "mod1024"])
@pytest.mark.parametrize("B", ROWBYTES)
def test_structured_mbits_keep_probes_short(dev, B, kind):
    """mbits that share their low bits (what a rank sees: mbits % nranks == rank) must not share homes.
    A CPU model of linear probing from the multiplicative mix's high bits inspects 1.51 slots per record
    at load 0.5; the bound of 3 leaves 2x for slots inspected again after lost compare-and-swap races.
    Low-bit homes inspect more than 1000."""
    i = np.arange(32768, dtype=np.uint64)
    if kind == "low16":
        mb = (splitmix64(i) << np.uint64(16)) | np.uint64(0x1234)
    else:
        mb = (splitmix64(i) >> np.uint64(12)) * np.uint64(1024) + np.uint64(5)
        assert (mb % np.uint64(1024) == 5).all()
    assert len(np.unique(mb)) == 32768
    for extra in (0, 8):
        tab, model = P.DeviceTable(65536, B, dev), Model(65536)
        rows = rows_for(32768, B, 50)
        rec = rec_to_dev(forge(mb, rows, 24 + B + extra), dev)
        st = tab.put_records(rec)
        assert (st.cpu().numpy() == model.put_fast(mb, rows)).all()
        entries, dropped, nb, probes = tab.counts()
        print(f"{kind} rowbytes {B}: {probes / 32768:.3f} slots inspected per record")
        assert (entries, dropped, nb) == (32768, 0, 1)
        assert 32768 <= probes <= 3 * 32768
        got = tab.get(rec).cpu().numpy()
        assert (got == model.replies(mb, 8, B)).all()


# ------------------------------------------------------------------ resolve ---
def np_resolve(replies, head, slot, keys, index, E, values, status):
    """putget.c:50-59 per reply; scatter_rows + compare + slice in numpy."""
    L = keys.shape[1]
    for p in range(replies.shape[0]):
        i = p if index is None else int(index[p])
        if replies[p, 0] == 0:
            status[i] = 2
        elif (replies[p, head:head + L] != keys[i]).any():
            status[i] = 3
        else:
            status[i] = 0
            values[i] = replies[p, head + slot:head + slot + E]


def forged_replies(m, n, L, E, slot, head, pad, seed):
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 256, (n, L), dtype=np.uint8)
    index = rng.permutation(n)[:m].astype(np.uint32)
    rep = rng.integers(0, 256, (m, head + slot + E + pad), dtype=np.uint8)
    kind = rng.integers(0, 4, m)  # 0 not found, 1 another key (one byte differs), 2-3 found
    rep[:, 0] = kind != 0
    rep[:, head:head + L] = keys[index]
    other = np.flatnonzero(kind == 1)
    rep[other, head + rng.integers(0, L, len(other))] ^= rng.integers(1, 256, len(other)).astype(np.uint8)
    return keys, index, rep


@pytest.mark.parametrize("E", [1, 8, 12, 40, 256])
@pytest.mark.parametrize("L", [8, 13, 32, 64])
def test_get_resolve(dev, L, E):
    for m in (1, 65, 4097):
        n = m + 9
        for head in (1, 8):
            for key_slot in (0, 32):
                if key_slot and key_slot < L:
                    continue
                slot = key_slot if key_slot else (L + 7) // 8 * 8
                keys, index, rep = forged_replies(m, n, L, E, slot, head, 0, L * E + m + head + key_slot)
                kd, rd = to_dev(keys, dev), to_dev(rep, dev)
                want_v = np.full((n, E), 0x5A, np.uint8)
                want_s = np.full(n, 0xEE, np.uint8)
                np_resolve(rep, head, slot, keys, index, E, want_v, want_s)
                # a dense index
                vals = torch.full((n, E), 0x5A, dtype=torch.uint8, device=dev)
                stat = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
                v, s = P.get_resolve(rd, kd, E, head=head, key_slot=key_slot,
                                     index=to_dev(index.view(np.int32), dev), values=vals, status=stat)
                assert P.last_kernel().startswith("k_get_resolve<")
                assert (s.cpu().numpy() == want_s).all()
                assert (v.cpu().numpy() == want_v).all()  # rows whose status is not 0 keep the pattern
                # the index in place at +12 of the client's own record batch, values row-strided
                rb = P.bucket_record_bytes(L)
                recs = np.zeros((m, rb), np.uint8)
                recs[:, 12:16] = index.view(np.uint8).reshape(m, 4)
                ix = P.record_fields(to_dev(recs, dev), L)[3]
                wide = torch.full((n, E + 24), 0x5A, dtype=torch.uint8, device=dev)
                stat.fill_(0xEE)
                v, s = P.get_resolve(rd, kd, E, head=head, key_slot=key_slot, index=ix, values=wide[:, 8:8 + E],
                                     status=stat)
                assert (s.cpu().numpy() == want_s).all()
                w = wide.cpu().numpy()
                assert (w[:, 8:8 + E] == want_v).all() and (w[:, :8] == 0x5A).all() and (w[:, 8 + E:] == 0x5A).all()
                # index=None: reply p answers key p; new outputs start as zeros / NotFound
                want_v0 = np.zeros((n, E), np.uint8)
                want_s0 = np.full(n, 2, np.uint8)
                np_resolve(rep, head, slot, keys[index], None, E, want_v0, want_s0)
                kp = np.concatenate([keys[index], keys[:n - m]])
                v, s = P.get_resolve(rd, to_dev(kp, dev), E, head=head, key_slot=key_slot)
                assert (s.cpu().numpy() == want_s0).all() and (v.cpu().numpy() == want_v0).all()


# ---------------------------------------------------------------- collision ---
def test_collision_is_by_mbits_alone(dev):
    """init.c keys entries by mbits alone: two different keys forged with one mbits share an entry, the
    second overwrites, and the client tells them apart by the key in the reply."""
    L, E = 8, 8
    B = 16
    tab = P.DeviceTable(64, B, dev)
    k1, k2, k3 = (np.frombuffer(s, np.uint8) for s in (b"first___", b"second__", b"absent__"))
    v1, v2 = np.arange(8, dtype=np.uint8), np.arange(8, 16, dtype=np.uint8)
    mb = np.array([77, 77], np.uint64)
    st = tab.put_records(rec_to_dev(forge(mb, np.stack([np.concatenate([k1, v1]), np.concatenate([k2, v2])]),
                                          24 + B), dev))
    assert st.cpu().tolist() == [1, 0] and tab.counts()[:3] == (1, 0, 1)
    replies = tab.get(to_dev(np.array([77, 77, 78], np.uint64).view(np.int64), dev))
    values, status = P.get_resolve(replies, to_dev(np.stack([k1, k2, k3]), dev), E)
    assert status.cpu().tolist() == [3, 0, 2]  # Collision, OK, NotFound (pdht.h:199-204)
    assert (values.cpu().numpy() == np.stack([np.zeros(8, np.uint8), v2, np.zeros(8, np.uint8)])).all()


# --------------------------------------------------------------- end to end ---
@pytest.mark.parametrize("L,E,key_slot", [(8, 8, 0), (13, 40, 32)])
def test_put_get_resolve_end_to_end(dev, L, E, key_slot):
    n, extra = 20011, 1000
    rng = np.random.default_rng(L * 100 + E)
    allk = np.unique(rng.integers(0, 256, (n + extra + 64, L), dtype=np.uint8), axis=0)
    allk = allk[rng.permutation(len(allk))][:n + extra]
    keys, never = allk[:n], allk[n:]
    values = rng.integers(0, 256, (n, E), dtype=np.uint8)
    records, _ = P.bucket_put_records(to_dev(keys, dev), to_dev(values, dev), 7, key_slot=key_slot)
    tab = P.DeviceTable(65536, records.shape[1] - 24, dev)
    st = tab.put_records(records)  # all seven buckets arrive at the one table
    assert int(st.count_nonzero()) == 0 and tab.counts()[:3] == (n, 0, 1)
    order = rng.permutation(n + extra)
    keys2 = np.concatenate([keys, never])[order]
    k2d = to_dev(keys2, dev)
    get_records, _ = P.bucket_records(k2d, 7, msg_type=0)
    replies = tab.get(get_records)
    sentinel = torch.full((n + extra, E), 0xC3, dtype=torch.uint8, device=dev)
    vals, status = P.get_resolve(replies, k2d, E, key_slot=key_slot, index=P.record_fields(get_records, L)[3],
                                 values=sentinel)
    was_put = order < n
    want = np.full((n + extra, E), 0xC3, np.uint8)
    want[was_put] = values[order[was_put]]
    assert (status.cpu().numpy() == np.where(was_put, 0, 2)).all()
    assert (vals.cpu().numpy() == want).all()  # in keys2's order


# ------------------------------------------------------------ graph capture ---
def test_put_and_get_in_a_graph(dev):
    B, m = 40, 1000
    tab, model = P.DeviceTable(4096, B, dev), Model(4096)
    rng = np.random.default_rng(60)
    mb = distinct_mbits(300, 60)[rng.permutation(np.concatenate([np.arange(300), rng.integers(0, 300, m - 300)]))]
    rows = rows_for(m, B, 60)
    rec = rec_to_dev(forge(mb, rows, 24 + B), dev)
    want_st = model.put_fast(mb, rows)
    q = to_dev(np.concatenate([mb, distinct_mbits(24, 61)]).view(np.int64), dev)
    st = torch.empty(m, dtype=torch.uint8, device=dev)
    ws = torch.empty(4 * m, dtype=torch.uint8, device=dev)
    out = torch.empty((m + 24, 8 + B), dtype=torch.uint8, device=dev)
    tab.put_records(rec, status=st, workspace=ws)  # eager
    eager_st, eager = st.clone(), tab.get(q, out=out).clone()
    assert (eager_st.cpu().numpy() == want_st).all()
    base = tab.counts()
    assert base[:3] == (300, 0, 1)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tab.put_records(rec, status=st, workspace=ws)
        tab.get(q, out=out)
    assert tab.counts()[2] == base[2]  # capture runs nothing
    for k in (1, 2):
        st.fill_(9)
        out.fill_(9)
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(st, eager_st) and torch.equal(out, eager)
        entries, dropped, nb, _ = tab.counts()
        assert (entries, dropped, nb) == (300, 0, base[2] + k)
