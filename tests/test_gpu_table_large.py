"""GPU checks of the device-resident table where every byte offset needs 64 bits (include/pdht_hip_table*.h:
geometry goes up to 2^31 slots of rows < 2^31 bytes, and slot * rowbytes, p * record_stride, p * reply_stride
and (base + e) * row_stride are 64-bit products).  A1 puts a table's rows region past 4 GiB and homes mbits
on both sides of byte 2^31 and byte 2^32 of the buffer; A2 keeps the table small and walks records, requests,
replies, exported records and resolved values through buffers of 4.6 GB at a stride of 65536 bytes.  Every
comparison is exact against the sequential dict models (tests/table_*_ref.py).

The choosers (mbits_for_slot, slot_of_byte, chosen_homes, large_keys) run without a GPU:
tests/test_table_ranges_cpu.py proves them against table_ref.home_high and probe_model."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

import table_acc_ref as ACC  # noqa: E402
import table_add_ref as ADD  # noqa: E402
import table_iter_ref as IT  # noqa: E402
import table_ref as R  # noqa: E402
import table_rmw_ref as RMW  # noqa: E402
from test_gpu_table import distinct_mbits, forge, rec_to_dev, rows_for, to_dev  # noqa: E402
from test_gpu_table_edges import rec16_to_dev, with_repeats  # noqa: E402

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
MIX_INV = pow(R.MIX, -1, 1 << 64)  # MIX is odd: the mix is a bijection of the 64-bit words


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------- choosers ---
def mbits_for_slot(slot, capacity, low):
    """The mbits whose home is `slot` and whose mix has `low` in the bits under the home (no search)."""
    k = R.log2_capacity(capacity)
    assert 0 <= slot < capacity and 0 <= low < 1 << (64 - k)
    return ((((slot << (64 - k)) | low) * MIX_INV) & M64)


LARGE_C = 1 << 20
LARGE_B = (8192, 8200)  # 512 16-byte pieces; 1025 8-byte pieces (more than a wave has lanes)


def slot_of_byte(byte, capacity, rowbytes):
    """The slot whose row contains byte `byte` of the table's buffer."""
    rows = IT.layout(capacity, rowbytes)[2]
    assert byte >= rows
    return (byte - rows) // rowbytes


def chosen_homes(capacity, rowbytes):
    """(named, spread): the homes A1 asks for by name, and a handful spread over the upper half -- all distinct,
    no two of the spread ones adjacent to anything, none at slots 1 and 2 (the wrap cluster lands there)."""
    C = capacity
    s31, s32 = slot_of_byte(1 << 31, C, rowbytes), slot_of_byte(1 << 32, C, rowbytes)
    named = [0, s31 - 1, s31, s31 + 1, s32 - 1, s32, s32 + 1, C - 2]
    rng = np.random.default_rng(7000 + rowbytes)
    spread = sorted(int(s) for s in C // 2 + 3 * rng.choice((C // 2 - 1000) // 3, 36, replace=False))
    assert len(set(named + spread)) == len(named) + len(spread) and not {1, 2, C - 1} & set(named + spread)
    assert all(b - a >= 3 for a, b in zip(spread, spread[1:])) and spread[0] > s32 + 1 and spread[-1] < C - 2
    return named, spread


def wrap_mbits(capacity):
    """Three mbits homed at the last ordinary slot: put one after the other (behind the key homed at slot 0) they
    sit at C - 1, 1 and 2."""
    return np.array([mbits_for_slot(capacity - 1, capacity, low) for low in (1, 2, 3)], np.uint64)


def created_homes(capacity, rowbytes, which):
    """Four homes in the upper half per inserting call (which = 0, 1, 2), between the spread ones."""
    _, spread = chosen_homes(capacity, rowbytes)
    free = [s + 1 for s in spread]  # spread homes are >= 3 apart: s + 1 is nobody's home or neighbour's slot
    return free[4 * which:4 * which + 4]


def large_keys(capacity, rowbytes):
    """(main, wrap, slot_of): the mbits of the first put batch (mbits 0 among them), the wrap cluster, and the
    slot every one of them must end in."""
    named, spread = chosen_homes(capacity, rowbytes)
    homes = named + spread
    main = np.array([mbits_for_slot(s, capacity, 0x1000 + i) for i, s in enumerate(homes)] + [0], np.uint64)
    wrap = wrap_mbits(capacity)
    slot_of = {int(k): s for k, s in zip(main[:-1], homes)}
    slot_of[0] = capacity
    slot_of.update({int(k): s for k, s in zip(wrap, (capacity - 1, 1, 2))})
    return main, wrap, slot_of


def below(slot_of, capacity):
    """mbits homed one slot below every chosen slot (slot 0 and the private slot C share C - 1), none of them
    stored."""
    homes = sorted({(s - 1) % capacity for s in slot_of.values()})
    return np.array([mbits_for_slot(s, capacity, 0x7777) for s in homes], np.uint64)


# -------------------------------------------------------------- helpers ---
def i64(mb, dev):
    return to_dev(np.asarray(mb, np.uint64).view(np.int64), dev)


def replies(state, q, head, B):
    out = np.zeros((len(q), head + B), np.uint8)
    for p, k in enumerate(np.asarray(q, np.uint64).tolist()):
        row = state.get(k)
        if row is not None:
            out[p, 0] = 1
            out[p, head:] = row
    return out


def put_model(state, mb, rows):
    """Last writer wins, for a batch that cannot overflow: the status."""
    m = len(mb)
    last = m - 1 - np.unique(mb[::-1], return_index=True)[1]
    want = np.ones(m, np.uint8)
    want[last] = 0
    for p in last:
        state[int(mb[p])] = rows[p].copy()
    return want


def set_last_word(rows, values):
    """The rows with their last 8 bytes replaced by `values` (int64 or float64, one per row)."""
    v = np.ascontiguousarray(values)
    rows[:, -8:] = v.view(np.uint8).reshape(len(rows), 8)
    return rows


# ============================================ A1: the rows region past 4 GiB ===
@pytest.mark.parametrize("B", LARGE_B)
def test_rows_past_4gib(dev, B):
    """2^20 slots of 8192 / 8200 bytes: one table of about 8.6 GB (the peak allocation; allocated, not filled --
    init clears the 16 MB of tags and winner words), freed at the end.  About 60 entries homed at slot 0, around
    the rows that hold bytes 2^31 and 2^32 of the buffer, over the upper half, at C - 2, C - 1 (a cluster that
    wraps to slots 1 and 2) and in mbits 0's private slot C, the highest offset of all.  Every call of the
    table on it against the dict models; at the end nothing is found one slot below any chosen slot."""
    C = LARGE_C
    rng = np.random.default_rng(7100 + B)
    main, wrap, slot_of = large_keys(C, B)
    rows_off = IT.layout(C, B)[2]
    assert rows_off + slot_of[int(main[5])] * B <= 1 << 32 < rows_off + (slot_of[int(main[5])] + 1) * B
    S = 24 + B + (8 if (24 + B) % 16 else 0)
    place = rec16_to_dev if B % 16 == 0 else rec_to_dev
    piece = 16 if B % 16 == 0 else 8
    tab, state, batches = P.DeviceTable(C, B, dev), {}, 0
    assert tab.nbytes > (1 << 33)

    def counted():
        assert tab.counts()[:3] == (len(state), 0, batches)

    # put_records: status and last-wins
    mb = with_repeats(main, 200, rng)
    rows = rows_for(200, B, 7101)
    st = tab.put_records(place(forge(mb, rows, S), dev))
    assert P.last_kernel() == f"k_table_claim+k_table_write<{piece}>"
    assert (st.cpu().numpy() == put_model(state, mb, rows)).all()
    batches += 1
    counted()
    for k in wrap:  # one record per batch: C - 1, then 1, then 2
        row = rows_for(1, B, 7102 + int(k & np.uint64(0xFF)))
        st = tab.put_records(place(forge(np.array([k]), row, S), dev))
        assert st.cpu().tolist() == [0]
        state[int(k)] = row[0].copy()
        batches += 1
        counted()
    keys = np.concatenate([main, wrap])
    absent = np.concatenate([distinct_mbits(9, 7103), below(slot_of, C)])

    def check_get():
        q = np.concatenate([keys, absent, np.array(sorted(set(state) - set(keys.tolist())), np.uint64)])
        for head in (8, 1):
            got = tab.get(i64(q, dev), head=head)
            assert (got.cpu().numpy() == replies(state, q, head, B)).all()
        counted()

    check_get()

    # update_records: present and absent mbits, repeats; the rows end in an integer-valued double
    mb = with_repeats(np.concatenate([keys, absent[:5]]), 200, rng)
    rows = set_last_word(rows_for(200, B, 7104), rng.integers(-(1 << 20), 1 << 20, 200).astype(np.float64))
    st = tab.update_records(place(forge(mb, rows, S), dev))
    assert (st.cpu().numpy() == RMW.update_ref(state, mb, rows)).all()
    batches += 1
    check_get()
    assert all(float(state[int(k)][-8:].view(np.float64)[0]).is_integer() for k in keys)

    # cswap at the first and the last word of the row
    for word_offset in (0, B - 8):
        q = with_repeats(np.concatenate([keys, absent[:5]]), 200, rng)
        hit = int(q[rng.integers(0, 200)]) if word_offset == 0 else int(keys[10])
        while hit not in state:
            hit = int(q[rng.integers(0, 200)])
        compare = int(state[hit][word_offset:word_offset + 8].view(np.uint64)[0])
        desired = int(np.float64(4242.0).view(np.uint64)) if word_offset else 0x0123456789ABCDEF
        got = tab.cswap(i64(q, dev), word_offset, compare, desired)
        assert (got.cpu().numpy() == RMW.cswap_ref(state, q, word_offset, compare, desired)).all()
        batches += 1
        check_get()

    # acc_records on the last element: f64 (integer-valued: bit-exact) then i64, each without and with insert
    vo = B - 8
    created = 0
    for kind, tdt, ndt in (("f64", torch.float64, np.float64), ("i64", torch.int64, np.int64)):
        for insert in (False, True):
            pool = keys
            if insert:
                new = np.array([mbits_for_slot(s, C, 0x2000 + created) for s in created_homes(C, B, created)], np.uint64)
                slot_of.update({int(k): s for k, s in zip(new, created_homes(C, B, created))})
                created += 1
                pool = np.concatenate([keys, new])
            mb = with_repeats(pool, 200, rng)
            if kind == "f64":
                add = rng.integers(-(1 << 20), 1 << 20, 200).astype(np.float64)
            else:
                add = rng.integers(0, 1 << 64, 200, dtype=np.uint64)
            rows = set_last_word(rows_for(200, B, 7105 + created), add)
            st = tab.acc_records(place(forge(mb, rows, S), dev), tdt, vo, 1, insert=insert)
            want, sums = ACC.acc_ref(state, mb, rows, ndt, vo, 1, insert, capacity=C)
            assert (st.cpu().numpy() == want).all() and all(s["seq"] == s["exact"] for s in sums.values())
            batches += insert
            check_get()
    assert created == 2 and len(state) == len(keys) + 8

    # add_records with replies: present mbits and four new ones
    new = np.array([mbits_for_slot(s, C, 0x3000) for s in created_homes(C, B, 2)], np.uint64)
    slot_of.update({int(k): s for k, s in zip(new, created_homes(C, B, 2))})
    mb = with_repeats(np.concatenate([keys, new]), 200, rng)
    rows = rows_for(200, B, 7110)
    st, rep = tab.add_records(place(forge(mb, rows, S), dev), replies=True)
    want, want_rep = ADD.add_ref(state, mb, rows, capacity=C)
    assert (st.cpu().numpy() == want).all() and (rep.cpu().numpy() == want_rep).all()
    batches += 1
    check_get()
    assert set(slot_of) == set(state)

    # entries: a window around the 2^32 crossing, and the whole table, in slot order
    by_slot = sorted(state, key=lambda k: slot_of[k])
    s32 = slot_of_byte(1 << 32, C, B)
    for first, n in ((s32 - 2, 5), (0, None)):
        hi = C + 1 if n is None else first + n
        want_keys = [k for k in by_slot if first <= slot_of[k] < hi]
        mbits, erows, slots = tab.entries(first, n)
        assert mbits.cpu().numpy().view(np.uint64).tolist() == want_keys
        assert slots.cpu().numpy().view(np.uint32).tolist() == [slot_of[k] for k in want_keys]
        assert (erows.cpu().numpy() == np.stack([state[k] for k in want_keys])).all()
    assert [slot_of[k] for k in by_slot[:3]] == [0, 1, 2] and slot_of[by_slot[-1]] == C
    assert tab.export(None).cpu().tolist() == [len(state), 0]  # the count-only form
    counted()

    # nothing landed one slot (or 2 GiB, or 4 GiB) away: the homes below the chosen slots answer "not found"
    q = below(slot_of, C)
    assert not set(q.tolist()) & set(state)
    for head in (8, 1):
        assert int(tab.get(i64(q, dev), head=head).count_nonzero()) == 0
    del tab
    torch.cuda.empty_cache()


# ====================================== A2: buffers past 4 GiB through their strides ===
WIDE_M, WIDE_S = 70000, 65536  # 70000 rows of 65536 bytes: rows 65536 .. 69999 start past 4 GiB
SMALL_C, SMALL_B = 1 << 17, 8


@pytest.fixture(scope="module")
def wide(dev):
    """Two wide uint8 buffers [70000, 65536] of about 4.6 GB each (the peak allocation of the A2 tests, next to
    a 3 MB table): `src` carries what the calls read, `dst` is filled with 0xA5 and receives what they write.
    Freed when the module is done."""
    src = torch.empty((WIDE_M, WIDE_S), dtype=torch.uint8, device=dev)
    dst = torch.full((WIDE_M, WIDE_S), 0xA5, dtype=torch.uint8, device=dev)
    assert src.numel() > (1 << 32) and src.stride(0) == WIDE_S
    yield src, dst
    del src, dst
    torch.cuda.empty_cache()


A5_WORD = int(np.frombuffer(b"\xA5" * 8, np.int64)[0])


def untouched(dst, lo, hi):
    """On the device: every byte of the wide buffer outside the columns [lo, hi) still holds 0xA5 (hi <= 64)."""
    assert 0 <= lo <= hi <= 64
    words = dst.view(torch.int64)  # [m, 8192]
    ok = bool((words[:, 8:] == A5_WORD).all())
    return ok and bool((dst[:, :lo] == 0xA5).all()) and bool((dst[:, hi:64] == 0xA5).all())


def restore(dst, lo, hi):
    dst[:, lo:hi].fill_(0xA5)


def load(src, rec, dev):
    """The records / replies `rec` [m, w] into the first w columns of the wide source; the view of them."""
    view = src[:, :rec.shape[1]]
    view.copy_(to_dev(rec, dev))
    return view


def small_table(dev, keys, rows):
    """A table of 2^17 slots that holds rows[i] under keys[i] (distinct), and the dict state."""
    tab = P.DeviceTable(SMALL_C, SMALL_B, dev)
    tab.put_records(rec_to_dev(forge(keys, rows, 24 + SMALL_B), dev), status=False)
    return tab, {int(k): rows[i].copy() for i, k in enumerate(keys)}


def check_state(tab, state, q, dev):
    got = tab.get(i64(q, dev)).cpu().numpy()
    assert (got == replies(state, q, 8, SMALL_B)).all()
    assert tab.counts()[0] == len(state)


@pytest.fixture(scope="module")
def wide_keys():
    """70000 distinct mbits, 2000 more that no table holds at first, and a shuffle (made once, never written)."""
    keys = distinct_mbits(WIDE_M + 2000, 7200)
    return keys[:WIDE_M], keys[WIDE_M:], np.random.default_rng(7201).permutation(WIDE_M)


def test_records_read_at_a_wide_stride(dev, wide, wide_keys):
    """put_records, update_records, acc_records(insert=True) and add_records read 70000 records at a stride of
    65536 bytes (two wide buffers of about 4.6 GB each are alive, see `wide`): record p >= 65536 lies past
    4 GiB and differs from record p - 65536.  Status exact; the final state through get."""
    src, _ = wide
    keys, extra, perm = wide_keys
    B, m = SMALL_B, WIDE_M
    tab, state = P.DeviceTable(SMALL_C, B, dev), {}
    rows = rows_for(m, B, 7210)
    st = tab.put_records(load(src, forge(keys, rows, 32), dev))
    assert (st.cpu().numpy() == put_model(state, keys, rows)).all() and len(state) == m
    check_state(tab, state, np.concatenate([keys, extra[:64]]), dev)
    # update: another order, the last 1000 records name absent mbits
    mb = np.concatenate([keys[perm][:-1000], extra[:1000]])
    rows = rows_for(m, B, 7211)
    st = tab.update_records(load(src, forge(mb, rows, 32), dev))
    assert (st.cpu().numpy() == RMW.update_ref(state, mb, rows)).all()
    check_state(tab, state, np.concatenate([keys, extra[:64]]), dev)
    # inserting accumulate: 1000 new mbits behind 69000 present ones, in the order reversed
    mb = np.concatenate([keys[perm][1000:], extra[:1000]])[::-1].copy()
    rows = rows_for(m, B, 7212)
    st = tab.acc_records(load(src, forge(mb, rows, 32), dev), torch.int64, 0, 1, insert=True)
    assert (st.cpu().numpy() == ACC.acc_ref(state, mb, rows, np.int64, 0, 1, True, capacity=SMALL_C)[0]).all()
    check_state(tab, state, np.concatenate([keys, extra]), dev)
    # add: the other 1000 new mbits at the END of the batch (past 4 GiB), each twice
    mb = np.concatenate([keys[perm][:-2000], np.repeat(extra[1000:], 2)])
    rows = rows_for(m, B, 7213)
    st = tab.add_records(load(src, forge(mb, rows, 32), dev))
    assert (st.cpu().numpy() == ADD.add_ref(state, mb, rows, capacity=SMALL_C)[0]).all()
    assert len(state) == m + 2000 and tab.counts()[:3] == (m + 2000, 0, 4)
    check_state(tab, state, np.concatenate([keys, extra]), dev)


def test_requests_read_and_replies_written_at_a_wide_stride(dev, wide, wide_keys):
    """get and cswap read their requests in place from records at a stride of 65536 bytes; get (head 8 and 1),
    cswap and add_records write their replies at that stride (two wide buffers of about 4.6 GB each, see
    `wide`).  Replies exact; every byte of the reply buffer outside the reply columns keeps 0xA5."""
    src, dst = wide
    restore(dst, 0, 64)  # whatever an earlier test that failed left behind
    keys, extra, perm = wide_keys
    B, m = SMALL_B, WIDE_M
    tab, state = small_table(dev, keys[:m - 3000], rows_for(m - 3000, B, 7220))
    mb = keys[perm]  # 3000 of them absent, spread over the batch
    rec = load(src, forge(mb, rows_for(m, B, 7221), 32), dev)
    for head in (8, 1):
        want = replies(state, mb, head, B)
        assert (tab.get(rec, head=head).cpu().numpy() == want).all()  # requests in place, dense replies
        out = dst[:, :head + B]
        assert tab.get(i64(mb, dev), head=head, out=out).data_ptr() == dst.data_ptr()  # dense requests, wide replies
        assert (out.cpu().numpy() == want).all() and untouched(dst, 0, head + B)
        restore(dst, 0, head + B)
        tab.get(rec, head=head, out=out)  # both at once
        assert (out.cpu().numpy() == want).all() and untouched(dst, 0, head + B)
        restore(dst, 0, head + B)
    # cswap: requests in place; the word of the entry of mb[69999] swaps, and nothing else equals it
    compare = int(state[int(keys[0])].view(np.uint64)[0])
    model = {k: v.copy() for k, v in state.items()}
    want = RMW.cswap_ref(model, mb, 0, compare, 0x1111111111111111)
    assert (tab.cswap(rec, 0, compare, 0x1111111111111111).cpu().numpy() == want).all()
    state = model
    check_state(tab, state, keys, dev)
    compare = int(state[int(mb[m - 1] if int(mb[m - 1]) in state else keys[1])].view(np.uint64)[0])
    want = RMW.cswap_ref(state, mb, 0, compare, 0x2222222222222222)
    out = dst[:, :16]
    tab.cswap(rec, 0, compare, 0x2222222222222222, out=out)
    assert (out.cpu().numpy() == want).all() and untouched(dst, 0, 16)
    restore(dst, 0, 16)
    check_state(tab, state, keys, dev)
    # add_records: the 3000 absent mbits are created from the wide records, the replies go to the wide buffer
    rows = rows_for(m, B, 7222)
    rec = load(src, forge(mb, rows, 32), dev)
    st, rep = tab.add_records(rec, replies=dst[:, :8 + B])
    want, want_rep = ADD.add_ref(state, mb, rows, capacity=SMALL_C)
    assert (st.cpu().numpy() == want).all() and (want == 0).sum() == 3000
    assert (rep.cpu().numpy() == want_rep).all() and untouched(dst, 0, 8 + B)
    restore(dst, 0, 8 + B)
    check_state(tab, state, np.concatenate([keys, extra[:64]]), dev)


def test_export_records_at_a_wide_stride(dev, wide, wide_keys):
    """export_records into records at a stride of 65536 bytes from a table of 72000 entries: entries 65536 ..
    69999 are written past 4 GiB (two wide buffers of about 4.6 GB each, see `wide`).  Equal to entries()
    taken densely; bytes +0 .. +11 of every record and everything behind +32 keep 0xA5."""
    _, dst = wide
    restore(dst, 0, 64)  # whatever an earlier test that failed left behind
    keys, extra, _ = wide_keys
    B, m = SMALL_B, WIDE_M
    allk = np.concatenate([keys, extra])
    tab, state = small_table(dev, allk, rows_for(len(allk), B, 7230))
    mbits, rows, slots = (t.cpu().numpy() for t in tab.entries())
    assert len(mbits) == len(allk) > 65537 and (np.diff(slots.view(np.uint32).astype(np.int64)) > 0).all()
    assert all((state[int(k)] == r).all() for k, r in zip(mbits.view(np.uint64)[::97], rows[::97]))
    count = tab.export_records(dst[:, :32])
    assert count.cpu().tolist() == [len(allk), m]
    got = dst[:, :32].cpu().numpy()
    assert (got[:, :12] == 0xA5).all() and untouched(dst, 12, 32)
    assert (np.ascontiguousarray(got[:, 12:16]).view(np.int32)[:, 0] == slots[:m]).all()
    assert (np.ascontiguousarray(got[:, 16:24]).view(np.int64)[:, 0] == mbits[:m]).all()
    assert (got[:, 24:32] == rows[:m]).all()
    # a slot range that starts inside the table, too
    first = int(slots.view(np.uint32)[3000])
    count = tab.export_records(dst[:, :32], first_slot=first)
    assert count.cpu().tolist() == [len(allk) - 3000, len(allk) - 3000]
    got = dst[:len(allk) - 3000, :32].cpu().numpy()
    assert (np.ascontiguousarray(got[:, 16:24]).view(np.int64)[:, 0] == mbits[3000:]).all()
    assert (got[:, 24:32] == rows[3000:]).all() and untouched(dst, 12, 32)
    restore(dst, 12, 32)


def test_get_resolve_at_wide_strides(dev, wide):
    """get_resolve with the replies AND the index read at a stride of 65536 bytes (the index in place at +12 of
    the same wide rows, the replies at +32) and the values written at that stride (two wide buffers of about
    4.6 GB each, see `wide`).  Status and values exact; the value buffer keeps 0xA5 everywhere else, also in
    the rows whose status is not 0."""
    src, dst = wide
    restore(dst, 0, 64)  # whatever an earlier test that failed left behind
    m, L, E, head = WIDE_M, 8, 8, 8
    rng = np.random.default_rng(7240)
    keys = rng.integers(0, 256, (m, L), dtype=np.uint8)
    index = rng.permutation(m).astype(np.uint32)
    kind = rng.integers(0, 4, m)  # 0 not found, 1 another key, 2-3 found
    img = rng.integers(0, 256, (m, 32 + head + L + E), dtype=np.uint8)
    img[:, 12:16] = index.view(np.uint8).reshape(m, 4)
    rep = img[:, 32:]
    rep[:, 0] = kind != 0
    rep[:, head:head + L] = keys[index]
    other = np.flatnonzero(kind == 1)
    rep[other, head + rng.integers(0, L, len(other))] ^= 0x40
    want_s = np.empty(m, np.uint8)
    want_s[index] = np.where(kind == 0, 2, np.where(kind == 1, 3, 0))
    want_v = np.full((m, E), 0xA5, np.uint8)
    ok = kind >= 2
    want_v[index[ok]] = rep[ok, head + L:head + L + E]
    view = load(src, img, dev)
    ix = src.view(torch.int32)[:, 3]
    assert ix.stride(0) * 4 == WIDE_S
    status = torch.full((m,), 0xEE, dtype=torch.uint8, device=dev)
    v, s = P.get_resolve(view[:, 32:], to_dev(keys, dev), E, head=head, index=ix, values=dst[:, :E], status=status)
    assert P.last_kernel().startswith("k_get_resolve<")
    assert (s.cpu().numpy() == want_s).all() and (want_s == 0).sum() > 30000 and (want_s[65536:] == 0).any()
    assert (v.cpu().numpy() == want_v).all() and untouched(dst, 0, E)
    restore(dst, 0, E)
