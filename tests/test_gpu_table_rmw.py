"""GPU checks of the table's update and compare-and-swap (include/pdht_hip_table_rmw.h): status, replies
and the table afterwards -- a get of every mbits and the counters -- byte-exact against the sequential
models of tests/table_rmw_ref.py, which apply one record after the other and know nothing of winner
words.  The row copy of an update is k_table_write itself (one added argument), so its piece counts are
those tests/test_gpu_table_edges.py sweeps for the put."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

import table_rmw_ref as R  # noqa: E402
from test_gpu_table import Model, distinct_mbits, forge, rec_to_dev, rows_for, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
UNUSED, USED = 0x0123456789ABCDEF, 0x0FEDCBA987654321


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------- helpers ---
def i64(mb, dev):
    return to_dev(np.asarray(mb, np.uint64).view(np.int64), dev)


def with_word(rows, k, value):
    """rows with their k-th 64-bit word set to value."""
    rows = rows.copy()
    rows[:, 8 * k:8 * k + 8] = np.frombuffer(int(value & M64).to_bytes(8, "little"), np.uint8)
    return rows


def filled(dev, capacity, B, mb, rows):
    """A table that holds rows[i] under mb[i] (distinct) after one put, and its state for the models."""
    tab = P.DeviceTable(capacity, B, dev)
    st = tab.put_records(rec_to_dev(forge(mb, rows, 24 + B), dev))
    assert int(st.count_nonzero()) == 0
    return tab, {int(k): rows[i].copy() for i, k in enumerate(mb)}


def replies8(state, q, B):
    """Head-8 get replies from a state."""
    out = np.zeros((len(q), 8 + B), np.uint8)
    for p, k in enumerate(np.asarray(q, np.uint64).tolist()):
        row = state.get(k)
        if row is not None:
            out[p, 0] = 1
            out[p, 8:] = row
    return out


def check_table(tab, state, q, dev, counts):
    """The table holds exactly `state` as far as the requests q can tell, and its four counters."""
    got = tab.get(i64(q, dev)).cpu().numpy()
    assert (got == replies8(state, q, tab.rowbytes)).all()
    assert tab.counts() == tuple(counts)


def olds(rep):
    return np.ascontiguousarray(rep[:, 8:16]).view(np.uint64).ravel()


def run_update(tab, state, mb, rows, dev, stride=None, **kw):
    """One update batch on the device and on the model; status compared; returns the status."""
    rec = rec_to_dev(forge(mb, rows, stride or 24 + tab.rowbytes), dev)
    before = tab.counts()
    st = tab.update_records(rec, **kw)
    want = R.update_ref(state, mb, rows)
    assert P.last_kernel() == "k_table_locate<last>+k_table_write<8>"
    got = st.cpu().numpy()
    assert (got == want).all()
    after = tab.counts()  # nothing inserted, nothing dropped, no put probe counted, one more batch
    assert after == (before[0], before[1], before[2] + (1 if len(mb) else 0), before[3])
    return got


def run_cswap(tab, state, mb, wo, compare, desired, dev, **kw):
    """One cswap batch on the device and on the model; replies compared; returns the replies."""
    before = tab.counts()
    rep = tab.cswap(i64(mb, dev), wo, compare, desired, **kw)
    assert P.last_kernel() == "k_table_locate<first>+k_table_cswap"
    want = R.cswap_ref(state, mb, wo, compare, desired)
    got = rep.cpu().numpy()
    assert got.shape == (len(mb), 16) and (got == want).all()
    after = tab.counts()
    assert after == (before[0], before[1], before[2] + (1 if len(mb) else 0), before[3])
    return got


# =============================================================== update ===
@pytest.mark.parametrize("m", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("B", [8, 40, 64])
def test_update_half_present_half_absent(dev, B, m):
    C, n = 1 << 13, 5000
    mb, rows = distinct_mbits(n, 11), rows_for(n, B, 11)
    absent = distinct_mbits(m + 1, 12)
    for extra in (0, 8):
        tab, state = filled(dev, C, B, mb, rows)
        q = mb[:m].copy()
        q[1::2] = absent[:m][1::2]  # odd positions are not in the table
        if m == 1 and extra:
            q = absent[:1]
        new = rows_for(m, B, 13 + extra)
        st = run_update(tab, state, q, new, dev, stride=24 + B + extra)
        present = np.isin(q, mb)
        assert (st == np.where(present, 0, 3)).all() and set(state) == {int(k) for k in mb}
        check_table(tab, state, np.concatenate([mb, absent]), dev, (n, 0, 2, tab.counts()[3]))
        assert int(tab.get(i64(absent, dev)).count_nonzero()) == 0  # still not found


def test_update_moves_16_byte_pieces_when_the_put_would(dev):
    """rowbytes 48, stride 80, records + 24 16-byte aligned: k_table_write<16>; any of the three off: <8>."""
    n, m = 500, 300
    for B, S, off, tag in ((48, 80, 8, 16), (48, 80, 0, 8), (48, 72, 8, 8), (40, 80, 8, 8)):
        mb, rows = distinct_mbits(n, 21), rows_for(n, B, 21)
        tab, state = filled(dev, 1 << 13, B, mb, rows)
        q = np.concatenate([mb[:m - 50], distinct_mbits(50, 22)])[np.random.default_rng(B + S).permutation(m)]
        new = rows_for(m, B, 23)
        buf = torch.empty(m * S // 8 + 2, dtype=torch.int64, device=dev).view(torch.uint8)[off:off + m * S].view(m, S)
        buf.copy_(to_dev(forge(q, new, S), dev))
        st = tab.update_records(buf)
        assert P.last_kernel() == f"k_table_locate<last>+k_table_write<{tag}>"
        assert (st.cpu().numpy() == R.update_ref(state, q, new)).all()
        tab.put_records(buf[:1], status=False)  # and the put agrees on the rule
        assert P.last_kernel() == f"k_table_claim+k_table_write<{tag}>"
        state[int(q[0])] = new[0].copy()
        check_table(tab, state, np.concatenate([mb, q]), dev, (n + (0 if int(q[0]) in set(mb.tolist()) else 1), 0, 3,
                                                                tab.counts()[3]))


def test_update_one_mbits_many_times(dev):
    B, m = 40, 4097
    mb, rows = distinct_mbits(100, 31), rows_for(100, B, 31)
    tab, state = filled(dev, 1 << 13, B, mb, rows)
    new = rows_for(m, B, 32)
    st = run_update(tab, state, np.full(m, mb[7], np.uint64), new, dev)
    assert (st[:-1] == 1).all() and st[-1] == 0 and (state[int(mb[7])] == new[-1]).all()
    ghost = distinct_mbits(1, 33)[0]
    st = run_update(tab, state, np.full(m, ghost, np.uint64), new, dev)
    assert (st == 3).all()
    check_table(tab, state, np.concatenate([mb, [ghost]]), dev, (100, 0, 3, tab.counts()[3]))


def test_update_mark_values(dev):
    """mbits 0 (the private slot) and 1 (the mark that says slot C is taken), present and absent."""
    B = 16
    marks = np.array([0, 1], np.uint64)
    others = distinct_mbits(20, 41)
    for held in (np.concatenate([marks, others]), others, np.concatenate([marks[:1], others]),
                 np.concatenate([marks[1:], others])):
        tab, state = filled(dev, 64, B, held, rows_for(len(held), B, 42))
        q = np.array([0, 1, int(others[3]), 1, 0, 0, int(others[3]), 1], np.uint64)
        st = run_update(tab, state, q, rows_for(len(q), B, 43), dev)
        assert set(st[q == 0]) == ({1, 0} if 0 in held else {3}) and set(st[q == 1]) == ({1, 0} if 1 in held else {3})
        check_table(tab, state, np.concatenate([marks, others]), dev, (len(held), 0, 2, tab.counts()[3]))


def test_update_completely_full_table(dev):
    """Capacity 64 with 64 entries and the private slot taken: the probe of an absent mbits walks all 64
    slots, wrapping, and ends with 3; present ones are updated."""
    B, C = 24, 64
    held = np.concatenate([distinct_mbits(C, 51), [0]]).astype(np.uint64)
    tab, state = filled(dev, C, B, held, rows_for(C + 1, B, 51))
    assert tab.counts()[:2] == (C + 1, 0)
    absent = distinct_mbits(200, 52)
    q = np.concatenate([absent, held, absent[:30], held[::3]])[np.random.default_rng(5).permutation(200 + 65 + 30 + 22)]
    st = run_update(tab, state, q, rows_for(len(q), B, 53), dev)
    assert (st[np.isin(q, absent)] == 3).all() and (st[np.isin(q, held)] != 3).all()
    check_table(tab, state, np.concatenate([held, absent]), dev, (C + 1, 0, 2, tab.counts()[3]))


def test_update_second_round_of_the_grid(dev):
    """m = 2^20 + 13 over 2^19 present mbits: the lane-per-record grid tops out at 8 workgroups per CU x 256
    lanes, so lanes take a second record."""
    B, C, n, m = 8, 1 << 20, 1 << 19, (1 << 20) + 13
    mb, rows = distinct_mbits(n, 61), rows_for(n, B, 61)
    tab, state = filled(dev, C, B, mb, rows)
    rng = np.random.default_rng(62)
    pool = np.concatenate([mb, distinct_mbits(n // 8, 63)])
    q = pool[rng.integers(0, len(pool), m)]
    new = rng.integers(0, 256, (m, B), dtype=np.uint8)
    rec = rec_to_dev(forge(q, new, 24 + B), dev)
    st = tab.update_records(rec).cpu().numpy()
    want = R.update_ref(state, q, new)
    assert (st == want).all() and {0, 1, 3} == set(np.unique(st))
    check_table(tab, state, pool, dev, (n, 0, 2, tab.counts()[3]))


# ======================================================== mixed batches ===
def test_put_update_cswap_share_the_winner_words(dev):
    """Sixteen batches alternating put / update / cswap on one table, every kind touching the same mbits,
    across one clear(): a winner word left by one kind never decides a later call of another kind (the
    put's and the update's last writer and the cswap's first request of an mbits stand at unrelated positions
    of batches of different lengths, so a stale word that decided would show)."""
    B, C, wo = 24, 256, 8
    tab, model = P.DeviceTable(C, B, dev), Model(C)
    pool = np.concatenate([[0, 1], distinct_mbits(60, 71)]).astype(np.uint64)
    rng = np.random.default_rng(72)
    batches = 0
    for t in range(16):
        if t == 9:
            tab.clear()
            model, batches = Model(C), 0
        m = int(rng.integers(100, 400))
        q = pool[rng.integers(0, len(pool) if t % 3 else 40, m)]  # puts insert only part of the pool
        state = R.state_of(model)
        if t % 3 == 0:
            rows = with_word(rows_for(m, B, 73 + t), 1, UNUSED)
            st = tab.put_records(rec_to_dev(forge(q, rows, 24 + B), dev)).cpu().numpy()
            assert (st == model.put_fast(q, rows)).all()
            state = R.state_of(model)
        elif t % 3 == 1:
            rows = with_word(rows_for(m, B, 73 + t), 1, UNUSED if t % 2 else USED)
            run_update(tab, state, q, rows, dev)
        else:
            run_cswap(tab, state, q, wo, UNUSED, USED, dev)
        R.into_model(model, state)
        batches += 1
        cnt = tab.counts()
        check_table(tab, state, pool, dev, (len(state), 0, batches, cnt[3]))


# ================================================================ cswap ===
@pytest.mark.parametrize("B,wo", [(8, 0), (40, 0), (40, 16), (40, 32), (64, 56)])
def test_cswap_distinct_claims(dev, B, wo):
    n = 4097
    mb = distinct_mbits(n, 81)
    rows = with_word(rows_for(n, B, 81), wo // 8, UNUSED)
    tab, state = filled(dev, 1 << 13, B, mb, rows)
    rep = run_cswap(tab, state, mb, wo, UNUSED, USED, dev)
    assert (rep[:, 0] == 1).all() and (olds(rep) == UNUSED).all()
    want = with_word(rows, wo // 8, USED)  # every word swapped, every other byte as it was
    assert all((state[int(k)] == want[i]).all() for i, k in enumerate(mb))
    check_table(tab, state, mb, dev, (n, 0, 2, tab.counts()[3]))


def dup_batch(mb, seed):
    """mbits j requested j + 1 times for j < 65, mb[65] 4097 times; positions shuffled by a fixed seed."""
    q = np.concatenate([np.repeat(mb[:65], np.arange(1, 66)), np.full(4097, mb[65], np.uint64)])
    return q[np.random.default_rng(seed).permutation(len(q))]


def test_cswap_duplicates_first_position_wins(dev):
    B, wo, n = 40, 8, 100
    mb = distinct_mbits(n, 91)
    rows = with_word(rows_for(n, B, 91), 1, UNUSED)
    q = dup_batch(mb, 92)
    first = np.zeros(len(q), bool)
    first[np.unique(q, return_index=True)[1]] = True  # np.unique's index is the lowest position
    runs = []
    for _ in range(3):
        tab, state = filled(dev, 1 << 13, B, mb, rows)
        rep = run_cswap(tab, state, q, wo, UNUSED, USED, dev)
        assert (olds(rep)[first] == UNUSED).all() and (olds(rep)[~first] == USED).all()
        runs.append((rep, tab.get(i64(mb, dev)).cpu().numpy()))
    assert all((r[0] == runs[0][0]).all() and (r[1] == runs[0][1]).all() for r in runs)
    again = run_cswap(tab, state, q, wo, UNUSED, USED, dev)  # the same batch once more: nothing left to claim
    assert (olds(again) == USED).all()
    assert (tab.get(i64(mb, dev)).cpu().numpy() == runs[0][1]).all()
    check_table(tab, state, mb, dev, (n, 0, 3, tab.counts()[3]))


def test_cswap_words_that_do_not_match(dev):
    B, wo, n = 24, 16, 100
    mb, rows = distinct_mbits(n, 101), rows_for(n, B, 101)
    tab, state = filled(dev, 1 << 13, B, mb, rows)
    before = tab.get(i64(mb, dev)).cpu().numpy()
    q = dup_batch(mb, 102)
    rep = run_cswap(tab, state, q, wo, UNUSED, USED, dev)
    word = {int(k): int(rows[i, wo:wo + 8].copy().view(np.uint64)[0]) for i, k in enumerate(mb)}
    assert (olds(rep) == np.array([word[int(k)] for k in q], np.uint64)).all()
    assert (tab.get(i64(mb, dev)).cpu().numpy() == before).all()


def test_cswap_compare_equals_desired(dev):
    B, wo, n = 16, 8, 100
    mb = distinct_mbits(n, 111)
    rows = with_word(rows_for(n, B, 111), 1, UNUSED)
    rows[::2, 8] ^= 0xFF  # every other word is something else
    tab, state = filled(dev, 1 << 13, B, mb, rows)
    before = tab.get(i64(mb, dev)).cpu().numpy()
    rep = run_cswap(tab, state, dup_batch(mb, 112), wo, UNUSED, UNUSED, dev)
    assert (rep[:, 0] == 1).all()
    assert (tab.get(i64(mb, dev)).cpu().numpy() == before).all()


@pytest.mark.parametrize("compare,desired", [(-1, -2), (1 << 63, 5), (5, (1 << 64) - 1), (-(1 << 63), -1)])
def test_cswap_top_bit_operands(dev, compare, desired):
    B, wo, n = 16, 0, 100
    mb = distinct_mbits(n, 121)
    rows = with_word(rows_for(n, B, 121), 0, compare)
    tab, state = filled(dev, 1 << 13, B, mb, rows)
    q = dup_batch(mb, 122)
    rep = run_cswap(tab, state, q, wo, compare, desired, dev)
    assert set(olds(rep).tolist()) == {compare & M64, desired & M64}
    assert all(int(state[int(k)][:8].view(np.uint64)[0]) == desired & M64 for k in np.unique(q))
    check_table(tab, state, mb, dev, (n, 0, 2, tab.counts()[3]))


def test_cswap_absent_mbits(dev):
    B, wo, n = 24, 8, 100
    mb = distinct_mbits(n, 131)
    tab, state = filled(dev, 1 << 13, B, mb, with_word(rows_for(n, B, 131), 1, UNUSED))
    absent = distinct_mbits(70, 132)
    q = np.concatenate([dup_batch(mb, 133)[:900], np.repeat(absent, 3)])[np.random.default_rng(134).permutation(1110)]
    rep = run_cswap(tab, state, q, wo, UNUSED, USED, dev)
    assert int(rep[np.isin(q, absent)].sum()) == 0  # {0, 0}
    check_table(tab, state, np.concatenate([mb, absent]), dev, (n, 0, 2, tab.counts()[3]))
    # a completely full table: the probes of absent mbits wrap and end
    C = 64
    held = np.concatenate([distinct_mbits(C, 135), [0]]).astype(np.uint64)
    tab, state = filled(dev, C, B, held, with_word(rows_for(C + 1, B, 135), 1, UNUSED))
    q = np.concatenate([absent, held, held, absent])[np.random.default_rng(136).permutation(2 * (70 + 65))]
    rep = run_cswap(tab, state, q, wo, UNUSED, USED, dev)
    assert int(rep[np.isin(q, absent)].sum()) == 0 and (rep[np.isin(q, held), 0] == 1).all()
    check_table(tab, state, np.concatenate([held, absent]), dev, (C + 1, 0, 2, tab.counts()[3]))


def test_cswap_mark_values(dev):
    B, wo = 16, 8
    marks = np.array([0, 1], np.uint64)
    others = distinct_mbits(20, 141)
    for held in (np.concatenate([marks, others]), others, np.concatenate([marks[:1], others]),
                 np.concatenate([marks[1:], others])):
        tab, state = filled(dev, 64, B, held, with_word(rows_for(len(held), B, 142), 1, UNUSED))
        q = np.array([0, 1, int(others[3]), 1, 0, 0, int(others[3]), 1], np.uint64)
        rep = run_cswap(tab, state, q, wo, UNUSED, USED, dev)
        assert rep[:, 0].tolist() == [int(k in held) for k in q]
        check_table(tab, state, np.concatenate([marks, others]), dev, (len(held), 0, 2, tab.counts()[3]))


def test_cswap_reads_get_records_in_place(dev):
    """bucket_records' get records (stride 32 for 8-byte keys, the mbits at +16); the table is keyed by the
    digests the records carry."""
    n, W, B = 1000, 3, 16
    keys = np.random.default_rng(151).integers(0, 256, (n, 8), dtype=np.uint8)
    keys[n // 2:] = keys[:n // 2]  # every key twice
    rec, offs = P.bucket_records(to_dev(keys, dev), W, msg_type=0, src_rank=1)
    assert rec.shape[1] == 32
    mb = P.record_fields(rec, 8)[4].cpu().numpy().view(np.uint64)
    held = np.ascontiguousarray(np.unique(mb)[::2])
    tab, state = filled(dev, 1 << 13, B, held, with_word(rows_for(len(held), B, 152), 0, UNUSED))
    rep = tab.cswap(rec, 0, UNUSED, USED).cpu().numpy()
    assert (rep == R.cswap_ref(state, mb, 0, UNUSED, USED)).all()
    assert (rep[:, 0] == np.isin(mb, held)).all() and int((olds(rep) == UNUSED).sum()) == len(held)
    check_table(tab, state, np.unique(mb), dev, (len(held), 0, 2, tab.counts()[3]))


@pytest.mark.parametrize("stride,off", [(16, 0), (16, 8), (24, 0), (32, 0), (32, 8), (48, 16)])
def test_cswap_reply_forms(dev, stride, off):
    """One 16-byte store (address and stride multiples of 16) or two 8-byte ones; every reply sits between
    guard bytes and the bytes of the stride beyond 16 keep theirs."""
    B, wo, n, m = 16, 8, 100, 777
    mb = distinct_mbits(n, 161)
    tab, state = filled(dev, 1 << 13, B, mb, with_word(rows_for(n, B, 161), 1, UNUSED))
    q = np.concatenate([mb, distinct_mbits(30, 162)])[np.random.default_rng(163).integers(0, n + 30, m)]
    buf = torch.full((m * stride + 64,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    out = buf[16 + off:16 + off + m * stride].view(m, stride)[:, :16]
    got = tab.cswap(i64(q, dev), wo, UNUSED, USED, out=out)
    assert got.data_ptr() == out.data_ptr()
    d = buf.cpu().numpy()
    body = d[16 + off:16 + off + m * stride].reshape(m, stride)
    assert (body[:, :16] == R.cswap_ref(state, q, wo, UNUSED, USED)).all()
    assert (body[:, 16:] == 0xA5).all() and (d[:16 + off] == 0xA5).all() and (d[16 + off + m * stride:] == 0xA5).all()


def test_cswap_workspace_of_exactly_the_queried_size(dev):
    """The workspace is written before it is read: zeros, ones and another call's leftovers give one result."""
    B, wo, n = 16, 8, 100
    mb = distinct_mbits(n, 171)
    rows = with_word(rows_for(n, B, 171), 1, UNUSED)
    q = np.concatenate([dup_batch(mb, 172), distinct_mbits(50, 173)])
    need = P.lib().pdht_table_cswap_workspace_bytes(len(q))
    assert need == 4 * len(q)
    ws = torch.empty(need // 4, dtype=torch.int32, device=dev).view(torch.uint8)
    res = []
    for fill in (0x00, 0xFF, None):
        if fill is not None:
            ws.fill_(fill)
        tab, state = filled(dev, 1 << 13, B, mb, rows)
        rep = run_cswap(tab, state, q, wo, UNUSED, USED, dev, workspace=ws)
        res.append((rep, tab.get(i64(mb, dev)).cpu().numpy()))
    assert all((r[0] == res[0][0]).all() and (r[1] == res[0][1]).all() for r in res)
    with pytest.raises(ValueError):
        tab.cswap(i64(q, dev), wo, UNUSED, USED, workspace=ws[:-4])


def test_cswap_hot_key_second_round_of_the_grid(dev):
    B, C, n, m = 8, 1 << 14, 5000, (1 << 20) + 13
    mb = distinct_mbits(n, 181)
    tab, state = filled(dev, C, B, mb, with_word(rows_for(n, B, 181), 0, UNUSED))
    rng = np.random.default_rng(182)
    q = np.concatenate([mb, distinct_mbits(500, 183)])[rng.integers(0, n + 500, m)]
    q[rng.random(m) < 0.9] = mb[17]
    rep = run_cswap(tab, state, q, 0, UNUSED, USED, dev)
    hot = np.flatnonzero(q == mb[17])
    assert olds(rep)[hot[0]] == UNUSED and (olds(rep)[hot[1:]] == USED).all()
    check_table(tab, state, np.unique(q), dev, (n, 0, 2, tab.counts()[3]))


def test_cswap_and_update_on_a_side_stream(dev):
    B, wo, n = 24, 8, 2000
    mb = distinct_mbits(n, 191)
    tab, state = filled(dev, 1 << 13, B, mb, with_word(rows_for(n, B, 191), 1, UNUSED))
    q = np.concatenate([mb, mb[::2], distinct_mbits(100, 192)])[np.random.default_rng(193).permutation(n + n // 2 + 100)]
    new = with_word(rows_for(len(q), B, 194), 1, UNUSED)
    qd, rec = i64(q, dev), rec_to_dev(forge(q, new, 24 + B), dev)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    rep1 = tab.cswap(qd, wo, UNUSED, USED, stream=s)
    st = tab.update_records(rec, stream=s)
    rep2 = tab.cswap(qd, wo, UNUSED, USED, stream=s)
    s.synchronize()
    assert (rep1.cpu().numpy() == R.cswap_ref(state, q, wo, UNUSED, USED)).all()
    assert (st.cpu().numpy() == R.update_ref(state, q, new)).all()
    assert (rep2.cpu().numpy() == R.cswap_ref(state, q, wo, UNUSED, USED)).all()
    check_table(tab, state, q, dev, (n, 0, 4, tab.counts()[3]))


def test_put_cswap_update_get_in_one_graph(dev):
    """put -> cswap -> update -> get captured as one linear chain and replayed twice.  The claimed entries
    were put before the capture; the graph's put brings other mbits, its update rewrites claimed rows with
    the flag set.  The batch number is read on the device, so each replay is a new batch: the first replay's
    claims see UNUSED once per mbits, the second replay's claims all see USED."""
    B, wo, C, n = 24, 8, 1 << 13, 500
    mb, extra, ghost = distinct_mbits(n, 201), distinct_mbits(300, 202), distinct_mbits(40, 203)
    tab, state = filled(dev, C, B, mb, with_word(rows_for(n, B, 201), 1, UNUSED))
    rng = np.random.default_rng(204)
    put_mb = extra[rng.integers(0, 300, 700)]
    put_rows = with_word(rows_for(700, B, 205), 1, UNUSED)
    claim = np.concatenate([mb, mb[:200], ghost])[rng.permutation(n + 240)]
    upd_mb = np.concatenate([mb[:300], mb[:50], ghost[:10]])[rng.permutation(360)]
    upd_rows = with_word(rows_for(360, B, 206), 1, USED)
    ask = np.concatenate([mb, extra, ghost])
    put_rec, upd_rec = rec_to_dev(forge(put_mb, put_rows, 24 + B), dev), rec_to_dev(forge(upd_mb, upd_rows, 24 + B), dev)
    claim_d, ask_d = i64(claim, dev), i64(ask, dev)
    ws = [torch.empty(4 * k, dtype=torch.uint8, device=dev) for k in (700, len(claim), 360)]
    st_put = torch.empty(700, dtype=torch.uint8, device=dev)
    st_upd = torch.empty(360, dtype=torch.uint8, device=dev)
    rep = torch.empty((len(claim), 16), dtype=torch.uint8, device=dev)
    got = torch.empty((len(ask), 8 + B), dtype=torch.uint8, device=dev)

    def chain():
        tab.put_records(put_rec, status=st_put, workspace=ws[0])
        tab.cswap(claim_d, wo, UNUSED, USED, out=rep, workspace=ws[1])
        tab.update_records(upd_rec, status=st_upd, workspace=ws[2])
        tab.get(ask_d, out=got)

    scratch = P.DeviceTable(C, B, dev)  # warm-up outside capture, on a table of its own
    real, tab.storage = tab.storage, scratch.storage
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    tab.storage = real
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    model = Model(C)
    for replay in range(2):
        for t in (st_put, st_upd, rep, got):
            t.fill_(0xEE)
        g.replay()
        torch.cuda.synchronize()
        R.into_model(model, state)
        want_put = model.put_fast(put_mb, put_rows)
        state = R.state_of(model)
        want_rep = R.cswap_ref(state, claim, wo, UNUSED, USED)
        want_upd = R.update_ref(state, upd_mb, upd_rows)
        assert (st_put.cpu().numpy() == want_put).all()
        r = rep.cpu().numpy()
        assert (r == want_rep).all()
        seen = olds(r)[np.isin(claim, mb)]
        assert (seen == USED).all() if replay else int((seen == UNUSED).sum()) == n
        assert (st_upd.cpu().numpy() == want_upd).all()
        assert (got.cpu().numpy() == replies8(state, ask, B)).all()
        assert tab.counts()[:3] == (n + len(np.unique(put_mb)), 0, 1 + 3 * (replay + 1))
