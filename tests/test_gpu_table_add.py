"""GPU checks of the table's insert-if-absent (include/pdht_hip_table_add.h): after every call the status,
the replies, a get of every mbits (plus absent ones), the exported entries and the four counters are
compared byte for byte against the sequential model of tests/table_add_ref.py, which applies one record
after the other and knows nothing of "first", "creator", winner words, waves or atomics.  Tables have 64
to 4096 slots except where a batch has to outgrow the grid."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

import table_add_ref as A  # noqa: E402
import table_rmw_ref as R  # noqa: E402
import table_acc_ref as ACC  # noqa: E402
from test_gpu_table import distinct_mbits, forge, rows_for, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------- helpers ---
def i64(mb, dev):
    return to_dev(np.asarray(mb, np.uint64).view(np.int64), dev)


def rec_at(rec, dev, off=0):
    """The records on the device at a 16-byte aligned address + off (off a multiple of 8): records + 24 is a
    multiple of 16 exactly when off % 16 == 8."""
    m, S = rec.shape
    buf = torch.empty(m * S // 8 + 8, dtype=torch.int64, device=dev).view(torch.uint8)
    assert buf.data_ptr() % 16 == 0 and off % 8 == 0
    out = buf[off:off + m * S].view(m, S)
    out.copy_(to_dev(rec, dev))
    return out


def write_tag(B, stride, off):
    return 16 if B % 16 == 0 and stride % 16 == 0 and (off + 24) % 16 == 0 else 8


def replies8(state, q, B):
    out = np.zeros((len(q), 8 + B), np.uint8)
    for p, k in enumerate(np.asarray(q, np.uint64).tolist()):
        row = state.get(k)
        if row is not None:
            out[p, 0] = 1
            out[p, 8:] = row
    return out


def check_table(tab, state, q, dev):
    """The table holds exactly `state`: a get of the requests q, and the exported entries."""
    got = tab.get(i64(q, dev)).cpu().numpy()
    assert (got == replies8(state, q, tab.rowbytes)).all()
    mbits, rows, _ = tab.entries()
    mbits, rows = mbits.cpu().numpy().view(np.uint64).tolist(), rows.cpu().numpy()
    assert sorted(mbits) == sorted(state)
    for k, r in zip(mbits, rows):
        assert (r == state[k]).all()


ABSENT = distinct_mbits(7, 999)  # mbits no test stores


def run_add(tab, state, mb, rows, dev, stride=None, off=0, replies=True, overflow=False, **kw):
    """One add batch on the device and on the model: last_kernel, status, replies, the table (get and export)
    and the counters compared.  overflow: the batch may drop; the set of dropped mbits is then read from the
    device's status (which new mbits lose is the schedule's choice) and the model checks the drop rules.
    Returns (status, replies) as numpy arrays."""
    B = tab.rowbytes
    stride = stride or 24 + B
    mb = np.ascontiguousarray(mb, np.uint64)
    rec = rec_at(forge(mb, rows, stride), dev, off)
    before, had = tab.counts(), set(state)
    out = tab.add_records(rec, replies=replies, **kw)
    st, rep = out if replies else (out, None)
    name = f"k_table_add_claim+k_table_add_write<{write_tag(B, stride, off)}>"
    if replies:
        name += f"+k_table_add_reply<{16 if (B // 8 + 1) % 2 == 0 else 8}>"  # fresh replies: aligned, dense
    assert P.last_kernel() == name
    got = st.cpu().numpy()
    lost = set(mb[got == 2].tolist())
    assert overflow or not lost
    assert not (lost & set(mb[got != 2].tolist()))  # all records of one mbits share one fate
    want, want_rep = A.add_ref(state, mb, rows, capacity=tab.capacity, dropped=lost)
    assert (got == want).all()
    if replies:
        rep = rep.cpu().numpy()
        assert (rep == want_rep).all()
        assert (rep == tab.get(rec, head=8).cpu().numpy()).all()  # a get after the call, records read in place
    check_table(tab, state, np.concatenate([np.unique(mb), ABSENT]), dev)
    after = tab.counts()
    assert after[:3] == (before[0] + len(set(state) - had), before[1] + int((got == 2).sum()), before[2] + 1)
    assert after[3] - before[3] >= len(mb) and after[0] == len(state)
    return got, rep


def filled(dev, capacity, B, mb, rows):
    """A table that holds rows[i] under mb[i] (distinct) after one add, and its state for the model."""
    tab, state = P.DeviceTable(capacity, B, dev), {}
    st, _ = run_add(tab, state, mb, rows, dev)
    assert (st == 0).all()
    return tab, state


def differing_rows(mb, B):
    """Rows in which any two records of one mbits (up to 256 of them; beyond, any record and the first) differ
    in every byte."""
    mb = np.asarray(mb, np.uint64)
    nth = np.zeros(len(mb), np.int64)
    seen = {}
    for p, k in enumerate(mb.tolist()):
        nth[p] = seen.get(k, 0)
        seen[k] = nth[p] + 1
    v = np.where(nth == 0, 0, 1 + (nth - 1) % 255)
    return ((v[:, None] + 31 * np.arange(B)[None, :]) & 0xFF).astype(np.uint8)


# ============================================================== sizes ===
@pytest.mark.parametrize("m", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("B", [16, 40])
def test_half_present(dev, B, m):
    """Distinct mbits, every other one present: 4 and an untouched row for those, 0 and the record's row for
    the rest; then the same batch again finds everything present."""
    mb = distinct_mbits(m, 3100 + m)
    tab, state = filled(dev, 8192, B, mb[::2], rows_for(len(mb[::2]), B, 3100))
    rows = rows_for(m, B, 3101)
    st, _ = run_add(tab, state, mb, rows, dev)
    assert (st == np.where(np.arange(m) % 2 == 0, 4, 0)).all()
    st, _ = run_add(tab, state, mb, rows_for(m, B, 3102), dev)
    assert (st == 4).all()


# ========================================================== duplicates ===
def test_duplicates_first_position_wins_on_every_run(dev):
    """c records per mbits for every c in 1 .. 65, a new and a present mbits with 4097 each, shuffled; every
    second mbits present.  Rows of one mbits differ in every byte, so any row but the lowest position's shows.
    Three runs on fresh tables give identical bytes."""
    B = 24
    keys = distinct_mbits(67, 3200)
    mb = np.concatenate([np.repeat(keys[:65], np.arange(1, 66)), np.full(4097, keys[65]), np.full(4097, keys[66])])
    mb = mb[np.random.default_rng(3201).permutation(len(mb))]
    rows = differing_rows(mb, B)
    first = {}
    for p, k in enumerate(mb.tolist()):
        first.setdefault(k, p)
    runs = []
    for _ in range(3):
        tab, state = filled(dev, 256, B, keys[::2], rows_for(34, B, 3202))
        before = {k: v.copy() for k, v in state.items()}
        st, rep = run_add(tab, state, mb, rows, dev)
        for k in keys.tolist():
            if k in before:
                assert (state[k] == before[k]).all() and (st[mb == k] == 4).all()
            else:
                assert (state[k] == rows[first[k]]).all() and st[first[k]] == 0 and (st[mb == k] == 0).sum() == 1
        runs.append((st, rep, tab.get(i64(keys, dev)).cpu().numpy()))
    for r in runs[1:]:
        assert all((a == b).all() for a, b in zip(r, runs[0]))


def test_mbits_zero_and_one(dev):
    """mbits 0 lives in its private slot and mbits 1 is its tag there: both are ordinary keys."""
    B = 16
    tab, state = P.DeviceTable(64, B, dev), {}
    mb = np.array([1, 0, 0, 1, 5, 0, 1] * 20, np.uint64)
    st, rep = run_add(tab, state, mb, differing_rows(mb, B), dev)
    assert st[:5].tolist() == [0, 0, 4, 4, 0] and (st[5:] == 4).all()
    assert (rep[2, 8:] == differing_rows(mb, B)[1]).all()
    st, _ = run_add(tab, state, mb[::-1].copy(), rows_for(len(mb), B, 3300), dev)
    assert (st == 4).all() and tab.counts()[0] == 3


def test_one_mbits_4097_times_into_an_empty_table(dev):
    B = 40
    tab, state = P.DeviceTable(64, B, dev), {}
    mb = np.full(4097, distinct_mbits(1, 3400)[0])
    rows = differing_rows(mb, B)
    st, rep = run_add(tab, state, mb, rows, dev)
    assert st[0] == 0 and (st[1:] == 4).all() and (rep[:, 8:] == rows[0]).all() and tab.counts()[0] == 1


# ============================================================ overflow ===
def test_a_64_slot_table_filled_overfilled_and_added_to_again(dev):
    B, C = 16, 64
    tab, state = P.DeviceTable(C, B, dev), {}
    a = distinct_mbits(C, 3500)
    st, _ = run_add(tab, state, a, rows_for(C, B, 3500), dev)  # filled exactly: every probe ends
    assert (st == 0).all() and tab.counts()[:2] == (C, 0)
    b = np.concatenate([distinct_mbits(30, 3501), np.array([1, 0], np.uint64)])
    mb = np.concatenate([a, np.repeat(b, 5), a[::-1]])
    mb = mb[np.random.default_rng(3502).permutation(len(mb))]
    st, rep = run_add(tab, state, mb, rows_for(len(mb), B, 3503), dev, overflow=True)
    present = np.isin(mb, a)
    assert (st[present] == 4).all()  # present ones still answer 4
    zero = mb == 0
    assert sorted(st[zero].tolist()) == [0, 4, 4, 4, 4]  # mbits 0 never competes for a slot
    assert (st[~present & ~zero] == 2).all() and (rep[st == 2] == 0).all()  # mbits 1 included
    assert tab.counts()[:2] == (C + 1, 31 * 5)
    st, _ = run_add(tab, state, mb, rows_for(len(mb), B, 3504), dev, overflow=True)  # and again: the same fates
    assert (st[present | zero] == 4).all() and (st[~present & ~zero] == 2).all()


def test_overflow_part_way(dev):
    """40 of 64 slots taken, 100 new mbits of 10 records each: 24 get in, whichever; the model checks that the
    dropped are new, whole and exactly as many as have to go.  The second round meets the same winners."""
    B, C = 24, 64
    old, new = distinct_mbits(40, 3600), distinct_mbits(100, 3601)
    tab, state = filled(dev, C, B, old, rows_for(40, B, 3600))
    mb = np.repeat(np.concatenate([old, new]), 10)
    mb = mb[np.random.default_rng(3602).permutation(len(mb))]
    st1, _ = run_add(tab, state, mb, differing_rows(mb, B), dev, overflow=True)
    assert len(state) == C and (st1 == 2).sum() == 76 * 10 and (st1 == 0).sum() == 24
    st2, _ = run_add(tab, state, mb, rows_for(len(mb), B, 3603), dev, overflow=True)
    assert ((st2 == 2) == (st1 == 2)).all() and (st2[st1 != 2] == 4).all()


# ===================================================== rows and pieces ===
@pytest.mark.parametrize("pieces", [1, 2, 5, 63, 64, 65, 129])
@pytest.mark.parametrize("P_", [16, 8])
def test_rows_of_many_pieces(dev, pieces, P_):
    """Rows of 1 .. 129 pieces of both widths: lane groups of 1 .. 64 lanes, and rows that a wave sweeps.  The
    16-byte form needs records + 24, the stride and the row to be multiples of 16; the 8-byte form gets an odd
    row (in 8s) or, where the row would allow 16, an address that does not."""
    B = pieces * P_
    off = 8 if P_ == 16 or B % 16 else 0
    stride = 24 + B + (8 if (24 + B) % 16 and P_ == 16 else 0)
    assert write_tag(B, stride, off) == P_
    keys = distinct_mbits(40, 3700 + pieces)
    tab, state = filled(dev, 64, B, keys[:20], rows_for(20, B, 3700))
    mb = keys[np.random.default_rng(3701).integers(0, 40, 150)]
    run_add(tab, state, mb, differing_rows(mb, B), dev, stride=stride, off=off)


@pytest.mark.parametrize("B,stride,off,tag", [(16, 40, 8, 8), (16, 48, 8, 16), (16, 48, 0, 8), (16, 48, 16, 8),
                                              (24, 48, 8, 8), (32, 64, 24, 16), (32, 72, 8, 8), (8, 32, 8, 8)])
def test_addresses_and_strides_select_the_piece(dev, B, stride, off, tag):
    assert write_tag(B, stride, off) == tag
    keys = distinct_mbits(50, 3800)
    tab, state = filled(dev, 64, B, keys[:25], rows_for(25, B, 3800))
    mb = keys[np.random.default_rng(3801).integers(0, 50, 333)]
    run_add(tab, state, mb, differing_rows(mb, B), dev, stride=stride, off=off)  # (it compares last_kernel)


# ===================================================== status, replies ===
def test_without_status_and_without_replies(dev):
    B = 16
    keys = distinct_mbits(30, 3900)
    mb = keys[np.random.default_rng(3901).integers(0, 30, 200)]
    rows = differing_rows(mb, B)
    want_state = {}
    want, want_rep = A.add_ref(want_state, mb, rows, capacity=64)
    for status in (None, False):
        for replies in (None, False, True):
            tab = P.DeviceTable(64, B, dev)
            out = tab.add_records(rec_at(forge(mb, rows, 40), dev), status=status, replies=replies)
            if replies:
                assert out[0] is None and (out[1].cpu().numpy() == want_rep).all()
                assert tuple(out[1].shape) == (200, 8 + B) and out[1].dtype == torch.uint8
            else:
                assert out is None
            check_table(tab, want_state, keys, dev)
    tab = P.DeviceTable(64, B, dev)
    mine = torch.full((200,), 0xEE, dtype=torch.uint8, device=dev)
    assert tab.add_records(rec_at(forge(mb, rows, 40), dev), status=mine).data_ptr() == mine.data_ptr()
    assert (mine.cpu().numpy() == want).all()
    empty = tab.add_records(torch.empty((0, 40), dtype=torch.uint8, device=dev), replies=True)
    assert empty[0].numel() == 0 and tuple(empty[1].shape) == (0, 8 + B) and tab.counts()[2] == 1


@pytest.mark.parametrize("B,pad,off,tag", [(16, 0, 0, 8), (16, 8, 0, 8), (24, 0, 0, 16), (24, 16, 16, 16), (24, 8, 0, 8),
                                           (24, 0, 8, 8), (8, 0, 0, 16), (8, 8, 8, 8), (40, 24, 0, 8), (1032, 0, 0, 16)])
def test_replies_between_guard_bytes(dev, B, pad, off, tag):
    """Replies into a caller's buffer at strides of 8 + rowbytes and more: the reply bytes are the model's, every
    byte of the pad, before the first and behind the last reply keeps its pattern.  16-byte pieces when address,
    stride and 8 + rowbytes allow."""
    keys = distinct_mbits(12, 4000)
    tab, state = filled(dev, 64, B, keys[:6], rows_for(6, B, 4000))
    m = 131
    mb = keys[np.random.default_rng(4001).integers(0, 12, m)]
    rows = differing_rows(mb, B)
    S = 8 + B + pad
    buf = torch.full((m * (S + 8) + 64,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[16 + off:16 + off + m * S].view(m, S)[:, :8 + B]
    st, rep = tab.add_records(rec_at(forge(mb, rows, 24 + B), dev), replies=view)
    assert rep.data_ptr() == view.data_ptr()
    assert P.last_kernel() == f"k_table_add_claim+k_table_add_write<8>+k_table_add_reply<{tag}>"
    want, want_rep = A.add_ref(state, mb, rows, capacity=64)
    d = buf.cpu().numpy()
    body = d[16 + off:16 + off + m * S].reshape(m, S)
    assert (st.cpu().numpy() == want).all() and (body[:, :8 + B] == want_rep).all()
    assert (body[:, 8 + B:] == 0xA5).all() and (d[:16 + off] == 0xA5).all() and (d[16 + off + m * S:] == 0xA5).all()
    for bad in (buf[4:4 + m * S].view(m, S)[:, :8 + B], buf[:m * (S + 4)].view(m, S + 4)[:, :8 + B],
                buf[:m * S].view(m, S)[:, :B], buf[:(m - 1) * S].view(m - 1, S)[:, :8 + B]):
        with pytest.raises(ValueError):
            tab.add_records(rec_at(forge(mb, rows, 24 + B), dev), replies=bad)


@pytest.mark.parametrize("fill", [0x00, 0xFF, "noise"])
def test_a_workspace_of_exactly_the_queried_size(dev, fill):
    """Whatever the workspace held: its contents on entry do not matter.  One byte less is refused."""
    B, m = 16, 4097
    keys = distinct_mbits(500, 4100)
    tab, state = filled(dev, 1024, B, keys[:250], rows_for(250, B, 4100))
    mb = keys[np.random.default_rng(4101).integers(0, 500, m)]
    need = P.table_add_workspace_bytes(m)
    assert need == 4 * m + 4100
    if fill == "noise":
        ws = to_dev(np.random.default_rng(4102).integers(0, 256, need, dtype=np.uint8), dev)
    else:
        ws = torch.full((need,), fill, dtype=torch.uint8, device=dev)
    run_add(tab, state, mb, differing_rows(mb, B), dev, workspace=ws)
    with pytest.raises(ValueError):
        tab.add_records(rec_at(forge(mb, rows_for(m, B, 1), 40), dev), workspace=ws[:-1])


# ========================================================= big batches ===
def test_second_round_of_the_grid_with_a_hot_mbits(dev):
    """2^20 + 13 records, 90 % of them on one mbits: past the reach of one round of k_table_add_claim's grid
    (8 workgroups of 256 lanes per CU), the last wave partly past the end, and most waves of it post the hot
    slot's first position once between them."""
    B, m = 8, (1 << 20) + 13
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert m > cus * 8 * 256 and m % 64
    keys = distinct_mbits(3000, 4200)
    tab, state = filled(dev, 4096, B, keys[:1500], rows_for(1500, B, 4200))
    rng = np.random.default_rng(4201)
    mb = keys[rng.integers(0, 3000, m)]
    mb[rng.random(m) < 0.9] = keys[2999]  # a new one
    mb[:5000] = keys[rng.integers(0, 2999, 5000)]  # whose first record comes late
    rows = rows_for(m, B, 4202)
    st, rep = run_add(tab, state, mb, rows, dev)
    f = int(np.flatnonzero(mb == keys[2999])[0])
    assert f >= 5000 and st[f] == 0 and (state[int(keys[2999])] == rows[f]).all()


# ========================================================= repeat calls ===
def test_sixteen_batches_of_every_kind_across_a_clear(dev):
    """add / put / update / cswap / acc in turn on one table over one pool of mbits, a clear in the middle:
    winner words and batch numbers of earlier calls of any kind decide nothing later."""
    B, C = 24, 256
    pool = np.concatenate([np.zeros(1, np.uint64), distinct_mbits(130, 4300)])
    rng = np.random.default_rng(4301)
    tab, state, batches = P.DeviceTable(C, B, dev), {}, 0
    for t, what in enumerate(["add", "put", "update", "cswap", "acc", "add", "put", "add", "clear",
                              "add", "update", "add", "acc", "cswap", "add", "put", "add"]):
        m = int(rng.integers(100, 600))
        mb = pool[rng.integers(0, 60 + 4 * t, m)]
        rows = rows_for(m, B, 4310 + t)
        rec = rec_at(forge(mb, rows, 24 + B), dev)
        if what == "clear":
            tab.clear()
            state, batches = {}, 0
            continue
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
            assert (tab.update_records(rec).cpu().numpy() == R.update_ref(state, mb, rows)).all()
        elif what == "cswap":
            held = [k for k in mb.tolist() if k in state]
            word = int(state[held[0]][8:16].view(np.uint64)[0])  # what one of the entries holds: it swaps
            got = tab.cswap(rec, 8, word, 77).cpu().numpy()
            assert (got == R.cswap_ref(state, mb, 8, word, 77)).all()
        else:
            st = tab.acc_records(rec, torch.int64, 16, insert=True).cpu().numpy()
            assert (st == ACC.acc_ref(state, mb, rows, np.int64, 16, 1, True, capacity=C)[0]).all()
        batches += 1
        assert tab.counts()[:3] == (len(state), 0, batches)
        check_table(tab, state, pool, dev)


def test_add_on_a_side_stream(dev):
    B, m = 16, 700
    keys = distinct_mbits(80, 4400)
    tab, state = filled(dev, 256, B, keys[:40], rows_for(40, B, 4400))
    mb = keys[np.random.default_rng(4401).integers(0, 80, m)]
    rows = differing_rows(mb, B)
    rec = rec_at(forge(mb, rows, 40), dev)
    ws = torch.empty(P.table_add_workspace_bytes(m), dtype=torch.uint8, device=dev)
    st = torch.full((m,), 0xEE, dtype=torch.uint8, device=dev)
    rep = torch.full((m, 8 + B), 0xEE, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    tab.add_records(rec, status=st, replies=rep, workspace=ws, stream=s)
    s.synchronize()
    want, want_rep = A.add_ref(state, mb, rows, capacity=256)
    assert (st.cpu().numpy() == want).all() and (rep.cpu().numpy() == want_rep).all()
    check_table(tab, state, keys, dev)


def test_add_get_put_add_in_a_graph(dev):
    """One captured graph of add(a) -> get -> put(b) -> add(c), replayed twice: every replay starts from the
    table the one before left, and the model is stepped along with it."""
    B, m = 40, 900
    keys = distinct_mbits(400, 4500)
    rng = np.random.default_rng(4501)
    batch = {x: keys[rng.integers(lo, hi, m)] for x, (lo, hi) in dict(a=(0, 250), b=(100, 300), c=(150, 400)).items()}
    rows = {x: rows_for(m, B, 4502 + i) for i, x in enumerate("abc")}
    rec = {x: rec_at(forge(batch[x], rows[x], 24 + B), dev) for x in "abc"}
    q = i64(keys, dev)
    tab, state = P.DeviceTable(1024, B, dev), {}
    ws = torch.empty(P.table_add_workspace_bytes(m), dtype=torch.uint8, device=dev)
    st = {x: torch.empty(m, dtype=torch.uint8, device=dev) for x in "abc"}
    rep = {x: torch.empty((m, 8 + B), dtype=torch.uint8, device=dev) for x in "ac"}
    out = torch.empty((400, 8 + B), dtype=torch.uint8, device=dev)

    def step():
        tab.add_records(rec["a"], status=st["a"], replies=rep["a"], workspace=ws)
        tab.get(q, out=out)
        tab.put_records(rec["b"], status=st["b"], workspace=ws[:4 * m])
        tab.add_records(rec["c"], status=st["c"], replies=rep["c"], workspace=ws)

    def model_step():
        want = {"a": A.add_ref(state, batch["a"], rows["a"], capacity=1024)}
        want["get"] = replies8(state, keys, B)
        for p, k in enumerate(batch["b"].tolist()):
            state[k] = rows["b"][p].copy()
        want["c"] = A.add_ref(state, batch["c"], rows["c"], capacity=1024)
        return want

    def compare(want):
        for x in "ac":
            assert (st[x].cpu().numpy() == want[x][0]).all() and (rep[x].cpu().numpy() == want[x][1]).all()
        assert (out.cpu().numpy() == want["get"]).all()
        check_table(tab, state, keys, dev)

    step()  # eager
    compare(model_step())
    base = tab.counts()
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    assert tab.counts() == base  # capture runs nothing
    for k in (1, 2):
        for t in list(st.values()) + list(rep.values()) + [out]:
            t.fill_(9)
        g.replay()
        torch.cuda.synchronize(dev)
        compare(model_step())
        assert tab.counts()[:3] == (len(state), 0, base[2] + 3 * k)
