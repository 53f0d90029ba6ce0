"""GPU checks of the table export and of rehash (include/pdht_hip_table_iter.h): every output byte-exact
against the numpy model of tests/table_iter_ref.py, which reads a copy of the table's storage by the
documented layout, and every output buffer between guard bytes (0xA5) that must survive.  T = 1024 is the
export's tile (kExportTile, pdht_amd/csrc/table_iter.h): tiles are counted from first_slot."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

import table_iter_ref as IR  # noqa: E402
import table_ref as R  # noqa: E402
from test_gpu_table import distinct_mbits, forge, rec_to_dev, rows_for, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

T = IR.TILE
CHAIN = "k_table_export_count+k_table_export_scan"
GUARD = 0xA5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def tag_for(piece):
    return f"{CHAIN}<0>" if piece is None else f"{CHAIN}+k_table_export_write<{piece}>"


def forged_table(dev, C, B, live, seed=0):
    """A DeviceTable whose storage is forge_storage's image, and the image."""
    img = IR.forge_storage(C, B, live, seed)
    tab = P.DeviceTable(C, B, dev)
    assert tab.nbytes == img.size
    tab.storage.copy_(to_dev(img, dev))
    return tab, img


def image(tab):
    return tab.storage.cpu().numpy().copy()


def guarded(dev, nbytes, front):
    """A uint8 view of `nbytes` bytes, `front` bytes into a buffer of guard bytes (16-byte aligned base)."""
    buf = torch.full((front + nbytes + 64,), GUARD, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[front:front + nbytes]


def check_export(tab, img, dev, first=0, nslots=None, max_entries=None, form="dense", rows_front=None,
                 row_pad=0, piece="auto", with_rows=True, with_slots=True, workspace=None, stream=None):
    """One export between guard bytes against the model.  form "dense": three arrays (rows at `rows_front`
    bytes into their buffer, default one row stride, with `row_pad` bytes between rows); "record": one record
    buffer of stride 24 + B + row_pad.  Returns (mbits, rows, slots, count2) as the model gave them."""
    C, B = tab.capacity, tab.rowbytes
    n = C + 1 - first if nslots is None else nslots
    m = n if max_entries is None else max_entries
    mb, rows, slots, (cnt, w) = IR.export_ref(img, C, B, first, n, m)
    count = torch.full((2,), -1, dtype=torch.int64, device=dev)
    kw = dict(first_slot=first, nslots=nslots, count=count, workspace=workspace, stream=stream)
    if form == "record":
        S = 24 + B + row_pad
        buf, body = guarded(dev, m * S, 64)
        rec = body.view(m, S)
        got = tab.export_records(rec, **kw)
        want_piece = 8 if m else None
    else:
        RS = B + row_pad
        rf = RS if rows_front is None else rows_front
        mbuf, mv = guarded(dev, 8 * m, 64)
        rbuf, rv = guarded(dev, RS * m, rf)
        sbuf, sv = guarded(dev, 4 * m, 64)
        rows_t = rv.view(m, RS)[:, :B] if with_rows else None
        slots_t = sv.view(torch.int32) if with_slots else None
        got = tab.export(mv.view(torch.int64), rows_t, slots_t, **kw)
        p16 = B % 16 == 0 and RS % 16 == 0 and rf % 16 == 0
        want_piece = None if m == 0 else 0 if not with_rows else 16 if p16 else 8
    if piece == "auto":
        piece = want_piece
    assert P.last_kernel() == tag_for(piece), (P.last_kernel(), piece)
    if stream is not None:
        stream.synchronize()
    assert got is count and tuple(count.cpu().tolist()) == (cnt, w)
    if form == "record":
        d = buf.cpu().numpy()
        assert (d[:64] == GUARD).all() and (d[64 + m * S:] == GUARD).all()
        r = d[64:64 + m * S].reshape(m, S)
        assert (r[:w, 12:16].copy().view(np.uint32).ravel() == slots).all()
        assert (r[:w, 16:24].copy().view(np.uint64).ravel() == mb).all()
        assert (r[:w, 24:24 + B] == rows).all()
        assert (r[:w, :12] == GUARD).all() and (r[:w, 24 + B:] == GUARD).all()  # +0 .. +11 and the pad: left alone
        assert (r[w:] == GUARD).all()  # nothing at or beyond entry max_entries
    else:
        d = mbuf.cpu().numpy()
        assert (d[:64] == GUARD).all() and (d[64 + 8 * w:] == GUARD).all()
        assert (d[64:64 + 8 * w].view(np.uint64) == mb).all()
        d = rbuf.cpu().numpy()
        if with_rows:
            assert (d[:rf] == GUARD).all() and (d[rf + RS * w:] == GUARD).all()
            r = d[rf:rf + RS * w].reshape(w, RS)
            assert (r[:, :B] == rows).all() and (r[:, B:] == GUARD).all()  # no byte between rows
        else:
            assert (d == GUARD).all()
        d = sbuf.cpu().numpy()
        if with_slots:
            assert (d[:64] == GUARD).all() and (d[64 + 4 * w:] == GUARD).all()
            assert (d[64:64 + 4 * w].view(np.uint32) == slots).all()
        else:
            assert (d == GUARD).all()
    return mb, rows, slots, (cnt, w)


# ------------------------------------------------------- 1. slot patterns ---
def slot_patterns(C):
    pats = {
        "none": [],
        "all": range(C + 1),
        "slot 0": [0],
        "slot C-1": [C - 1],
        "private": [C],
        "even": range(0, C + 1, 2),
        "odd": range(1, C + 1, 2),
        # a short run across every multiple of 64 (and so of T), the private slot's boundary included
        "straddle": [s for b in range(64, C + 1, 64) for s in range(b - 2, min(b + 2, C + 1))],
    }
    if C >= 4 * T:  # a tile left empty between two full ones, and the last whole tile empty as well
        pats["tiles"] = list(range(0, T)) + list(range(2 * T, 3 * T))
    return pats


def run_slot_patterns(dev, C, B):
    for k, (name, live) in enumerate(slot_patterns(C).items()):
        live = list(live)
        tab, img = forged_table(dev, C, B, live, seed=k)
        for form in ("dense", "record"):
            mb, rows, slots, cnt = check_export(tab, img, dev, form=form)
            assert slots.tolist() == live and cnt == (len(live), len(live)), name
            if live and live[-1] == C:
                assert mb[-1] == 0 and img[64 + 8 * C] == 1  # the private slot exports mbits 0, not its tag
            assert (mb[slots < C] != 0).all()


@pytest.mark.parametrize("B", [8, 16])
@pytest.mark.parametrize("C", [64, 4096])
def test_slot_patterns_on_forged_storage(dev, C, B):
    """Tags and rows written straight into table.storage: this pins the layout of DESIGN.md 4.7 (tags at
    +64, rows behind tags and winner words, the private slot at index C with tag 1)."""
    run_slot_patterns(dev, C, B)


# ---------------------------------------------------- 2. ranges and paging ---
@pytest.fixture(scope="module")
def loaded(dev):
    """Capacity 4096 at load ~0.6, built by put_records of distinct mbits plus mbits 0, and its storage
    image (made once, never written)."""
    C, B = 4096, 16
    mb = np.concatenate([distinct_mbits(2457, 900), np.zeros(1, np.uint64)])
    rows = rows_for(len(mb), B, 900)
    tab = P.DeviceTable(C, B, dev)
    st = tab.put_records(rec_to_dev(forge(mb, rows, 24 + B), dev))
    assert int(st.count_nonzero()) == 0 and tab.counts()[:3] == (2458, 0, 1)
    img = image(tab)
    img.setflags(write=False)
    return tab, img, mb, rows


FIRSTS = (0, 1, 63, 64, 65, T - 1, T, T + 1, 4095, 4096)


def run_ranges(dev, tab, img):
    C = tab.capacity
    for first in FIRSTS:
        for n in (1, 64, None):
            n = None if n is None or first + n > C + 1 else n
            check_export(tab, img, dev, first=first, nslots=n, form="record" if first % 2 else "dense")


def test_ranges(dev, loaded):
    """first_slot at and around multiples of 64 and of T, at C - 1 and at the private slot; 1 slot, 64 slots,
    to the end."""
    tab, img, _, _ = loaded
    run_ranges(dev, tab, img)


@pytest.mark.parametrize("me", [1, 63, 64, 65, 1000])
def test_paging(dev, loaded, me):
    """The whole table in pages of max_entries, resuming at the last slot + 1: the pages' concatenation is
    the single export, count2[0] of each page is the model's count of the rest, and entry max_entries of
    every buffer keeps its guard."""
    tab, img, _, _ = loaded
    C, B = tab.capacity, tab.rowbytes
    all_mb, all_rows, all_slots, (total, _) = IR.export_ref(img, C, B)
    assert total == 2458
    mbits = torch.empty(me + 1, dtype=torch.int64, device=dev)
    rows = torch.empty((me + 1, B), dtype=torch.uint8, device=dev)
    slots = torch.empty(me + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(P.table_export_workspace_bytes(C + 1), dtype=torch.uint8, device=dev)
    got_mb, got_rows, got_slots = [], [], []
    first, done = 0, 0
    while first <= C:
        for t in (mbits, rows, slots):
            t.view(torch.uint8).fill_(GUARD)
        cnt = tab.export(mbits[:me], rows[:me], slots[:me], first_slot=first, workspace=ws).cpu().tolist()
        assert cnt == [total - done, min(total - done, me)]
        w = cnt[1]
        if w == 0:
            break
        m_, r_, s_ = mbits.cpu().numpy(), rows.cpu().numpy(), slots.cpu().numpy()
        assert (m_[w:].view(np.uint8) == GUARD).all() and (r_[w:] == GUARD).all()
        assert (s_[w:].view(np.uint8) == GUARD).all()
        got_mb.append(m_[:w].view(np.uint64).copy())
        got_rows.append(r_[:w].copy())
        got_slots.append(s_[:w].view(np.uint32).copy())
        done += w
        first = int(got_slots[-1][-1]) + 1
    assert done == total
    assert (np.concatenate(got_mb) == all_mb).all() and (np.concatenate(got_slots) == all_slots).all()
    assert (np.concatenate(got_rows) == all_rows).all()


def test_cut_in_the_middle_of_a_tile(dev, loaded):
    """max_entries inside the first, a middle and the last tile, and one past the count."""
    tab, img, _, _ = loaded
    for me in (5, 700, 1500, 2457, 2458, 2459):
        for form in ("dense", "record"):
            _, _, _, cnt = check_export(tab, img, dev, max_entries=me, form=form)
            assert cnt == (2458, min(me, 2458))


# -------------------------------------------- 3. semantics against the put ---
def run_put_semantics(dev, B):
    C = 1024
    rng = np.random.default_rng(30 + B)
    pool = np.concatenate([distinct_mbits(400, 901), np.array([0, 1, 0xFFFFFFFFFFFFFFFF], np.uint64)])
    tab, state = P.DeviceTable(C, B, dev), None
    for k, m in enumerate((700, 500)):  # repeats inside a batch, overwrites across the two
        mb = rng.choice(pool[:300] if k == 0 else pool[150:], m)
        if k == 1:
            mb[7] = 0
        rows = rows_for(m, B, 910 + k)
        st = tab.put_records(rec_to_dev(forge(mb, rows, 24 + B), dev))
        want, state = R.put_ref(mb, rows, state)
        assert (st.cpu().numpy() == want).all()
    keys, krows = state
    mbits, rows, slots = tab.entries()
    assert mbits.dtype == torch.int64 and rows.dtype == torch.uint8 and slots.dtype == torch.int32
    assert tuple(rows.shape) == (len(keys), B) and tab.counts()[0] == len(keys) == mbits.numel()
    got = mbits.cpu().numpy().view(np.uint64)
    order = np.argsort(got, kind="stable")
    assert (got[order] == keys).all() and (rows.cpu().numpy()[order] == krows).all()
    s = slots.cpu().numpy()
    assert (np.diff(s) > 0).all() and s[-1] == C and got[-1] == 0  # slot order; mbits 0 last, in its own slot
    check_export(tab, image(tab), dev, form="record")


@pytest.mark.parametrize("B", [8, 40])
def test_export_after_puts_equals_the_reference_state(dev, B):
    """Two put batches with repeats and overwrites (table_ref.put_ref): the exported (mbits, row) pairs,
    sorted by mbits, are the reference state, and count2[0] == counts()[0]."""
    run_put_semantics(dev, B)


# ------------------------------------------------------------ 4. count-only ---
def test_count_only(dev, loaded):
    tab, img, _, _ = loaded
    for first, n in ((0, None), (65, 64), (4096, 1), (T - 1, 2)):
        want = IR.export_ref(img, 4096, 16, first, n, 0)[3]
        for mbits in (None, torch.empty(0, dtype=torch.int64, device=dev)):
            cnt = tab.export(mbits, first_slot=first, nslots=n)  # NULL outputs
            assert P.last_kernel() == f"{CHAIN}<0>"
            assert tuple(cnt.cpu().tolist()) == want and want[1] == 0
        check_export(tab, img, dev, first=first, nslots=n, max_entries=0)
        check_export(tab, img, dev, first=first, nslots=n, max_entries=0, form="record")


# ----------------------------------------------------------- 5. piece widths ---
def test_piece_widths(dev, loaded):
    """Rows move in 16-byte pieces when rowbytes, rows_out and row_stride are all multiples of 16, else in
    8-byte ones; a record buffer of stride 24 + rowbytes always takes <8>."""
    tab, img, _, _ = loaded
    assert tab.rowbytes == 16
    check_export(tab, img, dev, piece=16)                           # dense
    check_export(tab, img, dev, rows_front=24, piece=8)             # the same off by 8 bytes
    check_export(tab, img, dev, row_pad=8, rows_front=32, piece=8)  # a stride of 24
    check_export(tab, img, dev, row_pad=16, piece=16)               # a stride of 32
    check_export(tab, img, dev, form="record", piece=8)
    check_export(tab, img, dev, form="record", row_pad=8, piece=8)  # stride 48 from a 16-byte aligned base
    check_export(tab, img, dev, with_rows=False, piece=0)           # mbits and slot indices only
    check_export(tab, img, dev, with_slots=False, piece=16)
    check_export(tab, img, dev, with_rows=False, with_slots=False, piece=0)
    # records wider than their row from a base of 8 mod 16: the rows at +24 are 16-byte aligned
    m, S = 4097, 48
    buf, body = guarded(dev, m * S, 72)
    assert body.data_ptr() % 16 == 8
    cnt = tab.export_records(body.view(m, S))
    assert P.last_kernel() == tag_for(16)
    mb, rows, slots, (n, w) = IR.export_ref(img, 4096, 16)
    assert tuple(cnt.cpu().tolist()) == (n, w)
    d = buf.cpu().numpy()
    r = d[72:72 + m * S].reshape(m, S)
    assert (r[:w, 16:24].copy().view(np.uint64).ravel() == mb).all() and (r[:w, 24:40] == rows).all()
    assert (r[:w, 12:16].copy().view(np.uint32).ravel() == slots).all()
    assert (r[:w, :12] == GUARD).all() and (r[:w, 40:] == GUARD).all() and (r[w:] == GUARD).all()
    assert (d[:72] == GUARD).all() and (d[72 + m * S:] == GUARD).all()


# -------------------------------------------------------------- 6. wide rows ---
WIDE8 = (504, 512, 520, 1032)     # 63, 64, 65, 129 pieces of 8 bytes
WIDE16 = (1008, 1024, 1040, 2064)  # the same of 16


@pytest.mark.parametrize("B,piece", [(B, 8) for B in WIDE8] + [(B, 16) for B in WIDE16])
def test_wide_rows(dev, B, piece):
    """Rows of 63, 64, 65 and 129 pieces for both widths: up to 64 pieces a lane group (here the whole wave)
    moves a row at once, the pieces from 64 on are the wave's sweep."""
    assert B // piece in (63, 64, 65, 129)
    C, n = 1024, 300
    mb = np.concatenate([distinct_mbits(n - 1, 902), np.zeros(1, np.uint64)])
    tab = P.DeviceTable(C, B, dev)
    st = tab.put_records(rec_to_dev(forge(mb, rows_for(n, B, 920), 24 + B), dev))
    assert int(st.count_nonzero()) == 0
    img = image(tab)
    front = B + 8 if piece == 8 and B % 16 == 0 else None  # 8-byte pieces of a row that could move in 16
    _, _, _, cnt = check_export(tab, img, dev, rows_front=front, piece=piece)
    assert cnt == (n, n)
    check_export(tab, img, dev, max_entries=77, rows_front=front, piece=piece)
    check_export(tab, img, dev, form="record", piece=8)


# ------------------------------------------------------------- 7. grid reach ---
def test_grid_reach(dev):
    """One table past the reach of every launch.  Both persistent kernels (k_table_export_count,
    k_table_export_write) run min(tiles, cus * 8) workgroups of 256 lanes, a workgroup taking one tile of
    T = 1024 slots per round, so one round of the grid covers cus * 8 * 1024 slots; k_table_export_scan is
    one workgroup of 1024 lanes that takes 1024 tiles per round.  C = 2^22: 4097 tiles, the last one the
    private slot alone (it ends inside its first wave).  rowbytes 8 at load 0.07: the table is 96 MiB."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    C, B = 1 << 22, 8
    tiles = -(-(C + 1) // T)
    assert C + 1 > cus * 8 * T and tiles > cus * 8 and tiles > 1024 and (C + 1) % T == 1
    n = 300001
    mb = np.concatenate([distinct_mbits(n - 1, 903), np.zeros(1, np.uint64)])
    rows = rows_for(n, B, 930)
    tab = P.DeviceTable(C, B, dev)
    st = tab.put_records(rec_to_dev(forge(mb, rows, 24 + B), dev))
    assert int(st.count_nonzero()) == 0
    img = image(tab)
    want_mb, want_rows, want_slots, (cnt, _) = IR.export_ref(img, C, B)
    assert cnt == n and want_slots[-1] == C
    for form in ("dense", "record"):
        check_export(tab, img, dev, max_entries=n + 3, form=form)
    check_export(tab, img, dev, first=T + 1, max_entries=n)  # tiles off the 64-slot grid of the tags
    # and what it exported is what was put
    order = np.argsort(want_mb, kind="stable")
    by_put = np.argsort(mb, kind="stable")
    assert (want_mb[order] == mb[by_put]).all() and (want_rows[order] == rows[by_put]).all()


# ------------------------------------------------- 8. workspace and buffers ---
def test_workspace_contents_are_never_read(dev, loaded):
    """A workspace of exactly the queried size between guards, prefilled with 0xFF, with zeros and with
    another call's leftovers: the three runs agree bit for bit."""
    tab, img, _, _ = loaded
    C, B = tab.capacity, tab.rowbytes
    need = P.table_export_workspace_bytes(C + 1)
    assert need == 32
    buf, ws = guarded(dev, need, 256)
    other, _ = forged_table(dev, C, B, range(0, C + 1, 3), seed=77)
    m = C + 1
    outs = []
    for fill in (0xFF, 0x00, None):
        if fill is None:
            other.export(torch.empty(m, dtype=torch.int64, device=dev), workspace=ws)
        else:
            ws.fill_(fill)
        rec = torch.full((m, 24 + B), GUARD, dtype=torch.uint8, device=dev)
        cnt = tab.export_records(rec, workspace=ws)
        outs.append((rec, cnt))
        check_export(tab, img, dev, workspace=ws)
        d = buf.cpu().numpy()
        assert (d[:256] == GUARD).all() and (d[256 + need:] == GUARD).all()
    for rec, cnt in outs[1:]:
        assert torch.equal(rec, outs[0][0]) and torch.equal(cnt, outs[0][1])
    with pytest.raises(ValueError):
        tab.export(None, workspace=ws[:need - 1])
    with pytest.raises(ValueError):
        tab.export(None, workspace=buf[8:8 + need])  # misaligned


def test_side_stream(dev, loaded):
    tab, img, _, _ = loaded
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    check_export(tab, img, dev, stream=s)
    check_export(tab, img, dev, form="record", first=65, stream=s)
    torch.cuda.synchronize(dev)


def test_captured_graph_follows_the_table(dev):
    """One captured export, replayed after a further put_records: it matches a fresh model of the new state
    (count2 comes from a kernel on every replay, and the workspace is rebuilt by every replay)."""
    C, B = 4096, 16
    tab = P.DeviceTable(C, B, dev)
    mb = distinct_mbits(1000, 904)
    tab.put_records(rec_to_dev(forge(mb, rows_for(1000, B, 940), 24 + B), dev), status=False)
    m = C + 1
    rec = torch.empty((m, 24 + B), dtype=torch.uint8, device=dev)
    count = torch.empty(2, dtype=torch.int64, device=dev)
    ws = torch.empty(P.table_export_workspace_bytes(m), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):  # warm-up outside capture
        tab.export_records(rec, count=count, workspace=ws)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tab.export_records(rec, count=count, workspace=ws)
    more = np.concatenate([distinct_mbits(700, 905), mb[:50], np.zeros(1, np.uint64)])
    for rnd in (0, 1, 2):
        if rnd == 1:
            tab.put_records(rec_to_dev(forge(more, rows_for(len(more), B, 941), 24 + B), dev), status=False)
        rec.fill_(GUARD)
        count.fill_(-1)
        ws.fill_(0xFF if rnd == 2 else 0)
        g.replay()
        torch.cuda.synchronize(dev)
        want_mb, want_rows, want_slots, (n, w) = IR.export_ref(image(tab), C, B)
        assert n == (1000 if rnd == 0 else 1701) and tuple(count.cpu().tolist()) == (n, w)
        r = rec.cpu().numpy()
        assert (r[:w, 16:24].copy().view(np.uint64).ravel() == want_mb).all() and (r[:w, 24:] == want_rows).all()
        assert (r[:w, 12:16].copy().view(np.uint32).ravel() == want_slots).all()
        assert (r[:w, :12] == GUARD).all() and (r[w:] == GUARD).all()


# ---------------------------------------------------------------- 9. rehash ---
def replies_of(tab, q, dev):
    qd = to_dev(np.asarray(q, np.uint64).view(np.int64), dev)
    return [tab.get(qd, head=head).cpu().numpy() for head in (8, 1)]


def test_rehash_lets_a_full_table_take_the_dropped_records(dev):
    """A capacity-64 table is filled until a batch reports drops; rehash(128), the dropped records put
    again: all stored, and get of every mbits ever sent equals the reference replies."""
    B, S = 16, 40
    tab = P.DeviceTable(64, B, dev)
    mb1, rows1 = distinct_mbits(50, 906), rows_for(50, B, 950)
    st = tab.put_records(rec_to_dev(forge(mb1, rows1, S), dev))
    assert int(st.count_nonzero()) == 0
    mb2 = np.concatenate([distinct_mbits(30, 907), np.zeros(1, np.uint64), mb1[:5]])
    rows2 = rows_for(len(mb2), B, 951)
    rec2 = rec_to_dev(forge(mb2, rows2, S), dev)
    st2 = tab.put_records(rec2).cpu().numpy()
    lost = st2 == 2
    assert lost.sum() == 16 and tab.counts()[:3] == (65, 16, 2)  # 64 slots and the private one; a full owner
    _, state = R.put_ref(mb1, rows1)
    _, state = R.put_ref(mb2[~lost], rows2[~lost], state)
    old = tab.storage.clone()
    big = tab.rehash(128)
    assert (big.capacity, big.rowbytes) == (128, B) and big.counts()[:3] == (65, 0, 1)
    assert torch.equal(tab.storage, old)
    st3 = big.put_records(rec2[torch.from_numpy(np.flatnonzero(lost)).to(dev)].contiguous())
    assert int(st3.count_nonzero()) == 0 and big.counts()[:3] == (81, 0, 2)
    _, state = R.put_ref(mb2[lost], rows2[lost], state)
    q = np.concatenate([mb1, mb2, distinct_mbits(9, 908)])
    for head, got in zip((8, 1), replies_of(big, q, dev)):
        assert (got == R.replies_ref(state, q, head, B)).all()
    # a full table into one of its own capacity: 65 entries fit 64 slots only because mbits 0 is among them
    same = tab.rehash(64)
    assert same.counts()[:3] == (65, 0, 1)
    q = np.concatenate([mb1, mb2])
    for a, b in zip(replies_of(tab, q, dev), replies_of(same, q, dev)):
        assert (a == b).all()
    with pytest.raises(ValueError, match="do not fit"):
        big.rehash(64)  # 81 entries
    t65 = P.DeviceTable(128, B, dev)
    t65.put_records(rec_to_dev(forge(distinct_mbits(65, 909), rows_for(65, B, 952), S), dev), status=False)
    with pytest.raises(ValueError, match="do not fit"):
        t65.rehash(64)  # 65 ordinary entries, no mbits 0


@pytest.mark.parametrize("capacity,chunk_slots", [(4096, None), (1 << 20, 1500), (8192, 4097)])
def test_rehash_keeps_every_reply(dev, loaded, capacity, chunk_slots):
    """rehash to the same capacity and to 2^20 in 3 chunks: the replies for present and absent mbits are
    byte-identical before and after, the old table is unchanged, and the new table's counters are entries =
    the old one's, dropped 0, batches = the chunks that held an entry."""
    tab, img, mb, _ = loaded
    C, B = tab.capacity, tab.rowbytes
    S = 24 + B
    old = tab.storage.clone()
    q = np.concatenate([mb, distinct_mbits(500, 910)])
    before = replies_of(tab, q, dev)
    new = tab.rehash(capacity) if chunk_slots is None else tab.rehash(capacity, chunk_bytes=chunk_slots * S + 7)
    per = C + 1 if chunk_slots is None else chunk_slots
    live = IR.export_ref(img, C, B)[2]
    chunks = len(np.unique(live // per))
    assert chunks == (3 if chunk_slots == 1500 else 1)
    assert new.counts()[:3] == (2458, 0, chunks) and new.capacity == capacity
    assert torch.equal(tab.storage, old)
    for a, b in zip(before, replies_of(new, q, dev)):
        assert (a == b).all()
    with pytest.raises(ValueError, match="do not fit"):
        tab.rehash(2048)


def test_rehash_slot_by_slot(dev):
    """chunk_bytes of one record: every slot is a chunk of its own, and only the live ones become batches."""
    B = 16
    small, _ = forged_table(dev, 64, B, [0, 5, 6, 63, 64], seed=5)
    new = small.rehash(64, chunk_bytes=24 + B)
    assert new.counts()[:3] == (5, 0, 5)
    a = sorted(zip(*[t.cpu().numpy().tolist() for t in small.entries()[:2]]))
    b = sorted(zip(*[t.cpu().numpy().tolist() for t in new.entries()[:2]]))
    assert a == b and len(a) == 5 and sum(1 for mbits, _ in a if mbits == 0) == 1


def test_rehash_on_a_side_stream_and_caller_storage(dev, loaded):
    tab, img, mb, _ = loaded
    B = tab.rowbytes
    buf = torch.full((P.table_bytes(8192, B) + 512,), GUARD, dtype=torch.uint8, device=dev)
    storage = buf[256:256 + P.table_bytes(8192, B)]
    s = torch.cuda.Stream(dev)
    new = tab.rehash(8192, storage=storage, chunk_bytes=2000 * (24 + B), stream=s)
    s.synchronize()
    assert new.storage.data_ptr() == storage.data_ptr() and new.counts()[:3] == (2458, 0, 3)
    d = buf.cpu().numpy()
    assert (d[:256] == GUARD).all() and (d[256 + new.nbytes:] == GUARD).all()
    for a, b in zip(replies_of(tab, mb, dev), replies_of(new, mb, dev)):
        assert (a == b).all()


# ---------------------------------------------------------- 10. A/B variants ---
@pytest.mark.tuning
@pytest.mark.parametrize("variant", [0, 342, 343])
def test_export_variants(dev, variant):
    """Tuning variants 342 (the export's outputs stored in the other policy) and 343 (the write pass reads
    ballot masks saved by the count pass instead of the tags again): cases 1-3 through the tuning build."""
    with P.tuning(variant):
        run_slot_patterns(dev, 4096, 16)
        run_slot_patterns(dev, 64, 8)
        mb = np.concatenate([distinct_mbits(2457, 900), np.zeros(1, np.uint64)])
        tab = P.DeviceTable(4096, 16, dev)
        tab.put_records(rec_to_dev(forge(mb, rows_for(len(mb), 16, 900), 40), dev), status=False)
        run_ranges(dev, tab, image(tab))
        run_put_semantics(dev, 40)
