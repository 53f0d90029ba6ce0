"""GPU checks of the table's reduce (include/pdht_hip_table_reduce.h): after every call the status, the
replies (between guard bytes), the four counters and the table -- a get of every mbits plus absent ones --
against the sequential model of tests/table_reduce_ref.py, which applies one record after the other and
knows nothing of waves, atomics or identities.  Byte for byte for every op and type; ADD on doubles runs on
integer-valued doubles, where every order of the additions gives the same bits (the any-order bound of the
double sum is tests/test_gpu_table_acc.py's).  Operands are bit patterns throughout -- the doubles too, so
that no floating-point instruction of the test touches a NaN's payload.  Tables have 64 or 256 slots except
where a batch has to outgrow the grid."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

import table_reduce_ref as R  # noqa: E402
from test_gpu_table import distinct_mbits, forge, rec_to_dev, rows_for, to_dev  # noqa: E402
from test_gpu_table_acc import batch_shapes, check_table, filled, i64, rows_with  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = {"i32": (torch.int32, np.int32, np.uint32), "i64": (torch.int64, np.int64, np.uint64),
         "f64": (torch.float64, np.float64, np.uint64)}  # torch dtype, the model's, the words the test handles
BITWISE = ("and", "or", "xor")
COMBOS = [(k, o) for k in KINDS for o in R.OPS if not (k == "f64" and o in BITWISE)]  # 15


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------- helpers ---
def specials(kind, op):
    """The operands that decide: INT_MIN, INT_MAX, -1, 0, 1 of the width (a min that compared unsigned fails on
    them; every op's identity is among them), the masks for the bitwise ops, one of every kind of double."""
    if kind == "f64":
        return np.array(R.LADDER, np.uint64)
    w = 32 if kind == "i32" else 64
    v = [1 << (w - 1), (1 << (w - 1)) - 1, (1 << w) - 1, 0, 1]
    if op in BITWISE:
        v += [0xAAAAAAAAAAAAAAAA >> (64 - w), 0x5555555555555555 >> (64 - w)]
    return np.array(v, np.uint64).astype(KINDS[kind][2])


def operands(kind, op, m, elems, seed, special=0.3):
    """[m, elems] words: random ones over the whole range (doubles: over every exponent, both signs) with the
    specials mixed in.  ADD on doubles: integer-valued, |x| < 2^20, so that any order adds to the same bits."""
    rng = np.random.default_rng(seed)
    if kind == "f64" and op == "add":
        return rng.integers(-(1 << 20), 1 << 20, (m, elems)).astype(np.float64).view(np.uint64)
    if kind == "f64":
        with np.errstate(over="ignore"):  # (down into the subnormals and up to the largest exponent)
            v = np.ldexp(rng.standard_normal((m, elems)), rng.integers(-1080, 1022, (m, elems))).view(np.uint64).copy()
    else:
        v = rng.integers(0, 1 << (32 if kind == "i32" else 64), (m, elems), dtype=np.uint64).astype(KINDS[kind][2])
    if kind == "f64" or op != "add":
        sp = specials(kind, op)
        at = rng.random((m, elems)) < special
        v[at] = sp[rng.integers(0, len(sp), int(at.sum()))]
    return v


def reply_tag(B, off, S):
    return 16 if off % 16 == 0 and S % 16 == 0 and (B // 8 + 1) % 2 == 0 else 8


def tag_of(kind, op, insert, reply=None):
    t = kind + ("" if op == "add" else "," + op)
    name = f"k_table_acc_claim+k_table_acc<{t},insert>" if insert else f"k_table_acc<{t}>"
    return name + (f"+k_table_add_reply<{reply}>" if reply else "")


def run_red(tab, state, mb, rows, kind, op, vo, elems, dev, insert=False, replies=True, status=True, stride=None,
            dropped_ok=False, pad=0, off=0, **kw):
    """One reduce batch on the device and on the model: last_kernel, status, replies between guard bytes (at
    `off` bytes past a 16-byte boundary, `pad` bytes between them) and counters compared.  dropped_ok: the
    batch may overflow; the set of dropped mbits is then read from the device's status (which new mbits lose
    is the schedule's choice) and checked for consistency here.  Returns (status, the dropped mbits)."""
    tdt, ndt, _ = KINDS[kind]
    B, m = tab.rowbytes, len(mb)
    rec = rec_to_dev(forge(mb, rows, stride or 24 + B), dev)
    before, had = tab.counts(), set(state)
    S = 8 + B + pad
    buf = view = None
    if replies:
        buf = torch.full((m * S + 64,), 0xA5, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 16 == 0
        view = buf[16 + off:16 + off + m * S].view(m, S)[:, :8 + B]
    out = tab.reduce_records(rec, tdt, op, vo, elems, insert=insert, status=status, replies=view, **kw)
    assert P.last_kernel() == tag_of(kind, op, insert, reply_tag(B, off, S) if replies else None)
    st = out[0] if replies else out
    assert (st is None) == (not status)
    mb = np.asarray(mb, np.uint64)
    lost = set()
    if st is not None:
        got = st.cpu().numpy()
        lost = set(mb[got == 2].tolist())
    if lost:
        assert dropped_ok and insert
        assert not (lost & set(mb[got != 2].tolist()))  # all records of one mbits share one fate
        assert not (lost & had) and 0 not in lost        # present mbits and mbits 0 are never dropped
    want, want_rep = R.reduce_ref(state, mb, rows, ndt, op, vo, elems, insert, dropped=lost, capacity=tab.capacity)
    if st is not None:
        assert (got == want).all()
    else:
        assert not (want == 2).any()  # (without a status the batch must not overflow: nobody could say who lost)
    if replies:
        assert out[1].data_ptr() == view.data_ptr()
        d = buf.cpu().numpy()
        body = d[16 + off:16 + off + m * S].reshape(m, S)
        bad = np.flatnonzero((body[:, :8 + B] != want_rep).any(axis=1))
        assert len(bad) == 0, (bad[:5], body[bad[:2], :8 + B], want_rep[bad[:2]])
        assert (body[:, 8 + B:] == 0xA5).all() and (d[:16 + off] == 0xA5).all() and (d[16 + off + m * S:] == 0xA5).all()
    after = tab.counts()
    if not insert or m == 0:
        assert after == before  # no winner words, no batch number, nothing inserted, dropped or counted
    else:
        new = len(set(state) - had)
        assert after[:3] == (before[0] + new, before[1] + int((want == 2).sum()), before[2] + 1)
        assert after[3] - before[3] >= m  # every record inspects at least one slot
        assert after[0] == len(state)
    return want, lost


def held_table(dev, C, B, vo, kind, op, elems, n, seed):
    """A table of n entries whose regions hold operands of the kind (specials among them), and its state."""
    held = distinct_mbits(n, seed)
    tab, state = filled(dev, C, B, held, rows_with(n, B, vo, operands(kind, op, n, elems, seed), seed))
    return held, tab, state


# ===================================================== types x ops x regions ===
ELEMS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 129)


def regions(kind):
    """(B, vo, elems): every offset of the type (i32 at 0 / 4 / 12, the others at 0 / 8 / 24) and every group
    width, the combining limit on both sides (32 / 33) and the wave sweep (64 / 65 / 129); rows from 8 bytes
    up, the region at the row's end, in its middle or all of it."""
    size = 4 if kind == "i32" else 8
    out = []
    for i, e in enumerate(ELEMS):
        vo = ((0, 4, 12) if kind == "i32" else (0, 8, 24))[i % 3]
        B = (vo + e * size + 7) // 8 * 8 + (8 if i % 2 else 0)
        out.append((B, vo, e))
    out += [(8, 8 - size, 1), (16, 8, 1), (528, 24 if size == 8 else 12, 63 if size == 8 else 129)]
    return out


@pytest.mark.parametrize("kind,op", COMBOS)
def test_types_ops_and_regions(dev, kind, op):
    """Every type x op at every alignment of its region, groups of 1 .. 64 lanes and regions of more elements
    than a wave has lanes; a record stride with noise behind the row; noise in every row byte outside the
    region, which survives on present entries; repeats and absent mbits in the batch; replies from the slot
    store of flags 0.  Then the same batch once more with INSERT, which creates the absent ones."""
    C, n, m = 256, 40, 200
    for B, vo, elems in regions(kind):
        seed = 7000 + B * 7 + vo * 3 + elems
        held, tab, state = held_table(dev, C, B, vo, kind, op, elems, n, seed)
        absent = distinct_mbits(12, seed + 1)
        pool = np.concatenate([held, absent])
        mb = pool[np.random.default_rng(seed).integers(0, len(pool), m)]
        rows = rows_with(m, B, vo, operands(kind, op, m, elems, seed + 2), seed + 2)
        size = 4 if kind == "i32" else 8
        outside = {k: np.delete(v, np.s_[vo:vo + elems * size]) for k, v in state.items()}
        st, _ = run_red(tab, state, mb, rows, kind, op, vo, elems, dev, stride=24 + B + (16 if elems % 2 else 0))
        assert (st == np.where(np.isin(mb, held), 0, 3)).all() and set(state) == set(outside)
        for k, v in state.items():  # the model itself left the bytes outside the region alone
            assert (np.delete(v, np.s_[vo:vo + elems * size]) == outside[k]).all()
        check_table(tab, state, pool, dev)
        st, _ = run_red(tab, state, mb, rows, kind, op, vo, elems, dev, insert=True, stride=24 + B + 8, pad=8)
        assert (st == 0).all() and len(state) == n + len(np.unique(mb[np.isin(mb, absent)]))
        check_table(tab, state, pool, dev)


# ======================================================== batch sizes ===
SMALL = [("i64", "min", 16, 8, 1), ("i32", "xor", 24, 4, 3), ("f64", "max", 24, 8, 2), ("i32", "max", 8, 4, 1),
         ("f64", "min", 8, 0, 1), ("i64", "or", 40, 8, 4)]


@pytest.mark.parametrize("kind,op,B,vo,elems", SMALL)
@pytest.mark.parametrize("m", [1, 63, 64, 65, 4097])
def test_batch_sizes_half_absent(dev, m, kind, op, B, vo, elems):
    """1, a wave less one, a wave, a wave and one, and 4097 records, every other one on an absent mbits:
    flags 0 answers them 3 and zeros, INSERT creates them."""
    held, tab, state = held_table(dev, 256, B, vo, kind, op, elems, 60, 7100)
    absent = distinct_mbits(60, 7101)
    rng = np.random.default_rng(7102 + m)
    mb = np.where(np.arange(m) % 2 == 0, held[rng.integers(0, 60, m)], absent[rng.integers(0, 60, m)])
    rows = rows_with(m, B, vo, operands(kind, op, m, elems, 7103 + m), 7103)
    st, _ = run_red(tab, state, mb, rows, kind, op, vo, elems, dev)
    assert (st == np.where(np.arange(m) % 2 == 0, 0, 3)).all()
    check_table(tab, state, np.concatenate([held, absent]), dev)
    st, _ = run_red(tab, state, mb, rows, kind, op, vo, elems, dev, insert=True)
    assert (st == 0).all()
    check_table(tab, state, np.concatenate([held, absent]), dev)


# ========================================================== duplicates ===
def dup_shapes(h, absent):
    """tests/test_gpu_table_acc.py's shapes (lanes that share a slot fold first, two leaders per wave, the
    lanes left over post on their own; a repeat in a wave's last two lanes) and: one mbits 4097 times, two
    alternating over 4097 records, mbits 0 and 1 side by side."""
    s = dict(batch_shapes(h, absent))
    s["one_mbits_4097"] = np.full(4097, h[7])
    s["two_alternating_4097"] = np.tile(h[[3, 4]], 2049)[:4097]
    s["mbits_zero_and_one"] = np.concatenate([np.tile(np.array([0, 1], np.uint64), 100), h[1:3], np.ones(3, np.uint64)])
    return s


DUPS = sorted(dup_shapes(np.arange(100, dtype=np.uint64), np.arange(100, 110, dtype=np.uint64)))
DUP_REGIONS = [("i64", "min", 16, 8, 1), ("i32", "or", 24, 4, 3), ("f64", "min", 24, 8, 2), ("f64", "max", 8, 0, 1),
               ("i32", "and", 8, 4, 1), ("i64", "max", 272, 8, 33), ("f64", "max", 272, 8, 33), ("i64", "xor", 16, 0, 2)]


@pytest.mark.parametrize("kind,op,B,vo,elems", DUP_REGIONS)
@pytest.mark.parametrize("shape", DUPS)
def test_duplicates_within_and_across_waves(dev, shape, kind, op, B, vo, elems):
    """Present-only with replies, then INSERT on an empty table: every mbits of the batch is new, created from
    its first record, and its region is the op over all its records.  33 elements: one record per wave, every
    operand an atomic of its own (hot batches of that kind stay at 4097 records)."""
    n = 80
    held = np.concatenate([np.array([0, 1], np.uint64), distinct_mbits(n - 2, 7200)])
    absent = distinct_mbits(10, 7201)
    mb = dup_shapes(held, absent)[shape]
    m, seed = len(mb), 7202 + len(shape)
    tab, state = filled(dev, 256, B, held, rows_with(n, B, vo, operands(kind, op, n, elems, seed), seed))
    rows = rows_with(m, B, vo, operands(kind, op, m, elems, seed + 1), seed + 1)
    st, _ = run_red(tab, state, mb, rows, kind, op, vo, elems, dev)
    assert (st == np.where(np.isin(mb, held), 0, 3)).all()
    check_table(tab, state, np.concatenate([held, absent]), dev)
    fresh, state = P.DeviceTable(256, B, dev), {}
    st, _ = run_red(fresh, state, mb, rows, kind, op, vo, elems, dev, insert=True)
    assert (st == 0).all() and set(state) == set(np.unique(mb).tolist())
    first = {int(k): rows[i] for i, k in reversed(list(enumerate(mb)))}
    region = np.s_[vo:vo + elems * (4 if kind == "i32" else 8)]
    for k, v in state.items():  # everything outside the region is the FIRST record's
        assert (np.delete(v, region) == np.delete(first[k], region)).all()
    check_table(fresh, state, np.concatenate([held, absent]), dev)


@pytest.mark.parametrize("kind,op,B,vo,elems,insert", [("i64", "min", 8, 0, 1, True), ("f64", "max", 16, 8, 1, False),
                                                        ("i32", "or", 8, 0, 2, False)])
def test_second_round_of_the_grid_with_a_hot_mbits(dev, kind, op, B, vo, elems, insert):
    """2^20 + 13 records, 90 % of them on one mbits: past the reach of one round of the grids (8 workgroups of
    256 lanes per CU), the last wave partly past the end; most waves fold the hot slot's operands and post once
    between them.  Regions of at most 32 elements only."""
    m = (1 << 20) + 13
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert m > cus * 8 * 256 and m % 64
    keys = distinct_mbits(200, 7300)
    tab, state = filled(dev, 256, B, keys[:100], rows_with(100, B, vo, operands(kind, op, 100, elems, 7300), 7300))
    rng = np.random.default_rng(7301)
    mb = keys[rng.integers(0, 200, m)]
    mb[rng.random(m) < 0.9] = keys[150 if insert else 50]
    rows = rows_with(m, B, vo, operands(kind, op, m, elems, 7302, special=0.01), 7302)
    st, _ = run_red(tab, state, mb, rows, kind, op, vo, elems, dev, insert=insert)
    assert set(np.unique(st)) == ({0} if insert else {0, 3})
    check_table(tab, state, keys, dev)


def test_three_runs_leave_identical_bytes(dev):
    """A duplicate-heavy batch three times on equal tables, for an op of every family and doubles: table and
    replies are the same bytes on every run (and the model's: run_red)."""
    m = 4097
    for kind, op, B, vo, elems in [("f64", "min", 24, 8, 2), ("f64", "max", 272, 8, 33), ("i64", "xor", 16, 8, 1),
                                   ("i32", "max", 16, 4, 3)]:
        keys = distinct_mbits(12, 7400)
        rng = np.random.default_rng(7401)
        mb = keys[rng.integers(0, 12, m)]
        mb[rng.random(m) < 0.5] = keys[3]
        rows = rows_with(m, B, vo, operands(kind, op, m, elems, 7402), 7402)
        seen = []
        for _ in range(3):
            tab, state = filled(dev, 64, B, keys[:6], rows_with(6, B, vo, operands(kind, op, 6, elems, 7403), 7403))
            rec = rec_to_dev(forge(mb, rows, 24 + B), dev)
            st, rep = tab.reduce_records(rec, KINDS[kind][0], op, vo, elems, insert=True, replies=True)
            seen.append((st.cpu().numpy().tobytes(), rep.cpu().numpy().tobytes(),
                         tab.get(i64(keys, dev)).cpu().numpy().tobytes()))
        assert seen[0] == seen[1] == seen[2]
        want, want_rep = R.reduce_ref(state, mb, rows, KINDS[kind][1], op, vo, elems, True, capacity=64)
        assert seen[2][0] == want.tobytes() and seen[2][1] == want_rep.tobytes()  # and they are the model's
        check_table(tab, state, keys, dev)


# ============================================================ operands ===
@pytest.mark.parametrize("kind", ["i32", "i64"])
@pytest.mark.parametrize("op", ["min", "max", "and", "or", "xor"])
def test_integer_extremes_and_masks(dev, kind, op):
    """Nothing but INT_MIN, INT_MAX, -1, 0, 1 (and for the bitwise ops all ones, zero and the alternating
    masks), as operands and as what the entries hold: a min or max that compared unsigned gets -1 against 0
    wrong, one that compared a narrower or wider word gets INT_MIN against INT_MAX wrong."""
    B, vo, elems, n, m = 24, 8, 2 if kind == "i64" else 3, 30, 700
    sp = specials(kind, op)
    rng = np.random.default_rng(7500)
    held = distinct_mbits(n, 7500)
    tab, state = filled(dev, 64, B, held, rows_with(n, B, vo, sp[rng.integers(0, len(sp), (n, elems))], 7500))
    mb = held[rng.integers(0, n, m)]
    mb[::3] = held[2]
    rows = rows_with(m, B, vo, sp[rng.integers(0, len(sp), (m, elems))], 7501)
    run_red(tab, state, mb, rows, kind, op, vo, elems, dev)
    check_table(tab, state, held, dev)
    # each pair on an entry of its own, one record each: nothing folds, the atomic alone decides
    pairs = [(a, b) for a in sp for b in sp]
    held = distinct_mbits(len(pairs), 7502)
    old = np.array([[a] * elems for a, _ in pairs], KINDS[kind][2])
    new = np.array([[b] * elems for _, b in pairs], KINDS[kind][2])
    tab, state = filled(dev, 64, B, held, rows_with(len(pairs), B, vo, old, 7503))
    run_red(tab, state, held, rows_with(len(pairs), B, vo, new, 7504), kind, op, vo, elems, dev)
    check_table(tab, state, held, dev)


@pytest.mark.parametrize("op", ["min", "max"])
@pytest.mark.parametrize("B,vo,elems", [(24, 8, 2), (272, 8, 33), (8, 0, 1)])
def test_special_doubles_bit_for_bit(dev, op, B, vo, elems):
    """+-NaN with two payloads each (quiet and signalling), +-inf, +-DBL_MAX, +-subnormals and +-0.0 mixed half
    and half into random doubles, as operands and as the entries' old values; every pair of them on an entry of
    its own (the atomic alone: both signs of the operand against both signs of the word) and piled on few
    entries (the fold in key space).  Every word bit for bit: the result is one operand's bits."""
    sp = specials("f64", op)
    pairs = [(a, b) for a in sp for b in sp]
    held = distinct_mbits(len(pairs), 7600)  # 400 entries
    old = np.array([[a] * elems for a, _ in pairs], np.uint64)
    new = np.array([[b] * elems for _, b in pairs], np.uint64)
    tab, state = filled(dev, 1024, B, held, rows_with(len(pairs), B, vo, old, 7600))
    run_red(tab, state, held, rows_with(len(pairs), B, vo, new, 7601), "f64", op, vo, elems, dev)
    check_table(tab, state, held, dev)
    for (a, b), k in zip(pairs, held.tolist()):  # the model's own answer, spelt out: one of the two words
        w = state[k][vo:vo + 8].view(np.uint64)[0]
        assert w in (a, b) and w == R.reduce_word(R.OPS[op], np.float64, a, b)
    n, m = 20, 1500
    held, tab, state = held_table(dev, 64, B, vo, "f64", op, elems, n, 7602)
    rng = np.random.default_rng(7603)
    mb = held[rng.integers(0, n, m)]
    mb[rng.random(m) < 0.4] = held[5]
    rows = rows_with(m, B, vo, operands("f64", op, m, elems, 7604, special=0.5), 7604)
    run_red(tab, state, mb, rows, "f64", op, vo, elems, dev)
    check_table(tab, state, held, dev)
    fresh, state = P.DeviceTable(64, B, dev), {}
    run_red(fresh, state, mb, rows, "f64", op, vo, elems, dev, insert=True)
    check_table(fresh, state, held, dev)


# ============================================================== INSERT ===
@pytest.mark.parametrize("kind,op", COMBOS)
def test_insert_creates_from_the_first_record(dev, kind, op):
    """New mbits whose records carry different key-slot bytes, present and new ones side by side in one wave,
    mbits 0 created: the bytes outside the region are the first record's, the region is the op over all records
    of the mbits.  The op's identity (INT_MAX, INT_MIN, all ones, zero; for doubles the last and the first of
    totalOrder, both NaNs) is among the operands -- as the first, as the only and as every record of an mbits."""
    B, vo, elems, n = 32, 16, 2, 30  # bytes 0..15 the "key slot", 16..31 the region
    if kind == "i32":
        elems = 3
    held, tab, state = held_table(dev, 256, B, vo, kind, op, elems, n, 7700)
    new = np.concatenate([distinct_mbits(40, 7701), np.zeros(1, np.uint64)])
    mb = np.stack([np.tile(held[:8], 16), np.tile(new[:8], 16)], 1).ravel()  # present, new, present, new ...
    mb = np.concatenate([mb, new, new[::-1], held, np.zeros(5, np.uint64)])
    vals = operands(kind, op, len(mb), elems, 7702)
    ident = {"min": 1, "max": 0, "and": 2, "or": 3, "xor": 3, "add": 3}[op]  # its place among specials()
    if kind == "f64":
        ident = {"min": len(R.LADDER) - 1, "max": 0, "add": None}[op]
    if ident is not None:
        iv = specials(kind, op)[ident]
        firsts = np.unique(mb, return_index=True)[1]
        vals[firsts[::2]] = iv                 # the first record of every other mbits
        vals[mb == new[20]] = iv               # every record of one (it appears twice)
        vals[mb == held[20]] = iv              # the only record of a present one
    rows = rows_with(len(mb), B, vo, vals, 7702)
    first = np.unique(mb, return_index=True)[1]
    st, _ = run_red(tab, state, mb, rows, kind, op, vo, elems, dev, insert=True)
    assert (st == 0).all() and len(state) == n + 41
    for p in first:
        k = int(mb[p])
        if k not in set(held.tolist()):
            assert (state[k][:vo] == rows[p][:vo]).all()
            assert len({rows[q][:vo].tobytes() for q in np.flatnonzero(mb == mb[p])}) > 1  # the others differ
    check_table(tab, state, np.concatenate([held, new, distinct_mbits(5, 7703)]), dev)
    assert sorted(tab.entries()[0].cpu().numpy().view(np.uint64).tolist()) == sorted(state)


@pytest.mark.parametrize("kind,op,B,vo,elems", [("i64", "min", 8, 0, 1), ("i32", "xor", 40, 12, 3), ("f64", "max", 48, 8, 5),
                                                ("i64", "and", 16, 8, 1), ("f64", "add", 16, 8, 1)])
def test_insert_overflow_part_way(dev, kind, op, B, vo, elems):
    """More new mbits than free slots on a 64-slot table, each with many records, twice over: inserted =
    min(new, free); present mbits and their regions are never dropped; all records of an mbits share their
    fate (run_red checks both); and the model, fed with the set the device dropped, matches everything else --
    status, replies (zeros for the dropped), counters and every row."""
    C = 64
    rng = np.random.default_rng(7800 + B)
    old = distinct_mbits(40, 7800)
    tab, state = filled(dev, C, B, old, rows_with(40, B, vo, operands(kind, op, 40, elems, 7800), 7800))
    new = np.concatenate([distinct_mbits(100, 7801), np.array([1], np.uint64)])  # mbits 1 competes like any key
    pool = np.concatenate([old, new, np.zeros(1, np.uint64)])
    mb = np.concatenate([np.repeat(pool, 10), pool[rng.integers(0, len(pool), 4097 - 10 * len(pool))]])
    mb = mb[rng.permutation(len(mb))]
    winners = None
    for rnd in (0, 1):  # the same mbits again with new operands: tags are final
        rows = rows_with(len(mb), B, vo, operands(kind, op, len(mb), elems, 7810 + rnd), 7810 + rnd)
        before = tab.counts()
        st, lost = run_red(tab, state, mb, rows, kind, op, vo, elems, dev, insert=True, dropped_ok=True)
        won = set(state) - set(old.tolist()) - {0}
        assert won <= set(new.tolist()) and len(won) == C - 40 and len(lost) == 101 - (C - 40)
        if rnd == 0:
            winners = won
        assert won == winners and lost == set(new.tolist()) - winners
        assert tab.counts()[0] == C + 1 and \
            tab.counts()[1] - before[1] == int(np.isin(mb, np.array(sorted(lost), np.uint64)).sum())
        check_table(tab, state, np.concatenate([pool, distinct_mbits(5, 7802)]), dev)


def test_sixteen_calls_of_every_kind_across_a_clear(dev):
    """reduce (every op, with and without INSERT and replies) / put / update / acc / add in turn on one table
    over one pool of mbits, a clear in the middle: winner words, batch numbers and workspaces of earlier calls
    of any kind decide nothing later."""
    import table_acc_ref as ACC
    import table_add_ref as ADD
    import table_rmw_ref as RMW
    B, C, vo = 24, 256, 16
    pool = np.concatenate([np.zeros(1, np.uint64), distinct_mbits(130, 7900)])
    rng = np.random.default_rng(7901)
    tab, state, batches = P.DeviceTable(C, B, dev), {}, 0
    plan = [("min", True), "put", ("max", False), "update", ("or", True), "acc", ("xor", False), "add", "clear",
            ("and", True), ("add", True), "put", ("min", False), ("xor", True), "update", ("max", True), ("add", False)]
    for t, what in enumerate(plan):
        m = int(rng.integers(100, 600))
        mb = pool[rng.integers(0, 60 + 4 * t, m)]
        if what == "clear":
            tab.clear()
            state, batches = {}, 0
            continue
        if isinstance(what, tuple):
            op, insert = what
            rows = rows_with(m, B, vo, operands("i64", op, m, 1, 7910 + t), 7910 + t)
            run_red(tab, state, mb, rows, "i64", op, vo, 1, dev, insert=insert, replies=t % 3 != 0)
            batches += insert
        else:
            rows = rows_for(m, B, 7910 + t)
            rec = rec_to_dev(forge(mb, rows, 24 + B), dev)
            if what == "put":
                st = tab.put_records(rec).cpu().numpy()
                last = m - 1 - np.unique(mb[::-1], return_index=True)[1]
                want = np.ones(m, np.uint8)
                want[last] = 0
                assert (st == want).all()
                for p in last:
                    state[int(mb[p])] = rows[p].copy()
            elif what == "update":
                assert (tab.update_records(rec).cpu().numpy() == RMW.update_ref(state, mb, rows)).all()
            elif what == "acc":
                st = tab.acc_records(rec, torch.int64, vo, insert=True).cpu().numpy()
                assert (st == ACC.acc_ref(state, mb, rows, np.int64, vo, 1, True, capacity=C)[0]).all()
            else:
                assert (tab.add_records(rec).cpu().numpy() == ADD.add_ref(state, mb, rows, capacity=C)[0]).all()
            batches += 1
        assert tab.counts()[:3] == (len(state), 0, batches)
        check_table(tab, state, pool, dev)


# ====================================================== ADD equivalence ===
@pytest.mark.parametrize("kind,B,vo,elems", [("i32", 24, 4, 3), ("i64", 16, 8, 1), ("f64", 24, 8, 2), ("i64", 272, 8, 33)])
def test_add_is_the_accumulate(dev, kind, B, vo, elems):
    """ADD through the new call leaves the same table, status and counters as acc_records on a twin table, under
    the same kernel names: it is the same kernel."""
    n, m = 50, 900
    held, new = distinct_mbits(n, 8000), distinct_mbits(25, 8001)
    pool = np.concatenate([held, new, np.zeros(1, np.uint64)])
    rng = np.random.default_rng(8002)
    mb = pool[rng.integers(0, len(pool), m)]
    mb[rng.random(m) < 0.4] = held[9]
    start = rows_with(n, B, vo, operands(kind, "add", n, elems, 8003), 8003)
    rows = rows_with(m, B, vo, operands(kind, "add", m, elems, 8004), 8004)
    rec = rec_to_dev(forge(mb, rows, 24 + B), dev)
    a, state = filled(dev, 256, B, held, start)
    b, _ = filled(dev, 256, B, held, start)
    for insert in (False, True):
        sa = a.reduce_records(rec, KINDS[kind][0], P.PDHT_RED_ADD, vo, elems, insert=insert)
        ta = P.last_kernel()
        sb = b.acc_records(rec, KINDS[kind][0], vo, elems, insert=insert)
        assert ta == P.last_kernel() == tag_of(kind, "add", insert)
        assert (sa.cpu().numpy() == sb.cpu().numpy()).all() and a.counts()[:3] == b.counts()[:3]
        assert (a.get(i64(pool, dev)).cpu().numpy() == b.get(i64(pool, dev)).cpu().numpy()).all()
        # (an empty batch between; an empty tensor has no address, so it cannot ask for replies)
        run_red(a, state, mb[:0], rows[:0], kind, "add", vo, elems, dev, insert=insert, replies=False)
    sa, rep = a.reduce_records(rec, KINDS[kind][0], "add", vo, elems, replies=True)
    b.acc_records(rec, KINDS[kind][0], vo, elems)
    assert (rep.cpu().numpy() == b.get(rec).cpu().numpy()).all()  # "a get after the call"


# ================================================================ tuning ===
@pytest.mark.tuning
@pytest.mark.parametrize("kind,op,B,vo,elems", [("i64", "min", 16, 8, 1), ("i32", "max", 24, 4, 3), ("i64", "and", 16, 8, 1),
                                                ("i32", "or", 24, 4, 3), ("i64", "xor", 24, 8, 2), ("i32", "min", 8, 4, 1),
                                                ("i64", "max", 40, 8, 4), ("f64", "min", 24, 8, 2)])
def test_variant_without_the_in_wave_fold(dev, kind, op, B, vo, elems):
    """Tuning variant 344: every operand an atomic of its own, for the integer types; doubles keep the product's
    kernel under it.  Hot and mixed batches, present-only and INSERT, with replies, against the same model."""
    n = 60
    held, tab, state = held_table(dev, 256, B, vo, kind, op, elems, n, 8100)
    new = distinct_mbits(20, 8101)
    rng = np.random.default_rng(8102)
    pool = np.concatenate([held, new])
    mb = pool[rng.integers(0, len(pool), 900)]
    mb[rng.random(900) < 0.5] = held[9]
    rows = rows_with(900, B, vo, operands(kind, op, 900, elems, 8103), 8103)
    with P.tuning(344):
        run_red(tab, state, mb, rows, kind, op, vo, elems, dev)
        check_table(tab, state, pool, dev)
        run_red(tab, state, mb, rows, kind, op, vo, elems, dev, insert=True)
        check_table(tab, state, pool, dev)
    run_red(tab, state, mb, rows, kind, op, vo, elems, dev)  # and the product on the same table
    check_table(tab, state, pool, dev)


# =============================================================== replies ===
@pytest.mark.parametrize("insert", [False, True])
def test_status_and_replies_in_every_combination(dev, insert):
    """With status and replies, with either alone and with neither; the caller's own status tensor; an empty
    batch."""
    B, vo, n, m = 24, 8, 40, 333
    held, tab, state = held_table(dev, 256, B, vo, "i64", "min", 2, n, 8200)
    pool = np.concatenate([held, distinct_mbits(20, 8201)])
    for t, (status, replies) in enumerate([(True, True), (False, True), (None, False), (True, False), (False, True)]):
        mb = pool[np.random.default_rng(8202 + t).integers(0, len(pool), m)]
        rows = rows_with(m, B, vo, operands("i64", "min", m, 2, 8203 + t), 8203)
        run_red(tab, state, mb, rows, "i64", "min", vo, 2, dev, insert=insert, status=status, replies=replies)
        check_table(tab, state, pool, dev)
    mine = torch.full((m,), 0xEE, dtype=torch.uint8, device=dev)
    rec = rec_to_dev(forge(mb, rows, 24 + B), dev)
    assert tab.reduce_records(rec, torch.int64, "max", vo, 2, insert=insert, status=mine).data_ptr() == mine.data_ptr()
    want, _ = R.reduce_ref(state, mb, rows, np.int64, "max", vo, 2, insert)
    assert (mine.cpu().numpy() == want).all()
    before = tab.counts()
    empty = tab.reduce_records(torch.empty((0, 24 + B), dtype=torch.uint8, device=dev), torch.int64, "min", vo, 2,
                               insert=insert, replies=True)
    assert empty[0].numel() == 0 and tuple(empty[1].shape) == (0, 8 + B) and tab.counts() == before


@pytest.mark.parametrize("insert", [False, True])
@pytest.mark.parametrize("B,pad,off,tag", [(16, 0, 0, 8), (16, 8, 0, 8), (24, 0, 0, 16), (24, 16, 16, 16), (24, 8, 0, 8),
                                           (24, 0, 8, 8), (8, 0, 0, 16), (8, 8, 8, 8), (40, 24, 0, 8), (1032, 0, 0, 16)])
def test_replies_between_guard_bytes(dev, insert, B, pad, off, tag):
    """Replies into a caller's buffer at strides of 8 + rowbytes and more: the reply bytes are the model's,
    every byte of the pad, before the first and behind the last reply keeps its pattern (run_red).  16-byte
    pieces when address, stride and 8 + rowbytes allow.  What the wrapper refuses."""
    assert reply_tag(B, off, 8 + B + pad) == tag
    keys = distinct_mbits(12, 8300)
    vo = B - 8
    tab, state = filled(dev, 64, B, keys[:6], rows_with(6, B, vo, operands("f64", "max", 6, 1, 8300), 8300))
    m = 131
    mb = keys[np.random.default_rng(8301).integers(0, 12, m)]
    rows = rows_with(m, B, vo, operands("f64", "max", m, 1, 8302), 8302)
    run_red(tab, state, mb, rows, "f64", "max", vo, 1, dev, insert=insert, pad=pad, off=off)
    check_table(tab, state, keys, dev)
    S = 8 + B + pad
    buf = torch.zeros(m * (S + 8) + 64, dtype=torch.uint8, device=dev)
    rec = rec_to_dev(forge(mb, rows, 24 + B), dev)
    for bad in (buf[4:4 + m * S].view(m, S)[:, :8 + B], buf[:m * (S + 4)].view(m, S + 4)[:, :8 + B],
                buf[:m * S].view(m, S)[:, :B], buf[:(m - 1) * S].view(m - 1, S)[:, :8 + B]):
        with pytest.raises(ValueError):
            tab.reduce_records(rec, torch.float64, "max", vo, replies=bad, insert=insert)


@pytest.mark.parametrize("fill", [0x00, 0xFF, "leftovers"])
def test_a_workspace_of_exactly_the_queried_size(dev, fill):
    """All three sizes -- flags 0 with replies (4*m), INSERT with and without replies -- whatever the workspace
    held: zeros, 0xFF, or what another call left in it.  One byte less is refused; flags 0 without replies
    takes an empty one."""
    B, vo, m = 16, 8, 4097
    keys = distinct_mbits(300, 8400)
    tab, state = filled(dev, 1024, B, keys[:150], rows_with(150, B, vo, operands("i64", "max", 150, 1, 8400), 8400))
    mb = keys[np.random.default_rng(8401).integers(0, 300, m)]
    for t, (insert, replies) in enumerate([(False, True), (True, False), (True, True)]):
        need = P.table_reduce_workspace_bytes(m, insert=insert, replies=replies)
        assert need == (4 * m + 4100 if insert else 4 * m)
        ws = torch.full((need,), 0 if fill == 0 else 0xFF, dtype=torch.uint8, device=dev)
        rows = rows_with(m, B, vo, operands("i64", "max", m, 1, 8402 + t), 8402)
        if fill == "leftovers":  # of a call on another table with other records
            other = P.DeviceTable(64, B, dev)
            other.reduce_records(rec_to_dev(forge(mb[::-1].copy(), rows, 24 + B), dev), torch.int64, "or", vo,
                                 insert=insert, replies=replies, workspace=ws)
        run_red(tab, state, mb, rows, "i64", "max", vo, 1, dev, insert=insert, replies=replies, workspace=ws)
        check_table(tab, state, keys, dev)
        with pytest.raises(ValueError):
            tab.reduce_records(rec_to_dev(forge(mb, rows, 24 + B), dev), torch.int64, "max", vo, insert=insert,
                               replies=replies, workspace=ws[:-1])
    assert P.table_reduce_workspace_bytes(m) == 0
    run_red(tab, state, mb, rows, "i64", "max", vo, 1, dev, replies=False,
            workspace=torch.empty(0, dtype=torch.uint8, device=dev))


# ================================================== streams and graphs ===
def test_reduce_on_a_side_stream(dev):
    B, vo, m = 16, 8, 700
    keys = distinct_mbits(80, 8500)
    tab, state = filled(dev, 256, B, keys[:40], rows_with(40, B, vo, operands("f64", "min", 40, 1, 8500), 8500))
    mb = keys[np.random.default_rng(8501).integers(0, 80, m)]
    rows = rows_with(m, B, vo, operands("f64", "min", m, 1, 8502), 8502)
    rec = rec_to_dev(forge(mb, rows, 40), dev)
    ws = torch.empty(P.table_reduce_workspace_bytes(m, insert=True, replies=True), dtype=torch.uint8, device=dev)
    st = torch.full((m,), 0xEE, dtype=torch.uint8, device=dev)
    rep = torch.full((m, 8 + B), 0xEE, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    tab.reduce_records(rec, torch.float64, "min", vo, insert=True, status=st, replies=rep, workspace=ws, stream=s)
    s.synchronize()
    want, want_rep = R.reduce_ref(state, mb, rows, np.float64, "min", vo, 1, True, capacity=256)
    assert (st.cpu().numpy() == want).all() and (rep.cpu().numpy() == want_rep).all()
    check_table(tab, state, keys, dev)


def test_reduce_get_reduce_in_a_graph(dev):
    """One captured graph of reduce(min, insert, replies) -> get -> reduce(or), replayed twice: every replay
    starts from the table the one before left, and the model is stepped along with it."""
    B, vo, m = 40, 8, 900
    keys = distinct_mbits(400, 8600)
    rng = np.random.default_rng(8601)
    batch = {x: keys[rng.integers(lo, hi, m)] for x, (lo, hi) in dict(a=(0, 250), c=(150, 400)).items()}
    rows = {"a": rows_with(m, B, vo, operands("i64", "min", m, 3, 8602), 8602),
            "c": rows_with(m, B, vo, operands("i64", "or", m, 3, 8603, special=0.05) & np.uint64(0x0101010101010101), 8603)}
    rec = {x: rec_to_dev(forge(batch[x], rows[x], 24 + B), dev) for x in "ac"}
    q = i64(keys, dev)
    tab, state = P.DeviceTable(1024, B, dev), {}
    ws = torch.empty(P.table_reduce_workspace_bytes(m, insert=True, replies=True), dtype=torch.uint8, device=dev)
    st = {x: torch.empty(m, dtype=torch.uint8, device=dev) for x in "ac"}
    rep = torch.empty((m, 8 + B), dtype=torch.uint8, device=dev)
    out = torch.empty((400, 8 + B), dtype=torch.uint8, device=dev)

    def step():
        tab.reduce_records(rec["a"], torch.int64, "min", vo, 3, insert=True, status=st["a"], replies=rep, workspace=ws)
        tab.get(q, out=out)
        tab.reduce_records(rec["c"], torch.int64, "or", vo, 3, status=st["c"], workspace=ws[:0])

    def model_step():
        want = {"a": R.reduce_ref(state, batch["a"], rows["a"], np.int64, "min", vo, 3, True, capacity=1024)}
        want["get"] = R.replies8(state, keys, B)
        want["c"] = R.reduce_ref(state, batch["c"], rows["c"], np.int64, "or", vo, 3, False)
        return want

    def compare(want):
        for x in "ac":
            assert (st[x].cpu().numpy() == want[x][0]).all()
        assert (rep.cpu().numpy() == want["a"][1]).all() and (out.cpu().numpy() == want["get"]).all()
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
        for t in list(st.values()) + [rep, out]:
            t.fill_(9)
        g.replay()
        torch.cuda.synchronize(dev)
        compare(model_step())
        assert tab.counts()[:3] == (len(state), 0, base[2] + k)
