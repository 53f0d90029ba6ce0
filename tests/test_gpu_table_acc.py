"""GPU checks of the table's accumulate (include/pdht_hip_table_acc.h): status, counters and the table
afterwards -- a get of every mbits plus absent ones -- byte for byte against the sequential model of
tests/table_acc_ref.py, which applies one record after the other and knows nothing of winner words, waves
or atomics.  Integer sums wrap and are exact; double sums are bit-exact where every partial sum is an
integer below 2^53, and otherwise checked per word against math.fsum with the header's any-order bound
gamma_n * sum|x_i| (gamma_n = n*u / (1 - n*u), u = 2^-53) and nothing looser.  Tables have 64 or 256 slots
except where a batch has to outgrow the grid."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

import table_acc_ref as A  # noqa: E402
from test_gpu_table import distinct_mbits, forge, rec_to_dev, rows_for, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = {"i32": (torch.int32, np.int32, np.uint32), "i64": (torch.int64, np.int64, np.uint64),
         "f64": (torch.float64, np.float64, np.float64)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------- helpers ---
def i64(mb, dev):
    return to_dev(np.asarray(mb, np.uint64).view(np.int64), dev)


def addends(kind, m, elems, seed, small=False):
    """[m, elems] of the kind's storage type.  Integers: the full range (sums wrap), or small ones.
    Doubles: integer-valued with mixed signs, |x| < 2^20, so that every partial sum of fewer than 2^32 of
    them is an integer below 2^53 and any order of the additions gives the same bits."""
    rng = np.random.default_rng(seed)
    if kind == "f64":
        return rng.integers(-(1 << 20), 1 << 20, (m, elems)).astype(np.float64)
    hi = 1000 if small else (1 << 32 if kind == "i32" else 1 << 64)
    return rng.integers(0, hi, (m, elems), dtype=np.uint64).astype(KINDS[kind][2])


def rows_with(m, B, vo, values, seed):
    """Noise rows whose region at vo holds values [m, elems]."""
    rows = rows_for(m, B, seed)
    v = np.ascontiguousarray(values)
    rows[:, vo:vo + v.shape[1] * v.itemsize] = v.view(np.uint8).reshape(m, -1)
    return rows


def filled(dev, capacity, B, mb, rows):
    """A table that holds rows[i] under mb[i] (distinct) after one put, and its state for the model."""
    tab = P.DeviceTable(capacity, B, dev)
    st = tab.put_records(rec_to_dev(forge(mb, rows, 24 + B), dev))
    assert int(st.count_nonzero()) == 0
    return tab, {int(k): rows[i].copy() for i, k in enumerate(mb)}


def replies8(state, q, B):
    out = np.zeros((len(q), 8 + B), np.uint8)
    for p, k in enumerate(np.asarray(q, np.uint64).tolist()):
        row = state.get(k)
        if row is not None:
            out[p, 0] = 1
            out[p, 8:] = row
    return out


def check_table(tab, state, q, dev):
    """The table holds exactly `state` as far as the requests q can tell."""
    got = tab.get(i64(q, dev)).cpu().numpy()
    assert (got == replies8(state, q, tab.rowbytes)).all()


def run_acc(tab, state, mb, rows, kind, vo, elems, dev, insert=False, stride=None, dropped_ok=False, **kw):
    """One accumulate batch on the device and on the model: last_kernel, status and counters compared.
    dropped_ok: the batch may overflow; the set of dropped mbits is then read from the device's status
    (which new mbits lose is the schedule's choice) and checked for consistency here.
    Returns (status, the model's per-word sums for doubles, the dropped mbits)."""
    tdt, ndt, _ = KINDS[kind]
    rec = rec_to_dev(forge(mb, rows, stride or 24 + tab.rowbytes), dev)
    before = tab.counts()
    had = {k for k in state}
    st = tab.acc_records(rec, tdt, vo, elems, insert=insert, **kw)
    assert P.last_kernel() == (f"k_table_acc_claim+k_table_acc<{kind},insert>" if insert else f"k_table_acc<{kind}>")
    got = st.cpu().numpy()
    mb = np.asarray(mb, np.uint64)
    lost = set(mb[got == 2].tolist())
    if lost:
        assert dropped_ok and insert
        assert not (lost & set(mb[got != 2].tolist()))  # all records of one mbits share one fate
        assert not (lost & had) and 0 not in lost        # present mbits and mbits 0 are never dropped
    want, sums = A.acc_ref(state, mb, rows, ndt, vo, elems, insert, dropped=lost, capacity=tab.capacity)
    assert (got == want).all()
    after = tab.counts()
    if not insert or len(mb) == 0:
        assert after == before  # no winner words, no batch number, nothing inserted, dropped or counted
    else:
        new = len(set(state) - had)
        assert after[:3] == (before[0] + new, before[1] + int((got == 2).sum()), before[2] + 1)
        assert after[3] - before[3] >= len(mb)  # every record inspects at least one slot
        assert after[0] == len(state)
    return got, sums, lost


# ===================================================== types x regions ===
REGIONS = ([("i32", 40, vo, e) for vo in (0, 4, 12) for e in (1, 2, 3, 5)] +
           [(k, 72, vo, e) for k in ("i64", "f64") for vo in (0, 8, 32) for e in (1, 2, 5)] +
           [("i64", 8, 0, 1), ("f64", 8, 0, 1), ("i32", 8, 4, 1), ("i64", 16, 8, 1), ("i32", 16, 4, 3),
            ("f64", 40, 0, 5), ("i64", 48, 8, 5), ("f64", 48, 16, 4), ("i32", 48, 12, 9),
            ("i64", 520, 0, 65), ("f64", 528, 8, 65), ("i32", 520, 4, 129), ("i64", 264, 0, 33)])


@pytest.mark.parametrize("kind,B,vo,elems", REGIONS)
def test_types_and_regions(dev, kind, B, vo, elems):
    """Every type at every alignment of its region, rows of 8 .. 528 bytes, groups of 1 .. 64 lanes and a
    region of more elements than a wave has lanes; a record stride with noise behind the row; noise in every
    row byte outside the region, which survives on present entries; repeats and absent mbits in the batch.
    Then the same batch once more with INSERT, which creates the absent ones."""
    C, n, m = 256, 100, 600
    seed = 1000 + B * 7 + vo * 3 + elems
    held, absent = distinct_mbits(n, seed), distinct_mbits(30, seed + 1)
    tab, state = filled(dev, C, B, held, rows_with(n, B, vo, addends(kind, n, elems, seed), seed))
    pool = np.concatenate([held, absent])
    mb = pool[np.random.default_rng(seed).integers(0, len(pool), m)]
    rows = rows_with(m, B, vo, addends(kind, m, elems, seed + 2), seed + 2)
    outside = {k: np.delete(v, np.s_[vo:vo + elems * KINDS[kind][2]().itemsize]) for k, v in state.items()}
    st, _, _ = run_acc(tab, state, mb, rows, kind, vo, elems, dev, stride=24 + B + (16 if elems % 2 else 0))
    assert (st == np.where(np.isin(mb, held), 0, 3)).all() and set(state) == set(outside)
    for k, v in state.items():  # the model itself left the bytes outside the region alone
        assert (np.delete(v, np.s_[vo:vo + elems * KINDS[kind][2]().itemsize]) == outside[k]).all()
    check_table(tab, state, pool, dev)
    st, _, _ = run_acc(tab, state, mb, rows, kind, vo, elems, dev, insert=True, stride=24 + B + 8)
    assert (st == 0).all() and len(state) == n + len(np.unique(mb[np.isin(mb, absent)]))
    check_table(tab, state, pool, dev)


# ======================================================== batch shapes ===
def batch_shapes(h, absent):
    """h: present mbits, h[0] == 0 (the private slot); absent: mbits the table does not hold."""
    last2 = np.concatenate([h[1:64], h[63:64]])  # 64 records, the only repeat in lanes 62 and 63
    return {
        "m1": h[1:2], "m63": h[1:64], "m64": h[1:65], "m65": h[1:66],
        "one_mbits": np.full(333, h[7]),
        "two_alternating": np.tile(h[[3, 4]], 150),
        "three_per_wave": np.tile(h[[3, 4, 5]], 64),
        "five_per_wave": np.tile(h[[3, 4, 5, 6, 7]], 50)[:-3],
        "last_two_lanes": np.concatenate([last2, last2, h[1:10]]),
        "mbits_zero": np.concatenate([np.zeros(70, np.uint64), h[1:3], np.zeros(3, np.uint64), h[1:2]]),
        "absent_mixed": np.concatenate([np.stack([np.tile(h[[9, 10]], 60), np.tile(absent[:3], 40)], 1).ravel(),
                                        np.full(70, absent[5]), h[9:12]]),
    }


SHAPES = sorted(batch_shapes(np.arange(100, dtype=np.uint64), np.arange(100, 110, dtype=np.uint64)))


@pytest.mark.parametrize("kind,B,vo,elems", [("i64", 16, 8, 1), ("i32", 24, 4, 3), ("f64", 24, 8, 2), ("i32", 8, 4, 1)])
@pytest.mark.parametrize("shape", SHAPES)
def test_batch_shapes(dev, shape, kind, B, vo, elems):
    """The shapes that exercise the in-wave sums: lanes (groups of 1, 2 or 4 lanes) that share a slot add up
    first, two leaders per wave, the lanes left over post on their own.  Present-only, then INSERT on an
    empty table (every mbits of the batch is new, and created from its first record)."""
    n = 80
    held = np.concatenate([np.zeros(1, np.uint64), distinct_mbits(n - 1, 2000)])
    absent = distinct_mbits(10, 2001)
    mb = batch_shapes(held, absent)[shape]
    m, seed = len(mb), 2002 + len(shape)
    tab, state = filled(dev, 256, B, held, rows_with(n, B, vo, addends(kind, n, elems, seed), seed))
    rows = rows_with(m, B, vo, addends(kind, m, elems, seed + 1), seed + 1)
    st, _, _ = run_acc(tab, state, mb, rows, kind, vo, elems, dev)
    assert (st == np.where(np.isin(mb, held), 0, 3)).all()
    check_table(tab, state, np.concatenate([held, absent]), dev)
    fresh, state = P.DeviceTable(256, B, dev), {}
    st, _, _ = run_acc(fresh, state, mb, rows, kind, vo, elems, dev, insert=True)
    assert (st == 0).all() and set(state) == set(np.unique(mb).tolist())
    first = {int(k): rows[i] for i, k in reversed(list(enumerate(mb)))}
    region = np.s_[vo:vo + elems * KINDS[kind][2]().itemsize]
    for k, v in state.items():  # everything outside the region is the FIRST record's
        assert (np.delete(v, region) == np.delete(first[k], region)).all()
    check_table(fresh, state, np.concatenate([held, absent]), dev)
    mbits, erows, _ = fresh.entries()
    assert sorted(mbits.cpu().numpy().view(np.uint64).tolist()) == sorted(state)
    for k, r in zip(mbits.cpu().numpy().view(np.uint64).tolist(), erows.cpu().numpy()):
        assert (r == state[k]).all()


@pytest.mark.parametrize("kind,B,vo,elems,insert", [("i64", 264, 0, 33, False), ("i64", 8, 0, 1, True)])
def test_second_round_of_the_grid(dev, kind, B, vo, elems, insert):
    """A batch past the reach of the launch, so that the loops run a second round, the last one with part of
    a wave past the end.  table_grid caps a grid at 8 workgroups per CU of 4 waves: k_table_acc covers
    64 / G records per wave and round (G = 64 lanes for 33 elements: one record), k_table_acc_claim one
    record per lane."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    m = cus * 8 * 4 * (64 if elems == 1 else 1) + 4097 + 130
    assert m % 64 != 0
    n = 200
    held, extra = distinct_mbits(n, 2100), distinct_mbits(56, 2101)
    tab, state = filled(dev, 256, B, held, rows_with(n, B, vo, addends(kind, n, elems, 2100), 2100))
    pool = np.concatenate([held, extra, np.zeros(1, np.uint64)])
    rng = np.random.default_rng(2102)
    mb = pool[rng.integers(0, len(pool), m)]
    mb[rng.random(m) < 0.3] = held[17]  # and a hot one
    rows = rows_with(m, B, vo, addends(kind, m, elems, 2103), 2103)
    st, _, _ = run_acc(tab, state, mb, rows, kind, vo, elems, dev, insert=insert)
    assert set(np.unique(st)) == ({0} if insert else {0, 3})
    check_table(tab, state, pool, dev)


# ========================================================= wrap-around ===
@pytest.mark.parametrize("kind", ["i32", "i64"])
@pytest.mark.parametrize("spread", [False, True])
def test_integer_sums_wrap(dev, kind, spread):
    """Entries at 2^31 - 3 / 2^63 - 3 and just under 2^32 / 2^64, addends up to half the range: the sums pass
    the sign bit and the word's end, one mbits per wave or spread over the waves; the same on every run."""
    bits = 32 if kind == "i32" else 64
    udt = KINDS[kind][2]
    B, vo, elems, n, m = 24, 8, 2, 8, 512
    held = distinct_mbits(n, 2200)
    start = np.array([[(1 << (bits - 1)) - 3, (1 << bits) - 2]] * n, dtype=udt)
    rng = np.random.default_rng(2201 + bits)
    add = rng.integers(1, 1 << (bits - 1), (m, elems), dtype=np.uint64).astype(udt)
    add[::5] = 1
    mb = np.repeat(held, 64) if not spread else held[rng.integers(0, n, m)]
    true = {int(k): [int(start[0, j]) + sum(int(x) for x in add[mb == k, j]) for j in range(elems)] for k in held}
    assert all(v[0] >= 1 << bits and v[1] >= 1 << (bits + 1) for v in true.values())  # they do wrap
    rows = rows_with(m, B, vo, add, 2202)
    tables = []
    for _ in range(2):
        tab, state = filled(dev, 64, B, held, rows_with(n, B, vo, start, 2203))
        run_acc(tab, state, mb, rows, kind, vo, elems, dev)
        for k in held:
            assert state[int(k)][vo:vo + elems * bits // 8].view(udt).tolist() == [x % (1 << bits) for x in true[int(k)]]
        check_table(tab, state, held, dev)
        tables.append(tab.get(i64(held, dev)).cpu().numpy())
    assert (tables[0] == tables[1]).all()


# ============================================================= doubles ===
def test_integer_valued_doubles_are_bit_exact(dev):
    """Every partial sum, in any order, is an integer below 2^53: no addition rounds, so the table equals the
    position-order model bit for bit (run_acc compares nothing else), hot mbits included."""
    B, vo, elems, n, m = 40, 8, 3, 20, 3000
    held = distinct_mbits(n, 2300)
    tab, state = filled(dev, 64, B, held, rows_with(n, B, vo, addends("f64", n, elems, 2300), 2300))
    rng = np.random.default_rng(2301)
    mb = held[rng.integers(0, n, m)]
    mb[rng.random(m) < 0.5] = held[3]
    big = rng.integers(-(1 << 40), 1 << 40, (m, elems)).astype(np.float64)  # 3000 * 2^40 < 2^53
    _, sums, _ = run_acc(tab, state, mb, rows_with(m, B, vo, big, 2302), "f64", vo, elems, dev)
    assert all(s["seq"] == s["exact"] for s in sums.values())
    check_table(tab, state, held, dev)


def test_the_sign_of_a_double_zero(dev):
    """Words holding -0.0 and records that all add -0.0, several per wave: a present entry keeps -0.0, as any
    sequential order would (the lanes without an addend feed the in-wave sums -0.0, not +0.0); +0.0 among the
    addends makes it +0.0.  An entry the call creates starts from +0.0 (the header says so)."""
    B, vo, elems, n = 24, 8, 2, 6
    held = distinct_mbits(n, 2350)
    neg = np.full((n, elems), -0.0)
    tab, state = filled(dev, 64, B, held, rows_with(n, B, vo, neg, 2350))
    mb = np.concatenate([np.tile(held[:3], 40), held[3:5], np.full(70, held[5])])
    add = np.full((len(mb), elems), -0.0)
    add[mb == held[1], 1] = 0.0  # one word of one entry meets +0.0
    run_acc(tab, state, mb, rows_with(len(mb), B, vo, add, 2351), "f64", vo, elems, dev)
    check_table(tab, state, held, dev)  # byte for byte: the model's -0.0 + -0.0 = -0.0
    signs = {int(k): np.signbit(state[int(k)][vo:vo + 16].view(np.float64)).tolist() for k in held}
    assert signs[int(held[0])] == [True, True] and signs[int(held[1])] == [True, False]
    fresh = P.DeviceTable(64, B, dev)
    fresh.acc_records(rec_to_dev(forge(mb, rows_with(len(mb), B, vo, add, 2351), 24 + B), dev), torch.float64, vo, elems,
                      insert=True)
    got = fresh.get(i64(held[:5], dev)).cpu().numpy()
    words = np.ascontiguousarray(got[:, 8 + vo:8 + vo + 16]).view(np.float64)
    assert (got[:, 0] == 1).all() and (words == 0).all() and not np.signbit(words).any()


@pytest.mark.parametrize("kind,B,vo,elems", [("i64", 16, 8, 1), ("i32", 24, 4, 3), ("f64", 24, 8, 2)])
def test_variant_without_the_in_wave_sums(dev, kind, B, vo, elems):
    """Tuning variant 344: every addend an atomic of its own, for the integer types; doubles keep the
    product's kernel under it.  Hot and mixed batches, present-only and INSERT, against the same model."""
    n = 60
    held, new = distinct_mbits(n, 2360), distinct_mbits(20, 2361)
    tab, state = filled(dev, 256, B, held, rows_with(n, B, vo, addends(kind, n, elems, 2360), 2360))
    rng = np.random.default_rng(2362)
    pool = np.concatenate([held, new])
    mb = pool[rng.integers(0, len(pool), 900)]
    mb[rng.random(900) < 0.5] = held[9]
    rows = rows_with(900, B, vo, addends(kind, 900, elems, 2363), 2363)
    with P.tuning(344):
        run_acc(tab, state, mb, rows, kind, vo, elems, dev)
        check_table(tab, state, pool, dev)
        run_acc(tab, state, mb, rows, kind, vo, elems, dev, insert=True)
        check_table(tab, state, pool, dev)
    run_acc(tab, state, mb, rows, kind, vo, elems, dev)  # and the product on the same table
    check_table(tab, state, pool, dev)


@pytest.mark.parametrize("insert", [False, True])
def test_mixed_magnitude_doubles_within_the_any_order_bound(dev, insert):
    """1 000 records on 3 mbits, magnitudes 1e-8 .. 1e8 with mixed signs: the order of the additions is the
    schedule's, so each word is held to |got - fsum| <= gamma_n * sum|x_i| (n addends, the old value among
    them) and every other byte of the table to the model exactly."""
    B, vo, elems, m = 32, 8, 2, 1000
    held = distinct_mbits(3, 2400)
    rng = np.random.default_rng(2401)

    def mixed(k):
        return (10.0 ** rng.uniform(-8, 8, (k, elems))) * rng.choice([-1.0, 1.0], (k, elems))

    if insert:
        tab, state = P.DeviceTable(64, B, dev), {}
    else:
        tab, state = filled(dev, 64, B, held, rows_with(3, B, vo, mixed(3), 2402))
    mb = held[rng.integers(0, 3, m)]
    rows = rows_with(m, B, vo, mixed(m), 2403)
    _, sums, _ = run_acc(tab, state, mb, rows, "f64", vo, elems, dev, insert=insert)
    assert len(sums) == 3 * elems and sum(s["n"] for s in sums.values()) == elems * (m + (0 if insert else 3))
    got = tab.get(i64(held, dev)).cpu().numpy()
    want = replies8(state, held, B)
    region = np.s_[8 + vo:8 + vo + 8 * elems]
    assert (np.delete(got, region, axis=1) == np.delete(want, region, axis=1)).all()
    words = np.ascontiguousarray(got[:, region]).view(np.float64)
    for i, k in enumerate(held.tolist()):
        for j in range(elems):
            s = sums[(k, j)]
            bound = A.gamma(s["n"]) * s["abs"]
            err = abs(float(words[i, j]) - s["exact"])
            print(f"mbits {i} word {j}: n {s['n']}, |got - fsum| {err:.3e}, bound {bound:.3e}, "
                  f"|seq - fsum| {abs(s['seq'] - s['exact']):.3e}")
            assert err <= bound


# ============================================================== INSERT ===
def test_insert_creates_from_the_first_record(dev):
    """New mbits whose records carry different key-slot bytes, present and new ones side by side in one wave,
    mbits 0 created: the first record's bytes stay, the region is the sum of all."""
    B, vo, elems, n = 32, 16, 2, 30  # bytes 0..15 the "key slot", 16..31 two counters
    held = distinct_mbits(n, 2500)
    tab, state = filled(dev, 256, B, held, rows_with(n, B, vo, addends("i64", n, elems, 2500), 2500))
    new = np.concatenate([distinct_mbits(40, 2501), np.zeros(1, np.uint64)])
    mb = np.stack([np.tile(held[:8], 16), np.tile(new[:8], 16)], 1).ravel()  # present, new, present, new ...
    mb = np.concatenate([mb, new, new[::-1], held, np.zeros(5, np.uint64)])
    rows = rows_with(len(mb), B, vo, addends("i64", len(mb), elems, 2502), 2502)
    first = np.unique(mb, return_index=True)[1]
    st, _, _ = run_acc(tab, state, mb, rows, "i64", vo, elems, dev, insert=True)
    assert (st == 0).all() and len(state) == n + 41
    for p in first:
        k = int(mb[p])
        if k not in set(held.tolist()):
            assert (state[k][:vo] == rows[p][:vo]).all()
            assert len({rows[q][:vo].tobytes() for q in np.flatnonzero(mb == mb[p])}) > 1  # the others differ
    check_table(tab, state, np.concatenate([held, new, distinct_mbits(5, 2503)]), dev)
    assert sorted(tab.entries()[0].cpu().numpy().view(np.uint64).tolist()) == sorted(state)


def test_insert_counts_as_a_put_does(dev):
    """Twin tables, one fed by put_records and one by acc_records(insert=True) with the same records, every
    mbits twice: entries, dropped and batches agree after each batch, and so do the slots inspected by the
    second batch, when every mbits is present and no race can change the number (each mbits equally often,
    so that the sum over a cluster does not depend on who sits where in it)."""
    B, n = 16, 150
    keys = np.concatenate([distinct_mbits(n, 2600), np.zeros(1, np.uint64)])
    mb = np.tile(keys, 2)[np.random.default_rng(2601).permutation(2 * (n + 1))]
    rows = rows_with(len(mb), B, 8, addends("i64", len(mb), 1, 2602), 2602)
    rec = rec_to_dev(forge(mb, rows, 24 + B), dev)
    a, b = P.DeviceTable(256, B, dev), P.DeviceTable(256, B, dev)
    seen = []
    for rnd in (1, 2):
        a.acc_records(rec, torch.int64, 8, insert=True)
        b.put_records(rec)
        ca, cb = a.counts(), b.counts()
        assert ca[:3] == cb[:3] == (n + 1, 0, rnd)
        seen.append((ca[3], cb[3]))
    assert seen[1][0] - seen[0][0] == seen[1][1] - seen[0][1] >= len(mb)


@pytest.mark.parametrize("kind,B,vo,elems", [("i64", 8, 0, 1), ("i32", 40, 12, 3), ("f64", 48, 8, 5)])
def test_insert_overflow_part_way(dev, kind, B, vo, elems):
    """More new mbits than free slots on a 64-slot table, each with many records, twice over: inserted =
    min(new, free); present mbits and their sums are never dropped; all records of an mbits share their
    fate (run_acc checks both); and the model, fed with the set the device dropped, matches everything
    else -- status, counters and every row."""
    C = 64
    rng = np.random.default_rng(2700 + B)
    old = distinct_mbits(40, 2700)
    tab, state = filled(dev, C, B, old, rows_with(40, B, vo, addends(kind, 40, elems, 2700), 2700))
    new = np.concatenate([distinct_mbits(100, 2701), np.array([1], np.uint64)])  # mbits 1 competes like any key
    pool = np.concatenate([old, new, np.zeros(1, np.uint64)])
    mb = np.concatenate([np.repeat(pool, 10), pool[rng.integers(0, len(pool), 4097 - 10 * len(pool))]])
    mb = mb[rng.permutation(len(mb))]
    winners = None
    for rnd in (0, 1):  # the same mbits again with new addends: tags are final
        rows = rows_with(len(mb), B, vo, addends(kind, len(mb), elems, 2710 + rnd), 2710 + rnd)
        before = tab.counts()
        st, _, lost = run_acc(tab, state, mb, rows, kind, vo, elems, dev, insert=True, dropped_ok=True)
        won = set(state) - set(old.tolist()) - {0}
        assert won <= set(new.tolist()) and len(won) == C - 40 and len(lost) == 101 - (C - 40)
        if rnd == 0:
            winners = won
        assert won == winners and lost == set(new.tolist()) - winners
        assert tab.counts()[0] == C + 1 and \
            tab.counts()[1] - before[1] == int(np.isin(mb, np.array(sorted(lost), np.uint64)).sum())
        check_table(tab, state, np.concatenate([pool, distinct_mbits(5, 2702)]), dev)


# ========================================================= repeat calls ===
def test_three_batches_and_puts_between_them(dev):
    """flags 0, a put, INSERT, a put, flags 0 on one table, all over the same mbits: winner words and batch
    numbers of earlier calls decide nothing later (a put's last writer and the accumulate's first record
    stand at unrelated positions of batches of different lengths)."""
    B, vo, elems, C = 24, 8, 2, 256
    pool = np.concatenate([np.zeros(1, np.uint64), distinct_mbits(90, 2800)])
    rng = np.random.default_rng(2801)
    tab, state = filled(dev, C, B, pool[:40], rows_with(40, B, vo, addends("i64", 40, elems, 2800), 2800))
    batches = 1
    for t, what in enumerate(["acc", "put", "ins", "put", "acc", "ins", "acc"]):
        m = int(rng.integers(150, 500))
        mb = pool[rng.integers(0, 60 if what == "put" else len(pool), m)]
        rows = rows_with(m, B, vo, addends("i64", m, elems, 2810 + t), 2810 + t)
        if what == "put":
            st = tab.put_records(rec_to_dev(forge(mb, rows, 24 + B), dev)).cpu().numpy()
            last = m - 1 - np.unique(mb[::-1], return_index=True)[1]
            want = np.ones(m, np.uint8)
            want[last] = 0
            assert (st == want).all()
            for p in last:
                state[int(mb[p])] = rows[p].copy()
        else:
            run_acc(tab, state, mb, rows, "i64", vo, elems, dev, insert=what == "ins")
        batches += what != "acc"
        assert tab.counts()[:3] == (len(state), 0, batches)
        check_table(tab, state, pool, dev)


def test_acc_on_a_side_stream_with_a_caller_workspace(dev):
    """The caller's status and workspace of exactly the queried size, whatever they held, on a side stream."""
    B, vo, n, m = 16, 8, 50, 700
    held, new = distinct_mbits(n, 2900), distinct_mbits(30, 2901)
    pool = np.concatenate([held, new])
    mb = pool[np.random.default_rng(2902).integers(0, len(pool), m)]
    rows = rows_with(m, B, vo, addends("i64", m, 1, 2903), 2903)
    need = P.table_acc_workspace_bytes(m, insert=True)
    assert need == 4 * m + m and P.table_acc_workspace_bytes(m) == 0
    results = []
    for fill in (0x00, 0xFF):
        tab, state = filled(dev, 256, B, held, rows_with(n, B, vo, addends("i64", n, 1, 2900), 2900))
        ws = torch.full((need,), fill, dtype=torch.uint8, device=dev)
        st0 = torch.full((m,), 0xEE, dtype=torch.uint8, device=dev)
        status = torch.full((m,), 0xEE, dtype=torch.uint8, device=dev)
        s = torch.cuda.Stream(device=dev)
        rec = rec_to_dev(forge(mb, rows, 24 + B), dev)
        torch.cuda.synchronize(dev)
        assert tab.acc_records(rec, torch.int64, vo, status=st0, stream=s).data_ptr() == st0.data_ptr()
        tab.acc_records(rec, torch.int64, vo, insert=True, status=status, workspace=ws, stream=s)
        s.synchronize()
        w0, _ = A.acc_ref(state, mb, rows, np.int64, vo, 1, False)
        w1, _ = A.acc_ref(state, mb, rows, np.int64, vo, 1, True)
        assert (st0.cpu().numpy() == w0).all() and (status.cpu().numpy() == w1).all()
        check_table(tab, state, pool, dev)
        results.append(tab.get(i64(pool, dev)).cpu().numpy())
        with pytest.raises(ValueError):
            tab.acc_records(rec, torch.int64, vo, insert=True, workspace=ws[:-4])
    assert (results[0] == results[1]).all()


# ===================================================== IEEE specials ===
# NaN, infinities, sums that overflow and subnormals in the double accumulate.  The position-order model cannot
# say what these give (math.fsum raises on inf - inf and on overflow), so the expectation is computed here from
# rules that hold in ANY order of the additions -- tests/test_table_ranges_cpu.py checks special_expect against
# exact arithmetic on every input set below, in random sequential and tree orders.
SPECIAL_RULES = ("nan", "pinf", "ninf", "both", "overflow", "sub", "sub_zero", "sub_cross")
SPECIAL_REGIONS = ((24, 8, 2), (272, 8, 33), (48, 8, 5))  # (B, vo, elems): groups of 2 lanes; one record per
#                                                            wave, pure atomics; 5 elements in a 48-B row at +8
SPECIAL_SHAPES = ("m65", "one_mbits", "three_per_wave", "five_per_wave", "absent_mixed")
DBL_OVER = 1 << 1024  # anything that rounds to here or beyond is +inf (the threshold is 2^1024 - 2^970)


def _unit_exponent(x):
    """e with x = odd * 2^e (x finite, non-zero)."""
    num, den = abs(x).as_integer_ratio()
    return (num & -num).bit_length() - 1 - (den.bit_length() - 1)


def special_expect(xs):
    """What a word holds after xs[0] + xs[1] + ... added in ANY order or tree (xs[0]: the old value, +0.0 for an
    entry the call creates), or ValueError when no rule decides it:
      a NaN among them -> NaN (the payload is not specified);
      +inf and -inf -> NaN; only +inf -> +inf; only -inf -> -inf;
      finite, all multiples of one power of two 2^e with sum|x_i| < 2^53 * 2^e: every partial sum is such a
        multiple below 2^53 of them, so no addition rounds and the result is the exact sum (integers below
        2^53, multiples of 2^-1074 whether subnormal or just normal, a single non-zero value); a zero result is
        +0.0 (no -0.0 may be among the xs: a zero sum then comes from a cancellation or from +0.0 + +0.0);
      finite and all of one sign with |exact sum| * (1 - gamma_n) >= 2^1024: had no partial sum overflowed, the
        result would be within gamma_n of the exact sum and so past DBL_MAX; one did, and sums of one sign never
        come back from an infinity."""
    import math
    from fractions import Fraction
    xs = [float(x) for x in xs]
    if any(math.isnan(x) for x in xs):
        return math.nan
    pos, neg = math.inf in xs, -math.inf in xs
    if pos or neg:
        return math.nan if pos and neg else math.inf if pos else -math.inf
    if any(x == 0 and math.copysign(1.0, x) < 0 for x in xs):
        raise ValueError("-0.0 among the addends: the sign of a zero sum depends on the order")
    nz = [x for x in xs if x != 0]
    if not nz:
        return 0.0
    e = min(_unit_exponent(x) for x in nz)
    exact = sum(Fraction(x) for x in nz)
    total = sum(abs(Fraction(x)) for x in nz)
    if total < Fraction(2) ** (53 + e) and total < DBL_OVER:
        return float(exact)  # representable: an integer below 2^53 times 2^e, e >= -1074, below 2^1024
    n = len(xs)
    one_sign = all(x > 0 for x in nz) or all(x < 0 for x in nz)
    if one_sign and abs(exact) * (1 - Fraction(n, (1 << 53) - n)) >= DBL_OVER:
        return math.inf if exact > 0 else -math.inf
    raise ValueError("no order-independent rule for these addends")


def special_word(rule, r, has_old, rng, ki):
    """(old value or None, r addends) of one word under `rule`; "ordinary": integer-valued, |x| < 2^20."""
    import math
    add = [float(x) for x in rng.integers(-(1 << 20), 1 << 20, r)]
    old = float(rng.integers(-(1 << 20), 1 << 20)) if has_old else None
    if rule in ("nan", "pinf", "ninf"):
        v = {"nan": math.nan, "pinf": math.inf, "ninf": -math.inf}[rule]
        if has_old and ki % 3 == 2:
            old = v  # the entry holds it, the records are ordinary
        else:
            add[int(rng.integers(0, r)) if has_old else 0] = v  # a created entry: its first record carries it
    elif rule == "both":
        if has_old:
            old, add[int(rng.integers(0, r))] = math.inf, -math.inf
        else:
            add[0] = math.inf
            if r >= 2:
                add[r - 1] = -math.inf
    elif rule == "overflow":
        add = [1e308] * r
        old = 1e308 if has_old else None
    elif rule in ("sub", "sub_zero", "sub_cross"):
        if rule == "sub_cross":  # the sum ends at or above 2^52 units = 2^-1022, the smallest normal
            k = [(1 << 52) // r + int(x) for x in rng.integers(-1000, 1000, r)]
            k0 = 2000 * r + 7
            if not has_old:
                k[r - 1] += k0
            assert sum(k) + (k0 if has_old else 0) >= 1 << 52
        else:
            k = [int(x) * int(s) for x, s in zip(rng.integers(1, 1 << 20, r), rng.choice([-1, 1], r))]
            k0 = int(rng.integers(1, 1 << 20))
            if rule == "sub_zero":  # ends exactly 0 after being non-zero
                if has_old:
                    if sum(k) == 0:
                        k[0] += 1
                    k0 = -sum(k)
                elif r >= 2:
                    if sum(k[:-1]) == 0:
                        k[0] += 1
                    k[r - 1] = -sum(k[:-1])
        add = [math.ldexp(x, -1074) for x in k]
        old = math.ldexp(k0, -1074) if has_old else None
    else:
        assert rule == "ordinary"
    return old, add


def special_batch(rule, shape, elems, insert, seed=0):
    """The inputs of one special-values batch, made without a GPU: (held, old [n, elems], absent, mb, add [m,
    elems], rule_of) -- a table of the 80 mbits `held` (mbits 0 among them) whose words hold `old`, a batch of
    the shape `shape` of batch_shapes over them, and the rule of every word (mbits, element) the batch adds
    into: `rule` where (index of the mbits by first appearance + element) is even, "ordinary" elsewhere.
    insert: the batch goes to an EMPTY table with insert=True, so every word starts from +0.0."""
    held = np.concatenate([np.zeros(1, np.uint64), distinct_mbits(79, 2950)])
    absent = distinct_mbits(10, 2951)
    mb = batch_shapes(held, absent)[shape]
    rng = np.random.default_rng(2952 + seed + 7 * SPECIAL_RULES.index(rule) + 101 * SPECIAL_SHAPES.index(shape) + elems)
    old = rng.integers(-(1 << 20), 1 << 20, (len(held), elems)).astype(np.float64)
    add = np.zeros((len(mb), elems))
    row_of = {int(k): i for i, k in enumerate(held)}
    rule_of = {}
    order = []
    for k in mb.tolist():
        if k not in order:
            order.append(k)
    for ki, k in enumerate(order):
        at = np.flatnonzero(mb == np.uint64(k))
        present = not insert and k in row_of
        for j in range(elems):
            what = rule if (ki + j) % 2 == 0 else "ordinary"
            o, a = special_word(what, len(at), present, rng, ki)
            add[at, j] = a
            if present:
                old[row_of[k], j] = o
            if present or insert:
                rule_of[(k, j)] = what
    return held, old, absent, mb, add, rule_of


def special_words(held, old, mb, add, insert):
    """{(mbits, element): [old value or +0.0, the addends in position order]} of every word the batch adds into."""
    row_of = {} if insert else {int(k): i for i, k in enumerate(held)}
    words = {}
    for p, k in enumerate(mb.tolist()):
        if not insert and k not in row_of:
            continue
        for j in range(add.shape[1]):
            words.setdefault((k, j), [0.0 if insert else float(old[row_of[k], j])]).append(float(add[p, j]))
    return words


@pytest.mark.parametrize("B,vo,elems", SPECIAL_REGIONS)
@pytest.mark.parametrize("rule", SPECIAL_RULES)
def test_special_doubles_follow_ieee_in_any_order(dev, rule, B, vo, elems):
    """NaN, +-inf, inf - inf, sums that overflow and subnormals (exact multiples of 2^-1074: sums that end 0, and
    sums that cross into the normals at 2^-1022), in every other word of a batch; the words between them take
    integer-valued addends.  Distinct mbits (one atomic per record), one hot mbits and three and five mbits per
    wave (in-wave sums, then one atomic), mixed with absent ones; 33 elements (one record per wave, pure
    atomics, no in-wave sum) and 5 elements in a 48-B row at +8; present entries, and insert=True on an empty
    table, where the first record carries the special value and the word starts from +0.0.  Each word against
    special_expect (NaN by isnan, everything else bit for bit); the ordinary words also against the
    position-order sum; every byte outside the region, the status and the counters against the model."""
    import math
    region = np.s_[8 + vo:8 + vo + 8 * elems]
    for shape in SPECIAL_SHAPES:
        for insert in (False, True):
            held, old, absent, mb, add, rule_of = special_batch(rule, shape, elems, insert)
            m = len(mb)
            rows = rows_with(m, B, vo, add, 2960)
            if insert:
                tab, state = P.DeviceTable(256, B, dev), {}
                first = {int(k): rows[i] for i, k in reversed(list(enumerate(mb)))}
                state = {k: r.copy() for k, r in first.items()}  # outside the region: the FIRST record's bytes
                want_st = np.zeros(m, np.uint8)
            else:
                tab, state = filled(dev, 256, B, held, rows_with(len(held), B, vo, old, 2961))
                want_st = np.where(np.isin(mb, held), 0, 3).astype(np.uint8)
            before = tab.counts()
            st = tab.acc_records(rec_to_dev(forge(mb, rows, 24 + B), dev), torch.float64, vo, elems, insert=insert)
            assert P.last_kernel() == ("k_table_acc_claim+k_table_acc<f64,insert>" if insert else "k_table_acc<f64>")
            assert (st.cpu().numpy() == want_st).all()
            after = tab.counts()
            if insert:
                assert after[:3] == (len(state), 0, 1) and after[3] >= m
            else:
                assert after == before
            q = np.concatenate([held, absent])
            got = tab.get(i64(q, dev)).cpu().numpy()
            want = replies8(state, q, B)
            assert (np.delete(got, region, axis=1) == np.delete(want, region, axis=1)).all()
            gotw = np.ascontiguousarray(got[:, region]).view(np.float64)
            words = special_words(held, old, mb, add, insert)
            assert set(words) == set(rule_of) and rule in rule_of.values() and "ordinary" in rule_of.values()
            at = {int(k): i for i, k in enumerate(q)}
            for i, k in enumerate(q.tolist()):  # the words no record named keep what they held
                for j in range(elems):
                    if (k, j) not in words and k in state:
                        assert gotw[i, j].tobytes() == np.float64(old[i, j]).tobytes()
            bad = []
            for (k, j), xs in words.items():
                g, w = float(gotw[at[k], j]), special_expect(xs)
                if rule_of[(k, j)] == "ordinary":
                    seq = np.float64(xs[0])
                    for x in xs[1:]:
                        seq = seq + np.float64(x)
                    assert float(seq) == w and not math.isnan(w)  # the integer-valued-doubles rule
                same = math.isnan(g) if math.isnan(w) else np.float64(g).tobytes() == np.float64(w).tobytes()
                if not same:
                    bad.append((shape, insert, rule_of[(k, j)], len(xs) - 1, g.hex(), w.hex()))
            assert not bad, bad[:8]
