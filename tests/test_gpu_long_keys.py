"""GPU parity of the long-key and strided hash paths, swept over every length.

Once a 64-key tile of fixed rows no longer fits an LDS window
(63 * stride + L + 16 > 16384) each lane reads its own key from global memory
through GlobalReaderT (k_global), in 16-B loads with whole-line spans when
every row starts 16-B aligned, else in dword runs with a funnel shift; keys
of a variable-length batch that end past the wave's window take the same
reader, the others LdsReader.  These are integer kernels: a wrong branch of a
reader is wrong for one residue class of lengths or alignments and nothing
else, so the tests below walk every length, at the layouts that select each
reader, bit-exact against the oracle, and assert the kernel tag of every call.

Every fixed-key case is a view into one random device buffer (the same bytes
on the host); no case uploads keys of its own.
"""
import numpy as np
import pytest

from hash_ref import VAR_WINDOW_KERNELS, fixed_kernel, var_from_lds, var_kernel

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

pytestmark = pytest.mark.gpu

S0, S1 = 0x0123456789ABCDEF, 0xFEDCBA9876543210
K2 = 0x9AE16A3B2F90404F  # CityHash64 of the empty key


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def buf(dev):
    """(host bytes, the same bytes on the device); the device base is 16-B aligned."""
    host = np.random.default_rng(0xC17).integers(0, 256, 1 << 20, dtype=np.uint8)
    d = torch.from_numpy(host).to(dev)
    assert d.data_ptr() % 16 == 0
    return host, d


def rows(buf, base, n, S, L):
    """n rows of L bytes at stride S from byte `base` of the buffer: (host copy, device view)."""
    host, d = buf
    assert S >= L and base + n * S <= host.size
    return (np.ascontiguousarray(host[base:base + n * S].reshape(n, S)[:, :L]),
            d[base:base + n * S].view(n, S)[:, :L])


def pairs(t):
    return [tuple(int(x) for x in g) for g in u64(t).reshape(-1, 2)]


# digest -> (device call, oracle); the seeded oracles are per-key calls
DIGESTS = {
    "city64": (lambda kd: u64(P.city64_batch(kd)), lambda o, k: o.city64_fixed(k)),
    "city64_seeds": (lambda kd: [int(x) for x in u64(P.city64_seeds_batch(kd, S0, S1))],
                     lambda o, k: [o.city64_seeds(r.tobytes(), S0, S1) for r in k]),
    "city128": (lambda kd: u64(P.city128_batch(kd)), lambda o, k: o.city128_fixed(k)),
    "city128_seed": (lambda kd: pairs(P.city128_seed_batch(kd, (S0, S1))),
                     lambda o, k: [o.city128_seed(r.tobytes(), S0, S1) for r in k]),
    "citycrc128": (lambda kd: u64(P.citycrc128_batch(kd)), lambda o, k: o.city128_fixed(k, crc=True)),
    "citycrc128_seed": (lambda kd: pairs(P.citycrc128_seed_batch(kd, (S0, S1))),
                        lambda o, k: [o.citycrc128_seed(r.tobytes(), S0, S1) for r in k]),
}
FIVE = ("city64", "city64_seeds", "city128", "city128_seed", "citycrc128")


def check(oracle, name, k, kd, tag, where):
    got = np.asarray(DIGESTS[name][0](kd), dtype=np.uint64).reshape(len(k), -1)
    assert P.last_kernel() == tag, (name, where, P.last_kernel())
    want = np.asarray(DIGESTS[name][1](oracle, k), dtype=np.uint64).reshape(len(k), -1)
    assert (got == want).all(), (name, where, "keys", np.flatnonzero((got != want).any(axis=1))[:10])


# --------------------------------------- fixed long keys, three layouts ---
# layout -> (stride of length L, base): rows padded to a 16-B stride on a
# 16-B aligned base (GlobalReaderT<a16, lines>: dwordx4 spans, the dwordx2
# path at L % 16 == 8, the funnel at L % 8 != 0 for every span counted from
# the key's end), the same rows 8 B off (the plain reader, 8-B aligned), and
# packed rows 1 B off (the plain reader at every dword misalignment, since
# consecutive keys start L bytes apart)
LAYOUTS = {"padded": (lambda L: (L + 15) // 16 * 16, 0),
           "padded+8": (lambda L: (L + 15) // 16 * 16, 8),
           "packed+1": (lambda L: L, 1)}
LAYOUT_KERNEL = {"padded": "k_global<fixed,a16,lines>", "padded+8": "k_global<fixed>", "packed+1": "k_global<fixed>"}
N_LONG = 70  # one full wave and a ragged one (k_global: one lane per key)


def chunks(lo, hi, step=100):
    return [(a, min(a + step, hi + 1)) for a in range(lo, hi + 1, step)]


def long_case(buf, layout, L):
    stride, base = LAYOUTS[layout]
    S = stride(L)
    k, kd = rows(buf, base, N_LONG, S, L)
    return k, kd, S, base == 0


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("lo,hi", chunks(256, 640))
def test_long_keys_every_length(dev, oracle, buf, layout, lo, hi):
    """L = 256..640: (L - 1) >> 6 takes both parities for the paired rounds,
    (L - 16) % 128 every tail of city128_finish on the 16-byte Shifted reader.
    CityHashCrc128 is CityHash128 at these lengths."""
    for L in range(lo, hi):
        k, kd, S, aligned = long_case(buf, layout, L)
        tag = fixed_kernel(L, S, aligned)
        assert tag == LAYOUT_KERNEL[layout] + "@2"
        for name in FIVE:
            check(oracle, name, k, kd, tag, (layout, L))


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("lo,hi", chunks(901, 2900))
def test_crc_long_keys_every_length(dev, oracle, buf, layout, lo, hi):
    """L = 901..2900 through the CityHashCrc256 rounds (LDS CRC tables, 8 WG/CU).

    The line form streams block k as whole lines while
    line_end(k) = 240k + 16(k & 7) + (128 if (k & 7) == 7 else 256) <= L:
    line_end(2..11) = 768, 1024, 1280, 1536, 1792, 1920, 2176, 2432, 2688, 2944.
    For L in [line_end(k - 1), line_end(k)) the line form ends with block
    k - 1, so over 901..2900 it ends at each of the blocks 3..11: the last
    carried phase (k - 1) & 7 takes every value.  A plain block follows where
    block k exists (240 (k + 1) <= L): L = 960..1023 (k = 3), 1200..1279 (4),
    1440..1535 (5), 1680..1791 (6), 2160..2175 (8, the plain block after phase
    7's 128-B load), 2400..2431 (9), 2640..2687 (10) and 2880..2900 (11); for
    1792 <= L < 1920 the seven blocks all stream as lines and the tail follows
    phase 6.  (test_line_form_ends_at_every_phase checks this arithmetic.)
    2000 consecutive lengths also take every rest // 40 and rest % 40 of the
    tail (period 240) and both the 8-byte and the byte misalignments of
    L - 40."""
    for L in range(lo, hi):
        k, kd, S, aligned = long_case(buf, layout, L)
        tag = fixed_kernel(L, S, aligned, crc=True)
        assert tag == LAYOUT_KERNEL[layout] + "@8"
        check(oracle, "citycrc128", k, kd, tag, (layout, L))
        check(oracle, "citycrc128_seed", k[:4], kd[:4], tag, (layout, L))


def test_line_form_ends_at_every_phase():
    """The arithmetic of the docstring above: over L = 901..2900 the line form
    ends at each of the blocks 3..11 (every phase is the last one carried),
    and a plain block follows at all of them but 7."""
    def line_end(k):
        return 240 * k + 16 * (k & 7) + (128 if (k & 7) == 7 else 256)
    assert line_end(10) == 2688
    ends, plain_follows = set(), set()
    for L in range(901, 2901):
        k = next(k for k in range(13) if line_end(k) > L)
        ends.add(k)
        if k < L // 240:
            plain_follows.add(k)
    assert ends == set(range(3, 12)) and {(k - 1) & 7 for k in ends} == set(range(8))
    assert plain_follows == {3, 4, 5, 6, 8, 9, 10, 11}


# ------------------------------------------------ short keys on k_global ---
@pytest.mark.parametrize("stride", [272, 261])
@pytest.mark.parametrize("lo,hi", chunks(0, 255, 128))
def test_short_keys_on_global_reader(dev, oracle, buf, stride, lo, hi):
    """A key column of a wide record table: a row stride of 261 or more sends
    keys of any length through k_global, so len0to16, len17to32, len33to64 and
    murmur128 run on GlobalReaderT, in a16,lines form (stride 272) and plain
    (stride 261: every dword misalignment)."""
    n = 131
    for L in range(lo, hi):
        k, kd = rows(buf, 0, n, stride, L)
        tag = fixed_kernel(L, stride, True)
        assert tag == ("k_global<fixed,a16,lines>@2" if stride == 272 else "k_global<fixed>@2")
        for name in FIVE:
            check(oracle, name, k, kd, tag, (stride, L))
        if L == 0:  # the empty key's digests, read from nowhere
            assert (u64(P.city64_batch(kd)) == K2).all() and oracle.city64(b"") == K2
            assert pairs(P.city128_batch(kd)) == [oracle.city128(b"")] * n
            assert pairs(P.citycrc128_batch(kd)) == [oracle.citycrc128(b"")] * n


# ------------------------------------------ strided rows, window steps ---
def window_step_strides(L):
    """The strides on both sides of tile = 63 * S + L + 16 = 12288 and = 16384
    (the 12 KiB window, the 16 KiB window, k_global), and S = L + 1.  A stride
    below L is no layout (the library refuses it), so L = 200, whose packed
    tile of 12816 B is already past 12288, has the second step only."""
    s = [L + 1]
    for edge in (12288, 16384):
        at = (edge - L - 16) // 63  # the largest stride whose tile still fits
        s += [x for x in (at, at + 1) if x >= L]
    return sorted(set(s))


def test_window_step_strides():
    assert window_step_strides(100) == [101, 193, 194, 258, 259]
    assert window_step_strides(13) == [14, 194, 195, 259, 260]
    assert window_step_strides(64) == [65, 193, 194, 258, 259]
    assert window_step_strides(200) == [201, 256, 257]
    for L in (13, 64, 100, 200):
        tags = {fixed_kernel(L, S, False) for S in window_step_strides(L)}
        assert tags == {"k_window<fixed,nt,12K>@3", "k_window<fixed,nt,16K>@2", "k_global<fixed>@2"} - (
            {"k_window<fixed,nt,12K>@3"} if L == 200 else set())


@pytest.mark.parametrize("L", [13, 64, 100, 200])
def test_strided_rows_at_the_window_steps(dev, oracle, buf, L):
    for S in window_step_strides(L):
        for base in (0, 3):
            for n in (63, 64, 65, 257):
                k, kd = rows(buf, base, n, S, L)
                tag = fixed_kernel(L, S, base == 0)
                for name in ("city64", "city128", "citycrc128", "city64_seeds"):
                    check(oracle, name, k, kd, tag, (L, S, base, n))


def test_stride_below_keylen_is_refused(dev, buf):
    """L = 200 below its first window step: rows that overlap are no layout."""
    kd = torch.as_strided(buf[1], (64, 200), (191, 1))
    with pytest.raises(P.PdhtError, match="stride < keylen"):
        P.city64_batch(kd)


# ------------------------------------------- variable-length keys ---
# The ladder: keys of 0..2200 bytes, each length once, and one 16-B filler key
# (id 2201) that the steered orders repeat.  POOL holds them back to back; the
# digests of every id are computed once (fixture ladder_ref) and a batch's
# expected digests are a permutation of them.
LADDER = 2201
FILLER = LADDER
LEN = np.concatenate([np.arange(LADDER), [16]]).astype(np.int64)
START = np.concatenate([[0], np.cumsum(LEN)]).astype(np.int64)
POOL = np.random.default_rng(0x1ADDE2).integers(0, 256, int(START[-1]), dtype=np.uint8)
LONG_IDS = np.arange(901, LADDER)  # the lengths that take the CityHashCrc256 rounds
WINDOWS = (10224, 16384)
MISALIGN = (0, 1, 7, 15)


def steered_order(win, in_lds, in_global, seed):
    """An order (ids, whole 64-key tiles) in which window `win` holds every key
    of `in_lds` and none of `in_global`, at any base misalignment: each tile
    opens with keys of in_lds that end at most win - 16 bytes in, then keys of
    at most 900 bytes (largest first) until the tile is past the window's end,
    then its share of in_global and of the remaining short keys, then fillers."""
    rng = np.random.default_rng(seed)
    tiles, cur, tot = [], [], 0
    for i in rng.permutation(in_lds):
        if tot + LEN[i] > win - 16:
            tiles.append(cur)
            cur, tot = [], 0
        cur.append(int(i))
        tot += int(LEN[i])
    tiles.append(cur)
    short = list(range(900, -1, -1))
    for t in tiles:
        tot = int(LEN[t].sum())
        while tot <= win:
            t.append(short.pop(0))
            tot += int(LEN[t[-1]])
    rest = rng.permutation(np.concatenate([np.asarray(in_global, dtype=np.int64), np.asarray(short, dtype=np.int64)]))
    for j, i in enumerate(rest):
        tiles[j % len(tiles)].append(int(i))
    assert max(len(t) for t in tiles) <= 64
    return np.concatenate([t + [FILLER] * (64 - len(t)) for t in tiles]).astype(np.int64)


def _orders():
    """Two plain shuffles of the ladder (35 tiles, ragged last one, whose
    windows hold only their first few keys), and per window two steered
    orders that between them put each half of the long keys once inside the
    window and once past it.  (The long keys are 2 MB and the 35 windows of a
    bare ladder hold 0.6 MB at most, so no two orders of it can show every
    long key from LDS; the fillers make room for more tiles.)"""
    o = {"shuffle-a": np.random.default_rng(1).permutation(LADDER),
         "shuffle-b": np.random.default_rng(2).permutation(LADDER)}
    half = np.random.default_rng(3).permutation(LONG_IDS)
    x, y = half[:half.size // 2], half[half.size // 2:]
    for win in WINDOWS:
        o[f"lds{win}-x"] = steered_order(win, x, y, 4)
        o[f"lds{win}-y"] = steered_order(win, y, x, 5)
    return o


ORDERS = _orders()


def batch_of(order):
    """(key bytes, offsets) of the ids in `order`, back to back."""
    offs = np.concatenate([[0], np.cumsum(LEN[order])]).astype(np.int64)
    data = np.concatenate([POOL[START[i]:START[i] + LEN[i]] for i in order])
    return data, offs


@pytest.fixture(scope="module")
def ladder_ref(oracle):
    offs = START.astype(np.uint64)
    return {"city64": oracle.city64_var(POOL, offs), "city128": oracle.city128_var(POOL, offs),
            "citycrc128": oracle.city128_var(POOL, offs, crc=True)}


VAR_ABI = {"city64": ("pdht_city64_batch_var_dev", 1), "city128": ("pdht_city128_batch_var_dev", 2),
           "citycrc128": ("pdht_citycrc128_batch_var_dev", 2)}


def var_digests(name, dd, od, win):
    """The digests of a batch through window `win`: the wrapper when the
    batch's mean key length selects that window, else the C ABI with
    nbytes = 0 (unknown: the short-key window)."""
    n = od.numel() - 1
    total = int(od[-1].item() - od[0].item())
    if VAR_WINDOW_KERNELS[win] == var_kernel(total, n):
        got = getattr(P, name + "_var_batch")(dd, od)
    else:
        assert win == 10224
        got = torch.empty((n, VAR_ABI[name][1]), dtype=torch.int64, device=dd.device)
        assert getattr(P.lib(), VAR_ABI[name][0])(dd.data_ptr(), 0, od.data_ptr(), n, got.data_ptr(), None) == 0
    assert P.last_kernel() == VAR_WINDOW_KERNELS[win]
    return u64(got).reshape(n, -1)


def misaligned(data, m, dev):
    """`data` on the device, m bytes past a 16-B aligned address."""
    t = torch.empty(data.size + 16, dtype=torch.uint8, device=dev)
    assert t.data_ptr() % 16 == 0
    t[m:m + data.size].copy_(torch.from_numpy(data))
    return t[m:m + data.size]


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_var_length_ladder(dev, oracle, ladder_ref, order):
    """Every length 0..2200 in one batch, through both windows, at four base
    misalignments (the window's edge moves with them), bit-exact."""
    ids = ORDERS[order]
    data, offs = batch_of(ids)
    od = torch.from_numpy(offs).to(dev)
    for m in MISALIGN:
        dd = misaligned(data, m, dev)
        for win in WINDOWS:
            for name, ref in ladder_ref.items():
                got = var_digests(name, dd, od, win)
                bad = np.flatnonzero((got != ref[ids].reshape(got.shape)).any(axis=1))
                assert bad.size == 0, (name, order, m, win, "lengths", sorted(set(LEN[ids[bad]].tolist()))[:20])


def test_var_ladder_orders_show_every_long_key_from_lds_and_from_global():
    """With the kernel's own rule (hash_ref.var_from_lds) over the offsets of
    the batches test_var_length_ladder runs: per window, every length above
    900 is hashed at least once out of LDS and once from global memory."""
    for win in WINDOWS:
        lds, glb = np.zeros(LADDER, bool), np.zeros(LADDER, bool)
        for order, ids in ORDERS.items():
            offs = np.concatenate([[0], np.cumsum(LEN[ids])])
            for m in MISALIGN:
                inside = var_from_lds(offs, m, win)
                ladder = ids < LADDER
                lds[ids[ladder & inside]] = True
                glb[ids[ladder & ~inside]] = True
            if order.startswith("shuffle"):
                print(f"window {win}, {order} alone at misalignment {m}: {int(inside[ids > 900].sum())} of "
                      f"{LONG_IDS.size} long keys from LDS")
        print(f"window {win}: of the {LONG_IDS.size} lengths 901..2200, {int(lds[LONG_IDS].sum())} seen from LDS and "
              f"{int(glb[LONG_IDS].sum())} from global memory; of 0..900, {int(lds[:901].sum())} and "
              f"{int(glb[:901].sum())}")
        assert lds[LONG_IDS].all() and glb[LONG_IDS].all(), win


@pytest.mark.parametrize("k", [1, 64, 100])
def test_var_offsets_not_from_zero(dev, oracle, ladder_ref, k):
    """offsets[k:] over the whole data tensor: the batch starts k keys in (its
    tiles, and so its windows, move), the digests are rows k: of the full
    batch's."""
    ids = ORDERS["shuffle-a"]
    data, offs = batch_of(ids)
    dd, od = misaligned(data, 0, dev), torch.from_numpy(offs).to(dev)
    for name, ref in ladder_ref.items():
        full = u64(getattr(P, name + "_var_batch")(dd, od)).reshape(ids.size, -1)
        got = u64(getattr(P, name + "_var_batch")(dd, od[k:])).reshape(ids.size - k, -1)
        assert P.last_kernel() == var_kernel(int(offs[-1] - offs[k]), ids.size - k) == VAR_WINDOW_KERNELS[16384]
        assert (got == full[k:]).all() and (got == ref[ids[k:]].reshape(got.shape)).all(), name


@pytest.mark.parametrize("win", WINDOWS)
def test_var_keys_at_the_window_edge(dev, oracle, win):
    """Per base misalignment m = 0..15, three tiles whose second key ends d =
    -1, 0, +1 bytes from the window's end behind a first key that fills the
    window up to 200 bytes (about 10 or 16 KiB through LdsReader, the CRC
    rounds and their LDS tables included), then 62 keys of 0..40 bytes, all
    past the window; a tile of 16-B fillers keeps the mean key length on this
    window's side of 160 B."""
    rng = np.random.default_rng(win)
    for m in range(16):
        lens, at = [], 0
        for d in (-1, 0, 1):
            a = (m + at) % 16  # the tile's first byte within its 16-B block
            tile = [win - a - 200, 200 + d] + rng.integers(0, 41, 62).tolist()
            lens += tile
            at += sum(tile)
        lens += [16] * 64
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        inside = var_from_lds(offs, m, win)
        assert inside[[0, 64, 128]].all() and inside[[1, 65, 129]].tolist() == [True, True, False]
        assert not inside[130:192].any() and inside[192:].all()  # (empty keys right at the edge stay inside)
        data = rng.integers(0, 256, int(offs[-1]), dtype=np.uint8)
        dd, od = misaligned(data, m, dev), torch.from_numpy(offs).to(dev)
        assert var_kernel(int(offs[-1]), len(lens)) == VAR_WINDOW_KERNELS[win]
        uo = offs.astype(np.uint64)
        for name, want in (("city64", oracle.city64_var(data, uo)), ("city128", oracle.city128_var(data, uo)),
                           ("citycrc128", oracle.city128_var(data, uo, crc=True))):
            got = u64(getattr(P, name + "_var_batch")(dd, od)).reshape(len(lens), -1)
            assert P.last_kernel() == VAR_WINDOW_KERNELS[win]
            bad = np.flatnonzero((got != want.reshape(got.shape)).any(axis=1))
            assert bad.size == 0, (name, win, m, "keys", bad[:10])
