"""The case grids of test_gpu_key_lengths.py and test_gpu_moduli.py, and what
they cover, asserted without a GPU.

The GPU files import the grids from here.  Every key length gets one case per
rank count; the byte offset of the keys, nptes, the value size E and the
key-slot form rotate over those cases instead of forming a product, so the
tests below check that the rotation still brings every branch the generic
bucketing path can take (bucket.h: packed_key_hash on GlobalReader, copy_row,
OutRecT::key_copy's pad loop; table.h: k_get_resolve's group-strided compare)
together with both offsets and both generic kernel shapes.

The last tests restate make_fastmod (pdht_hip.hip) and FastMod::mod
(kernels.h) in Python integers and run them over the adversarial grid that
test_gpu_moduli.py hands the device."""
import numpy as np

import bucket_ref as B

# ---------------------------------------------------------------- lengths ---
LENGTHS = tuple(range(1, 73)) + (80, 96, 100, 127, 128, 129, 255, 256, 257, 1000)
N = 16384 + 8192 + 2048 + 77  # two wg<8> tiles (four wg<4> tiles), the last one ragged with whole waves idle
NRANKS = (1, 7, 1000, 4097)  # nbits 0, 3, 10, 13; k_bucket_scatter_wg<8> up to 4096 ranks, wg<4> above
NPTES = (1, 3, 0xFFFFFFFB, 0x80000000, 65537)
ES = (1, 8, 12, 40, 64, 256)
OFFSETS = (0, 1)  # of the keys' first byte from a 16-B aligned address


def big_slot(L):
    """The smallest multiple of 8 that is >= max(L, 32)."""
    return (max(L, 32) + 7) // 8 * 8


def bucket_cases():
    """(L, nranks, offset, nptes, E, key_slot), one per length and rank count.
    The offset alternates with the length and flips again every 16 lengths,
    so that L and L + 16 meet a rank count at different offsets."""
    cases = []
    for iL, L in enumerate(LENGTHS):
        for inr, nr in enumerate(NRANKS):
            off = OFFSETS[(iL + iL // 16 + inr) % 2]
            nptes = NPTES[(iL + inr) % len(NPTES)]
            E = ES[(iL + 2 * inr + iL // len(ES)) % len(ES)]
            slot = big_slot(L) if ((iL + inr) // 2) % 2 else 0
            cases.append((L, nr, off, nptes, E, slot))
    return cases


BUCKET_CASES = bucket_cases()


def chunks(step=12):
    """LENGTHS in runs of at most `step` lengths and about 260 key bytes per key, one run per pytest case."""
    out, cur, tot = [], [], 0
    for L in LENGTHS:
        if cur and (len(cur) == step or tot + L > 260):
            out.append(tuple(cur))
            cur, tot = [], 0
        cur.append(L)
        tot += L
    out.append(tuple(cur))
    return out


CHUNKS = chunks()


def generic_kernel(nranks):
    return "k_bucket_scatter_wg<8>" if nranks <= 4096 else "k_bucket_scatter_wg<4>"


def expected_kernel(L, nranks, off, records):
    """At offset 0 whatever bucket_ref._bucket_kernel predicts (8/16/32-B keys take the staged and two-pass
    kernels there), the generic kernel in every other case."""
    return B._bucket_kernel(L, nranks, 0, records) if off == 0 else generic_kernel(nranks)


def city64_branch(L):
    """The length branch of city64 (city_core.h) a key of L bytes takes."""
    return "1-3" if L <= 3 else "4-7" if L <= 7 else "8-16" if L <= 16 else "17-32" if L <= 32 else \
        "33-64" if L <= 64 else ">64"


# ---------------------------------------------------------------- resolve ---
CHAIN_N, CHAIN_ABSENT = 3000, 200
HEADS = (1, 8)
FORGE_ES = (1, 256)


def chain_params(L):
    """(E, key_slot) of the put / get / resolve chain at length L."""
    i = LENGTHS.index(L)
    return ES[i % len(ES)], big_slot(L) if (i // len(ES)) % 2 else 0


def resolve_piece(head, slot, E):
    """get_resolve()'s piece (pdht_table.hip) for replies and values in 256-B aligned allocations, replies of
    head + slot + E bytes and value rows of E bytes."""
    bits = (head + slot) | (head + slot + E) | E
    return 16 if bits % 16 == 0 else 8 if bits % 8 == 0 else 4 if bits % 4 == 0 else 1


def resolve_group(L, head, slot, E):
    """k_get_resolve's lane group G: lanes for the value pieces and for the key at 4 bytes a lane, a power of
    two, at most a wave."""
    want = max(E // resolve_piece(head, slot, E), (L + 3) // 4)
    G = 1
    while G < 64 and G < want:
        G *= 2
    return G


# ---------------------------------------------------------------- placement ---
PLACE_LENGTHS = (8, 16, 32, 64, 13, 100, 200, 256, 300, 1000)
PLACE_N = 70_001
PLACE_NRANKS = (1000, 4096, 4097)  # LDS bins, the LDS limit (kHistLds = 4096), global atomics
PLACE_KEYSETS = ("random", "identical", "alternating")


def place_kernel(L, hist):
    """launch_fixed's choice (launch.h) for PLACE_N packed, 16-B aligned keys."""
    from hash_ref import fixed_kernel
    if L == 8:
        return "k_fixed_direct<8,8,nt,1024>@1" if hist else "k_fixed_direct<8,4,nt>@8"
    if L == 16:
        return "k_fixed_direct<16,2,nt,1024>@2" if hist else "k_fixed_direct<16,2,nt>@8"
    if L == 32:
        return "k_fixed_direct<32,2,nt>@8"
    if L == 64:
        return "k_fixed_xpose64<nt,d2,1024>@1" if hist else "k_fixed_xpose64<nt,d2>@3"
    return fixed_kernel(L, L, True)


# ------------------------------------------------------------------ moduli ---
M64 = (1 << 64) - 1
# every rank count and nptes a test of the suite hands the library
SUITE_MODULI = (1, 2, 3, 4, 5, 7, 8, 9, 64, 255, 256, 511, 512, 600, 1000, 1024, 1025, 1462, 1463, 1535, 1536,
                1574, 1575, 2047, 2048, 2049, 4096, 4097, 8192, 65537, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
NAMED_MODULI = (0x7FFFFFFF, 0x7FFFFFED, 0xFFFFFFFB, 65537)


def pow2_edges(kmax, top):
    """2^k - 1, 2^k, 2^k + 1 for k = 1..kmax, within 1..top, in that order, each once."""
    out = []
    for k in range(1, kmax + 1):
        for d in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            if 1 <= d <= top and d not in out:
                out.append(d)
    return out


NPTES_EDGES = pow2_edges(32, (1 << 32) - 1)
NRANKS_EDGES = pow2_edges(31, (1 << 31) - 1)  # nranks is c->size, an int
PLACE_MODULI = [(NPTES_EDGES[i % len(NPTES_EDGES)], NRANKS_EDGES[i % len(NRANKS_EDGES)])
                for i in range(max(len(NPTES_EDGES), len(NRANKS_EDGES)))]  # the diagonal of the two lists
MODULI_N = 4099
MODULI_BUCKET = [(L, 7, nptes) for L in (8, 13) for nptes in NPTES_EDGES]


def divisors():
    rng = np.random.default_rng(0xD1F)
    d = set(NPTES_EDGES) | set(SUITE_MODULI) | set(NAMED_MODULI)
    d |= {int(x) for x in rng.integers(1, 1 << 32, 300, dtype=np.uint64)}
    for bits in rng.integers(1, 33, 300):  # a random bit length, then a value of exactly that length
        d.add(int(rng.integers(1 << (int(bits) - 1), 1 << int(bits), dtype=np.uint64)))
    return sorted(d)


def dividends(d, rng):
    """The dividends that show a wrong magic number or shift for divisor d: the ends of the range, and the
    multiples of d (with their neighbours) at the largest quotients, at small ones and at 20 random ones."""
    top = (1 << 64) // d
    qs = [top, top - 1, top // 2, 1, 2]
    qs += [int(q) for q in rng.integers(0, min(top, M64), 20, dtype=np.uint64, endpoint=True)]
    n = [0, 1, d - 1, d, d + 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, M64 - 1, M64]
    for q in qs:
        n += [q * d - 1, q * d, q * d + 1]
    return [x for x in n if 0 <= x <= M64]


def moduli_grid():
    """[(divisor, [dividends])], seeded."""
    rng = np.random.default_rng(0x64D)
    return [(d, dividends(d, rng)) for d in divisors()]


def make_fastmod(d):
    """make_fastmod (pdht_hip.hip) in Python integers: (d, m, sh, pow2)."""
    if d & (d - 1) == 0:
        return d, 0, 0, 1
    l = (d - 1).bit_length()  # ceil(log2 d)
    m = (((1 << l) - d) << 64) // d + 1
    assert 0 < m <= M64 and 2 <= l <= 64
    return d, m, l - 1, 0


def fastmod(f, n):
    """FastMod::mod (kernels.h) with every intermediate cut to 64 bits."""
    d, m, sh, pow2 = f
    if pow2:
        return n & (d - 1)
    t = (m * n) >> 64
    q = ((t + (((n - t) & M64) >> 1)) & M64) >> sh
    return (n - q * d) & M64


# =================================================================== tests ===
def test_lengths_and_batch():
    assert LENGTHS[:72] == tuple(range(1, 73))
    assert set(LENGTHS[72:]) == {80, 96, 100, 127, 128, 129, 255, 256, 257, 1000}
    assert N == 26701 and N > 2 * 8 * 1024 and N > 3 * 4 * 2048  # (tiles of W x 16 keys per lane x 64 lanes)
    assert [L for c in CHUNKS for L in c] == list(LENGTHS)
    assert max(len(c) for c in CHUNKS) <= 12 and max(sum(c) for c in CHUNKS if len(c) > 1) <= 260
    nbits = []
    for nr in NRANKS:
        b = 0
        while (1 << b) < nr:
            b += 1
        nbits.append(b)
    assert nbits == [0, 3, 10, 13]
    assert {generic_kernel(nr) for nr in NRANKS} == {"k_bucket_scatter_wg<8>", "k_bucket_scatter_wg<4>"}


def test_every_length_meets_every_rank_count_and_both_offsets():
    assert len(BUCKET_CASES) == len(LENGTHS) * len(NRANKS)
    assert {(c[0], c[1]) for c in BUCKET_CASES} == {(L, nr) for L in LENGTHS for nr in NRANKS}
    for L in LENGTHS:
        mine = [c for c in BUCKET_CASES if c[0] == L]
        assert {c[2] for c in mine} == {0, 1}, L
        assert {bool(c[5]) for c in mine} == {False, True}, L  # both key-slot forms
        for c in mine:
            assert c[5] in (0, big_slot(L)) and big_slot(L) % 8 == 0 and big_slot(L) >= max(L, 32) > big_slot(L) - 8


def test_every_residue_of_16_at_both_offsets_in_both_generic_shapes():
    """packed_key_hash's GlobalReader and copy_row see the key's address modulo 16 and 4: consecutive keys
    start L bytes apart, so L % 16 and the offset of key 0 give every alignment class."""
    for wg in ("k_bucket_scatter_wg<8>", "k_bucket_scatter_wg<4>"):
        for records in (False, True):
            seen = {(L % 16, off) for (L, nr, off, *_r) in BUCKET_CASES
                    if expected_kernel(L, nr, off, records) == wg}
            assert seen == {(r, off) for r in range(16) for off in (0, 1)}, (wg, records)


def test_copy_row_dword_branch():
    """copy_row copies dwords when source, destination and L are all multiples of 4: offset 0 and L % 4 == 0
    on the generic kernel (8/16/32-B keys leave it at offset 0).  Every such length but 64 is new."""
    dword = {L for (L, nr, off, *_r) in BUCKET_CASES
             if off == 0 and L % 4 == 0 and expected_kernel(L, nr, off, False).startswith("k_bucket_scatter_wg")}
    assert dword == {L for L in LENGTHS if L % 4 == 0 and L not in (8, 16, 32)}
    assert {12, 20, 24, 28, 64, 1000} <= dword
    # and the byte branch at those lengths too (offset 1), 8/16/32 included
    byte = {L for (L, nr, off, *_r) in BUCKET_CASES if off == 1 and L % 4 == 0}
    assert byte == {L for L in LENGTHS if L % 4 == 0}


def test_keys_out_ends_off_a_dword():
    ends = {(N * L) % 4 for L in LENGTHS}
    assert ends == {0, 1, 2, 3} and N % 4 == 1


def test_every_record_pad():
    """OutRecT::key_copy zero-fills from L to the stride: every pad length 0..7, on both generic shapes."""
    for wg in ("k_bucket_scatter_wg<8>", "k_bucket_scatter_wg<4>"):
        pads = {-L % 8 for (L, nr, off, *_r) in BUCKET_CASES if expected_kernel(L, nr, off, True) == wg}
        assert pads == set(range(8)), wg


def test_every_city64_branch_at_both_offsets():
    want = {"1-3", "4-7", "8-16", "17-32", "33-64", ">64"}
    for off in (0, 1):
        for wg in ("k_bucket_scatter_wg<8>", "k_bucket_scatter_wg<4>"):
            got = {city64_branch(L) for (L, nr, o, *_r) in BUCKET_CASES
                   if o == off and expected_kernel(L, nr, o, False) == wg}
            assert got == want, (off, wg)
    assert {city64_branch(L) for L in (1, 3, 4, 7, 8, 16, 17, 32, 33, 64, 65)} == want


def test_nptes_and_value_sizes_rotate_over_everything():
    for nr in NRANKS:
        assert {c[3] for c in BUCKET_CASES if c[1] == nr} == set(NPTES)
        assert {c[4] for c in BUCKET_CASES if c[1] == nr} == set(ES)
    for off in (0, 1):
        assert {c[3] for c in BUCKET_CASES if c[2] == off} == set(NPTES)
        assert {c[4] for c in BUCKET_CASES if c[2] == off} == set(ES)
    for slot_on in (False, True):
        assert {c[4] for c in BUCKET_CASES if bool(c[5]) == slot_on} == set(ES)
    for r in range(8):  # every E and every nptes meets every pad
        assert {c[4] for c in BUCKET_CASES if c[0] % 8 == r} == set(ES)
        assert {c[3] for c in BUCKET_CASES if c[0] % 8 == r} == set(NPTES)


def test_staged_and_two_pass_kernels_only_where_predicted():
    other = {(L, nr) for (L, nr, off, *_r) in BUCKET_CASES
             if not expected_kernel(L, nr, off, False).startswith("k_bucket_scatter_wg")}
    assert other and {L for L, _ in other} <= {8, 16, 32}
    assert all(off == 0 for (L, nr, off, *_r) in BUCKET_CASES if (L, nr) in other)


def test_chain_and_forged_replies_put_L_on_both_sides_of_the_group():
    for L in LENGTHS:
        E, slot = chain_params(L)
        assert E in ES and slot in (0, big_slot(L))
    assert {chain_params(L)[0] for L in LENGTHS} == set(ES)
    assert {bool(chain_params(L)[1]) for L in LENGTHS} == {False, True}
    below, at, above, groups = set(), set(), set(), set()
    for L in LENGTHS:
        slot = (L + 7) // 8 * 8
        for head in HEADS:
            for E in FORGE_ES:
                G = resolve_group(L, head, slot, E)
                groups.add(G)
                (below if L < G else at if L == G else above).add(L)
    assert groups == {1, 2, 4, 8, 16, 32, 64}
    # E = 1: the key alone sizes the group (G = 1 for L <= 4, 2 for L <= 8); E = 256 at head 1 moves bytes: G = 64
    assert all(resolve_group(L, h, 8, 1) == (1 if L <= 4 else 2) for L in range(1, 9) for h in HEADS)
    assert all(resolve_group(L, 1, (L + 7) // 8 * 8, 256) == 64 for L in LENGTHS)
    assert set(range(1, 64)) <= below and 64 in at and {65, 72, 100, 1000} <= above and set(range(3, 73)) <= above


def test_place_lengths_hit_every_kernel_family():
    fam = {}
    for L in PLACE_LENGTHS:
        for hist in (False, True):
            fam.setdefault(place_kernel(L, hist).split("<")[0] + ("<fixed" if L not in (8, 16, 32, 64) else ""),
                           set()).add((L, hist))
    assert set(fam) == {"k_fixed_direct", "k_fixed_xpose64", "k_window<fixed", "k_global<fixed"}
    for name, cases in fam.items():
        assert {h for _, h in cases} == {False, True}, name
    assert {place_kernel(L, True) for L in (13, 100, 200, 256, 300, 1000)} == {
        "k_window<fixed,nt,12K>@3", "k_window<fixed,nt,16K>@2", "k_global<fixed,a16,lines>@2", "k_global<fixed>@2"}
    assert max(PLACE_NRANKS) > 4096 and 4096 in PLACE_NRANKS and min(PLACE_NRANKS) < 4096  # kHistLds


def test_moduli_edges():
    assert NPTES_EDGES[:6] == [1, 2, 3, 4, 5, 7] and NPTES_EDGES[-2:] == [(1 << 31) + 1, (1 << 32) - 1]
    assert max(NPTES_EDGES) == (1 << 32) - 1 and max(NRANKS_EDGES) == (1 << 31) - 1
    for k in range(1, 33):
        for d in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            assert (d in NPTES_EDGES) == (d < 1 << 32)
            assert (d in NRANKS_EDGES) == (d < 1 << 31)
    assert {p for p, _ in PLACE_MODULI} == set(NPTES_EDGES) and {r for _, r in PLACE_MODULI} == set(NRANKS_EDGES)
    # every nptes edge meets bucketing, on the staged (8 B) and on the generic (13 B) kernel
    for L in (8, 13):
        assert {c[2] for c in MODULI_BUCKET if c[0] == L} == set(NPTES_EDGES)
    assert set(NPTES) <= set(NPTES_EDGES) | {0xFFFFFFFB}


def test_moduli_grid_shape():
    grid = moduli_grid()
    ds = [d for d, _ in grid]
    assert ds == sorted(set(ds)) and 600 <= len(ds) <= 740 and ds[0] == 1 and ds[-1] == (1 << 32) - 1
    assert set(NPTES_EDGES) | set(SUITE_MODULI) | set(NAMED_MODULI) <= set(ds)
    assert {d.bit_length() for d in ds} == set(range(1, 33))
    pairs = sum(len(ns) for _, ns in grid)
    print(f"{len(ds)} divisors, {pairs} pairs")
    assert 40_000 <= pairs <= 70_000
    for d, ns in grid:
        top = (1 << 64) // d
        assert {0, 1, d - 1, d, M64, 1 << 63} <= set(ns) and all(0 <= n <= M64 for n in ns)
        assert top * d in ns or top * d > M64
        assert top * d - 1 in ns and (top - 1) * d in ns and 2 * d + 1 in ns
    assert grid == moduli_grid()  # seeded


def test_fastmod_restated_agrees_with_python_integers():
    """make_fastmod + FastMod::mod, restated, against % over the whole grid: the check the reference alone
    passes."""
    bad, pairs = [], 0
    for d, ns in moduli_grid():
        f = make_fastmod(d)
        for n in ns:
            pairs += 1
            if fastmod(f, n) != n % d:
                bad.append((d, n))
    assert not bad, (len(bad), pairs, bad[:5])


def test_fastmod_restated_notices_the_mutations():
    """The grid is only worth its launches if a magic number without its + 1, or a shift one off, fails on it."""
    grid = moduli_grid()

    def wrong(mutate):
        out = set()
        for d, ns in grid:
            f = make_fastmod(d)
            if f[3]:
                continue
            g = mutate(f)
            if any(fastmod(g, n) != n % d for n in ns):
                out.add(d)
        return out
    not_pow2 = {d for d, _ in grid if d & (d - 1)}
    assert wrong(lambda f: (f[0], f[1] - 1, f[2], 0)) == not_pow2
    assert wrong(lambda f: (f[0], f[1], f[2] + 1, 0)) == not_pow2
    assert wrong(lambda f: (f[0], f[1], max(f[2] - 1, 0), 0)) >= {d for d in not_pow2 if d > 3}
