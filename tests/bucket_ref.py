"""Helpers of the bucketing tests: keys whose ranks are chosen, the rank
distributions built from them, the two-pass digit split, the kernel the
library is expected to pick, and one checker per output kind.

The checkers never trust a requested rank: they hash the batch that was
actually sent with oracle.pdht_hash_fixed and compare every output byte for
byte with np.argsort(rank, kind="stable") of it."""
from collections import OrderedDict

import numpy as np

POOL = 1 << 20
TILE = 2048  # the smallest tile of any bucketing kernel, a divisor of the others

_POOLS = OrderedDict()


def _oracle():
    from oracle import oracle as O
    return O


def _pool(L, nranks):
    """2^20 random L-byte keys sorted by rank, hashed once per (L, nranks):
    (keys in rank order, first pool row of every rank, pool keys per rank).
    The few most recent pools are kept (32 MiB each at 32-B keys)."""
    if (L, nranks) in _POOLS:
        _POOLS.move_to_end((L, nranks))
        return _POOLS[L, nranks]
    rng = np.random.default_rng(L * 100003 + nranks)
    pool = rng.integers(0, 256, (POOL, L), dtype=np.uint8)
    _, _, r = _oracle().pdht_hash_fixed(pool, 1, nranks)
    count = np.bincount(r, minlength=nranks).astype(np.int64)
    assert count.min() > 0, (L, nranks)
    starts = np.concatenate([[0], np.cumsum(count)[:-1]])
    _POOLS[L, nranks] = (pool[np.argsort(r, kind="stable")], starts, count)
    while len(_POOLS) > 4:
        _POOLS.popitem(last=False)
    return _POOLS[L, nranks]


def keys_with_ranks(ranks, L, nranks, seed):
    """uint8 [n, L]: key i hashes to rank ranks[i] (a random pool key of that rank; repeats are fine)."""
    ranks = np.asarray(ranks, dtype=np.int64)
    assert ranks.ndim == 1 and (ranks.size == 0 or (ranks.min() >= 0 and ranks.max() < nranks))
    pool, starts, count = _pool(L, nranks)
    pick = np.random.default_rng(seed).integers(0, 1 << 62, ranks.size, dtype=np.int64)
    return pool[starts[ranks] + pick % count[ranks]]


def digits(L, nranks, records):
    """(fbits, F, C) of the two-pass sort's rank = c * F + f, restating
    digit_split() of pdht_bucket.hip: the balanced split, and one fine bit
    more for array outputs of 8/16-B keys while it stays within 8 bits and
    within the rank's bits."""
    nbits = 0
    while (1 << nbits) < nranks:
        nbits += 1
    fbits = (nbits + 1) // 2
    if not records and L <= 16 and fbits + 1 <= min(8, nbits):
        fbits += 1
    F = 1 << fbits
    return fbits, F, (nranks + F - 1) // F


def _bucket_kernel(L, nranks, variant, records=False):
    """Product: the staged scatter for 8/16/32-B keys below the two-pass
    threshold (arrays 1575 / 1575 / 2049 ranks, records 2048 / 1463 / 256 for
    8 / 16 / 32-B keys), two passes from it, the generic
    kernel for other lengths.  Tuning variants: 21 forces the generic-length
    kernel, 70 one pass up to 2048 ranks, 71 two passes from 2 ranks up, 85
    the staged scatter in the static tile order instead of per-XCD tickets,
    83 / 87 / 89 the staged scatter with owner-table ranking on 8 x 16 / 4 x
    16 tiles or with ballots, at any nranks."""
    wg = "k_bucket_scatter_wg<8>" if nranks <= 4096 else "k_bucket_scatter_wg<4>"
    if variant == 21:
        return wg
    if L in (8, 16, 32):
        two_pass_from = ({8: 2048, 16: 1463, 32: 256} if records else {8: 1575, 16: 1575, 32: 2049})[L]
        one_pass = variant == 70 and nranks <= 2048
        if (variant == 71 and nranks >= 2) or (not one_pass and nranks >= two_pass_from):
            # the tile-local form (r06); the r02-r05 form under 290 and its shape variants
            r05 = variant in (290, 202, 264) or 265 <= variant <= 272
            return f"k_bucket_pass2<{L}B>" if r05 else f"k_bucket_tl_pass2<{L}B>"
        # staged_shape(): owner-table ranking from 512 ranks, on 8 x 16
        # tiles for array outputs of 8/16-B keys while 81920 + 52 B per rank
        # of dynamic LDS and the kernel's 40 fixed bytes fit a CU, else (and
        # for records) on 4 x 16 tiles while 40960 + 28 B per rank stay within
        # 80 KiB; ballots otherwise
        if variant == 83:
            return f"k_bucket_scatter_staged<{L}B,own,8x16>"
        if variant == 87:
            return f"k_bucket_scatter_staged<{L}B,own>"
        if variant in (85, 89) or nranks < 512:
            return f"k_bucket_scatter_staged<{L}B>"
        if not records and L != 32 and 81920 + 52 * nranks + 40 <= 160 * 1024:
            return f"k_bucket_scatter_staged<{L}B,own,8x16>"
        if 40960 + 28 * nranks <= 80 * 1024:
            return f"k_bucket_scatter_staged<{L}B,own>"
        return f"k_bucket_scatter_staged<{L}B>"
    return wg


# ------------------------------------------------------------ distributions ---
DISTRIBUTIONS = ("one_rank_first", "one_rank_last", "fine_last", "fine_first", "coarse_first", "coarse_last",
                 "ascending", "descending", "round_robin", "strided", "tile_alternating", "hot", "zipf")


def fine_digit(name, L, nranks, records):
    """f0 of "fine_last" / "fine_first": F - 1 and 0 (below F ranks the last fine digit that exists)."""
    _, F, _ = digits(L, nranks, records)
    return min(F, nranks) - 1 if name == "fine_last" else 0


def hot_rank(nranks):
    return nranks // 3


def alternating_pair(nranks):
    """(a, b) of "tile_alternating": ranks 1 and nranks - 2."""
    return 1, nranks - 2


def rank_sequence(name, n, L, nranks, records, seed=0):
    """The n requested ranks of distribution `name` (int64)."""
    rng = np.random.default_rng(seed)
    _, F, C = digits(L, nranks, records)
    i = np.arange(n, dtype=np.int64)
    if name == "one_rank_first":
        return np.zeros(n, np.int64)
    if name == "one_rank_last":
        return np.full(n, nranks - 1, np.int64)
    if name in ("fine_last", "fine_first"):
        cand = np.arange(fine_digit(name, L, nranks, records), nranks, F)
        return cand[rng.integers(0, cand.size, n)]
    if name in ("coarse_first", "coarse_last"):
        c0 = 0 if name == "coarse_first" else C - 1
        return rng.integers(c0 * F, min((c0 + 1) * F, nranks), n)
    if name == "ascending":
        return np.sort(rng.integers(0, nranks, n))
    if name == "descending":
        return np.sort(rng.integers(0, nranks, n))[::-1].copy()
    if name == "round_robin":
        return i % nranks
    if name == "strided":
        return (i * 257) % nranks
    if name == "tile_alternating":
        a, b = alternating_pair(nranks)
        return np.where((i // TILE) % 2 == 0, a, b)
    if name == "hot":
        return np.where(rng.random(n) < 0.9, hot_rank(nranks), rng.integers(0, nranks, n))
    if name == "zipf":
        p = 1.0 / np.arange(1, nranks + 1)
        return rng.permutation(nranks)[rng.choice(nranks, n, p=p / p.sum())]
    raise ValueError(name)


def exact_fine_sequence(n, m, f0, L, nranks, records, seed=0):
    """Exactly m of n ranks have fine digit f0, spread over its coarse digits
    and over the batch; the others are uniform over the other fine buckets."""
    rng = np.random.default_rng(seed)
    _, F, _ = digits(L, nranks, records)
    all_r = np.arange(nranks)
    inside, outside = all_r[all_r % F == f0], all_r[all_r % F != f0]
    ranks = outside[rng.integers(0, outside.size, n)]
    ranks[rng.permutation(n)[:m]] = inside[rng.integers(0, inside.size, m)]
    return ranks


# ----------------------------------------------------------------- checkers ---
def reference(k, nptes, nranks):
    """(mbits, ptindex, rank, stable bucket order, bucket offsets) of the batch k, from the oracle."""
    k = np.ascontiguousarray(k)
    if k.shape[0]:
        m, p, r = _oracle().pdht_hash_fixed(k, nptes, nranks)
    else:
        m, p, r = np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    order = np.argsort(r, kind="stable")
    offs = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=nranks))])
    return m, p, r, order, offs


def _np(t):
    return t.cpu().numpy()


def check_arrays(k, nptes, nranks, got, ref=None):
    """bucket_batch's (keys | None, mbits, ptindex | None, index | None, offsets) of the batch k: the
    assertions of test_gpu_parity.py's test_bucket_batch.  `ref` = reference(k, nptes, nranks), if at hand."""
    m, p, r, order, offs = ref if ref is not None else reference(k, nptes, nranks)
    ko, mb, pt, ix, of = got
    assert (_np(of) == offs).all()
    assert (_np(mb).view(np.uint64) == m[order]).all()
    if ix is not None:
        assert _np(ix).dtype == np.int32
        assert (_np(ix).view(np.uint32) == order).all()
    if pt is not None:
        assert (_np(pt).view(np.uint32) == p[order]).all()
    if ko is not None:
        assert (_np(ko) == k[order]).all()


def check_records(k, nranks, rec, got_offs, msg_type=1, src_rank=0, ht_index=0, ref=None):
    """bucket_records' (records [n, 24 + L rounded up to 8], offsets) of the batch k: the assertions of
    test_bucket_records.  `ref` = reference(k, any nptes, nranks), if at hand."""
    m, _, r, order, offs = ref if ref is not None else reference(k, 1, nranks)
    n, L = k.shape
    assert tuple(rec.shape) == (n, 24 + (L + 7) // 8 * 8)
    assert (_np(got_offs) == offs).all()
    if n == 0:
        return
    R = _np(rec)
    w32 = R[:, :16].copy().view(np.uint32)
    assert (w32[:, 0] == msg_type).all() and (w32[:, 1] == src_rank).all() and (w32[:, 2] == ht_index).all()
    assert (w32[:, 3] == order).all()
    assert (R[:, 16:24].copy().view(np.uint64).ravel() == m[order]).all()
    assert (R[:, 24:24 + L] == k[order]).all()
    assert (R[:, 24 + L:] == 0).all()
