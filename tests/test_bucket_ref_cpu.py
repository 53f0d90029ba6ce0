"""bucket_ref.py proved on the CPU: the keys it hands out hash to the ranks
asked for, its digit split is the library's, and every rank distribution of
test_gpu_bucket_skew.py has the property that names it -- each asserted on the
oracle's ranks of the keys, never on the ranks requested."""
import numpy as np
import pytest

import bucket_ref as B

N = 70001


def oracle_ranks(oracle, ranks, L, nranks, seed=1):
    k = B.keys_with_ranks(ranks, L, nranks, seed)
    assert k.dtype == np.uint8 and k.shape == (len(ranks), L)
    return oracle.pdht_hash_fixed(k, 1, nranks)[2].astype(np.int64)


@pytest.mark.parametrize("L,nranks", [(8, 7), (8, 8192), (13, 1000), (13, 4097), (16, 1574), (32, 2049), (32, 8192)])
def test_keys_have_the_requested_ranks(oracle, L, nranks):
    want = np.random.default_rng(L + nranks).integers(0, nranks, 50_000)
    want[:nranks] = np.arange(nranks)  # every rank at least once
    assert (oracle_ranks(oracle, want, L, nranks) == want).all()
    # another seed: other keys, the same ranks
    a, b = B.keys_with_ranks(want, L, nranks, 1), B.keys_with_ranks(want, L, nranks, 2)
    assert (a != b).any() and (oracle.pdht_hash_fixed(b, 1, nranks)[2] == want).all()
    assert B.keys_with_ranks(np.zeros(0, np.int64), L, nranks, 0).shape == (0, L)


@pytest.mark.parametrize("L,records,nranks,want", [
    (8, False, 8192, (8, 256, 32)), (32, False, 8192, (7, 128, 64)), (8, True, 8192, (7, 128, 64)),
    (8, False, 2049, (7, 128, 17)), (32, False, 2049, (6, 64, 33)), (8, False, 2, (1, 2, 1)),
    (16, False, 8192, (8, 256, 32)), (16, True, 2049, (6, 64, 33)), (8, False, 7, (3, 8, 1)),
    (32, True, 1000, (5, 32, 32))])
def test_digits(L, records, nranks, want):
    assert B.digits(L, nranks, records) == want


def test_bucket_kernel_names():
    """The expected-kernel function at the thresholds the skew tests straddle."""
    k = B._bucket_kernel
    assert k(8, 1574, 0) == "k_bucket_scatter_staged<8B,own,8x16>" and k(8, 2049, 0) == "k_bucket_tl_pass2<8B>"
    assert k(32, 1574, 0) == "k_bucket_scatter_staged<32B>" and k(32, 1000, 0) == "k_bucket_scatter_staged<32B,own>"
    assert k(8, 7, 0) == k(8, 7, 0, records=True) == "k_bucket_scatter_staged<8B>"
    # records rank by owner tables on 4 x 16 tiles from 512 ranks while 40960 + 28 B per rank fit 80 KiB
    assert k(8, 1000, 0, records=True) == "k_bucket_scatter_staged<8B,own>"
    assert k(8, 1574, 0, records=True) == "k_bucket_scatter_staged<8B>"
    assert k(16, 1574, 0, records=True) == "k_bucket_tl_pass2<16B>" and k(32, 1000, 0, records=True) == "k_bucket_tl_pass2<32B>"
    assert k(13, 1000, 0) == "k_bucket_scatter_wg<8>" and k(13, 4097, 0, records=True) == "k_bucket_scatter_wg<4>"


def test_records_kernel_agrees_with_the_put_tests():
    """test_gpu_put.py keeps its own statement of the records' kernel choice: the two agree."""
    from test_gpu_put import _bucket_kernel as put_kernel
    for L in (8, 13, 16, 32, 64):
        for nranks in (1, 7, 255, 256, 511, 512, 1000, 1462, 1463, 1574, 2047, 2048, 2049, 4096, 4097, 8192):
            assert B._bucket_kernel(L, nranks, 0, records=True) == put_kernel(L, nranks), (L, nranks)


@pytest.mark.parametrize("records", [False, True])
@pytest.mark.parametrize("L,nranks", [(8, 7), (8, 2049), (16, 1574), (32, 8192), (13, 1000)])
def test_distributions_have_their_property(oracle, L, nranks, records):
    _, F, C = B.digits(L, nranks, records)
    r = {name: oracle_ranks(oracle, B.rank_sequence(name, N, L, nranks, records), L, nranks)
         for name in B.DISTRIBUTIONS}
    assert (r["one_rank_first"] == 0).all() and (r["one_rank_last"] == nranks - 1).all()
    for name in ("fine_last", "fine_first"):
        f0 = B.fine_digit(name, L, nranks, records)
        assert (r[name] % F == f0).all()
        # ... and all of that fine bucket's coarse digits occur
        assert len(np.unique(r[name])) == len(range(f0, nranks, F))
    assert B.fine_digit("fine_last", L, nranks, records) == min(F, nranks) - 1
    assert (r["coarse_first"] // F == 0).all() and (r["coarse_last"] // F == C - 1).all()
    assert len(np.unique(r["coarse_first"])) == min(F, nranks)
    assert len(np.unique(r["coarse_last"])) == nranks - (C - 1) * F
    assert (np.diff(r["ascending"]) >= 0).all() and (np.diff(r["descending"]) <= 0).all()
    assert len(np.unique(r["ascending"])) > min(nranks, 1000) * 0.9  # many buckets: boundaries inside tiles
    i = np.arange(N)
    assert (r["round_robin"] == i % nranks).all() and (r["strided"] == i * 257 % nranks).all()
    for t in range(0, N, B.TILE):  # every tile holds equal counts, give or take the ragged end
        c = np.bincount(r["round_robin"][t:t + B.TILE], minlength=nranks)
        assert c.max() - c.min() <= 1
    a, b = B.alternating_pair(nranks)
    assert (a, b) == ((1, 5) if nranks == 7 else (1, nranks - 2))
    assert (r["tile_alternating"] == np.where(i // 2048 % 2 == 0, a, b)).all()
    hot = np.bincount(r["hot"], minlength=nranks)
    assert hot.argmax() == B.hot_rank(nranks) and 0.89 * N < hot.max() < 0.91 * N + N / nranks
    assert (hot > 0).sum() > min(nranks, 1000) * 0.5  # the rest is spread out
    z = np.sort(np.bincount(r["zipf"], minlength=nranks))[::-1]
    h = (1.0 / np.arange(1, nranks + 1)).sum()
    assert abs(z[0] - N / h) < 5 * np.sqrt(N / h) and abs(z[1] - N / (2 * h)) < 5 * np.sqrt(N / (2 * h))


def test_ragged_last_coarse_bucket():
    """2049 ranks: rank 2048 is alone in the last coarse bucket under both digit splits; 8192: a full one."""
    for records in (False, True):
        assert (B.rank_sequence("coarse_last", 100, 8, 2049, records) == 2048).all()
        _, F, _ = B.digits(8, 8192, records)
        assert set(B.rank_sequence("coarse_last", 20000, 8, 8192, records)) == set(range(8192 - F, 8192))


@pytest.mark.parametrize("m", [1023, 1024, 1025, 4097, 8193])
@pytest.mark.parametrize("L,nranks,records", [(8, 8192, False), (32, 2049, False), (16, 1574, True)])
def test_exact_fine_sequence(oracle, L, nranks, records, m):
    _, F, _ = B.digits(L, nranks, records)
    r = oracle_ranks(oracle, B.exact_fine_sequence(20000, m, 0, L, nranks, records, seed=m), L, nranks)
    assert ((r % F) == 0).sum() == m
    assert len(np.unique(r[r % F == 0])) > 1  # spread over the coarse digits
    assert len(np.unique(r % F)) == F  # the rest reaches every other fine bucket


def test_checkers_catch_a_wrong_order(oracle):
    """The checkers accept the reference's own outputs and refuse a swap of two rows."""
    class T:  # the little of a tensor that the checkers use
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return self

        def numpy(self):
            return self.a

        @property
        def shape(self):
            return self.a.shape

    L, nranks = 13, 7
    k = B.keys_with_ranks(B.rank_sequence("round_robin", 500, L, nranks, False), L, nranks, 3)
    m, p, r, order, offs = B.reference(k, 3, nranks)
    good = (k[order], m[order].view(np.int64), p[order].view(np.int32), order.astype(np.uint32).view(np.int32), offs)
    B.check_arrays(k, 3, nranks, tuple(T(x) for x in good))
    rec = np.zeros((500, 40), np.uint8)
    rec[:, 0:4] = np.array([1], np.uint32).view(np.uint8)
    rec[:, 4:8] = np.array([5], np.uint32).view(np.uint8)
    rec[:, 12:16] = order.astype(np.uint32).view(np.uint8).reshape(-1, 4)
    rec[:, 16:24] = m[order].view(np.uint8).reshape(-1, 8)
    rec[:, 24:24 + L] = k[order]
    B.check_records(k, nranks, T(rec), T(offs), src_rank=5)
    swapped = order.copy()
    swapped[[3, 4]] = swapped[[4, 3]]  # same bucket, unstable order
    assert r[order[3]] == r[order[4]]
    with pytest.raises(AssertionError):
        B.check_arrays(k, 3, nranks, tuple(T(x) for x in good[:3] + (swapped.astype(np.uint32).view(np.int32), offs)))
    rec[0, 39] = 1  # a pad byte
    with pytest.raises(AssertionError):
        B.check_records(k, nranks, T(rec), T(offs), src_rank=5)
