"""Destination bucketing on rank distributions that are not uniform.

Every other bucketing test draws uniformly random keys.  Here the keys are
picked so that their ranks follow a chosen sequence (bucket_ref.py): whole
batches in one rank, one fine or one coarse bucket of the two-pass sort,
batches already in bucket order or in reverse, exactly equal counts per tile,
tiles that alternate between two ranks, a hot rank, a Zipf law -- on the
ballot, both owner-table, the two-pass and both generic-length kernels, for
arrays and for wire records.  Byte-exact against the oracle's stable order of
the batch actually sent; the kernel that ran is asserted in every case."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import bucket_ref as B  # noqa: E402
import pdht_amd as P  # noqa: E402

pytestmark = pytest.mark.gpu

N = 70001  # several tiles of every kernel, a ragged last one, one count-chunk per tile
# the ballot shape (7), both owner-table shapes (1000; 1574), both sides of every one-pass / two-pass
# threshold of the key sizes (1574 | 2049 for arrays, 1000 | 1574 | 2049 for records), digits that are no
# power of two (1574, 2049) and the LDS digit bound (8192); 13-B keys: the generic kernel in 8 and in 4 waves
CONFIGS = [(L, nr) for L in (8, 16, 32) for nr in (7, 1000, 1574, 2049, 8192)] + [(13, 1000), (13, 4097)]
KINDS = ("arrays", "records")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def two_pass(L, nranks, kind):
    return B._bucket_kernel(L, nranks, 0, kind == "records").startswith("k_bucket_tl_pass2")


_LAST = {}


def batch(key, make_ranks, L, nranks):
    """Keys of the requested ranks and their reference, made once per `key` and shared by the arrays and the
    records case that follow each other (the latest only: a 2M-key reference is ~100 MB)."""
    if _LAST.get("key") != key:
        _LAST.clear()
        k = B.keys_with_ranks(make_ranks(), L, nranks, seed=7)
        _LAST.update(key=key, k=k, ref=B.reference(k, 3, nranks))
    return _LAST["k"], _LAST["ref"]


def run_and_check(dev, kind, k, ref, L, nranks):
    kd = to_dev(k, dev)
    if kind == "arrays":
        got = P.bucket_batch(kd, 3, nranks)
        assert P.last_kernel() == B._bucket_kernel(L, nranks, 0)
        B.check_arrays(k, 3, nranks, got, ref)
    else:
        rec, offs = P.bucket_records(kd, nranks, src_rank=5, ht_index=3)
        assert P.last_kernel() == B._bucket_kernel(L, nranks, 0, records=True)
        B.check_records(k, nranks, rec, offs, P.PDHT_PUT, 5, 3, ref)


@pytest.mark.parametrize("L,nranks,dist,kind", [(L, nr, d, kind) for (L, nr) in CONFIGS for d in B.DISTRIBUTIONS
                                                for kind in KINDS])
def test_bucket_distributions(dev, L, nranks, dist, kind):
    """The thirteen rank sequences of bucket_ref.DISTRIBUTIONS.  The two digit splits differ between arrays
    and records (digits()), so "one fine bucket" and "one coarse bucket" are built per output kind; the
    other sequences are shared by both."""
    records = kind == "records"
    per_kind = dist.startswith(("fine_", "coarse_")) and B.digits(L, nranks, False) != B.digits(L, nranks, True)
    k, ref = batch((L, nranks, dist, records if per_kind else None),
                   lambda: B.rank_sequence(dist, N, L, nranks, records, seed=L + nranks), L, nranks)
    run_and_check(dev, kind, k, ref, L, nranks)


@pytest.mark.parametrize("L,nranks", [(L, nr) for L in (8, 16, 32) for nr in (1000, 8192)])
def test_bucket_records_few_distinct_keys(dev, L, nranks):
    """test_gpu_parity.py's test_bucket_skewed (three distinct keys, 700 001 of them) on wire records."""
    rng = np.random.default_rng(L + nranks)
    k = rng.integers(0, 256, (3, L), dtype=np.uint8)[rng.integers(0, 3, 700_001)]
    run_and_check(dev, "records", k, B.reference(k, 3, nranks), L, nranks)


# pass 2's sub-tile is 1024 (32-B records), 2048 (16-B keys, 32-B arrays, 8-B records) or 4096 keys (8-B
# arrays): each at one less, exactly and one more, and two sub-tiles plus one
EDGE_M = (1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8193)
EDGE_CONFIGS = [(L, nr, kind) for kind in KINDS for L in (8, 16, 32) for nr in (1000, 1574, 2049, 8192)
                if two_pass(L, nr, kind)]


def test_edge_configs_are_the_two_pass_ones():
    assert len(EDGE_CONFIGS) == 6 + 2 + 3 + 4
    assert all(nr >= 2049 for (L, nr, kind) in EDGE_CONFIGS if kind == "arrays")
    assert {nr for (L, nr, kind) in EDGE_CONFIGS if kind == "records" and L == 32} == {1000, 1574, 2049, 8192}


@pytest.mark.parametrize("m", EDGE_M)
@pytest.mark.parametrize("L,nranks,kind", EDGE_CONFIGS)
def test_bucket_exact_subtile_edges(dev, L, nranks, kind, m):
    """20 000 keys (one pass-2 segment per fine bucket), exactly m of them in fine bucket 0, spread over its
    coarse digits -- at 2049 ranks the ragged last coarse bucket among them -- and the rest uniform over
    the other fine buckets: the segment of fine bucket 0 is exactly m keys long."""
    records = kind == "records"
    ranks = B.exact_fine_sequence(20000, m, 0, L, nranks, records, seed=m + nranks)
    k = B.keys_with_ranks(ranks, L, nranks, seed=m)
    ref = B.reference(k, 3, nranks)
    _, F, _ = B.digits(L, nranks, records)
    assert (ref[2] % F == 0).sum() == m
    run_and_check(dev, kind, k, ref, L, nranks)


@pytest.mark.parametrize("L,nranks,dist,kind", [(L, nr, d, kind) for nr in (2049, 8192) for L in (8, 32)
                                                for d in ("fine_last", "fine_first", "ascending", "hot")
                                                for kind in KINDS])
def test_bucket_several_segments_per_fine_bucket(dev, L, nranks, dist, kind):
    """Batches large enough that pass 2 splits every fine bucket into several segments of count-chunks
    (about 480 chunks per segment at F = 256): a wrong chunk prefix at a segment's first chunk,
    running[c] = base + chunkcnt[g0][r], would show here, on the distributions that fill or empty whole
    segments."""
    records = kind == "records"
    n = ((2 << 20) if nranks == 8192 else (1 << 20)) + 100_003
    per_kind = dist.startswith("fine_") and B.digits(L, nranks, False) != B.digits(L, nranks, True)
    k, ref = batch((L, nranks, dist, n, records if per_kind else None),
                   lambda: B.rank_sequence(dist, n, L, nranks, records, seed=L + nranks + 1), L, nranks)
    run_and_check(dev, kind, k, ref, L, nranks)


@pytest.mark.parametrize("parity", [0, 1])
def test_bucket_chunk_histogram_at_its_limit(dev, parity):
    """Pass 1 keeps a count-chunk's rank histogram as u16 halves of u32 words in LDS; the launcher sizes a
    chunk at 32768 keys at most (ct = 8 tiles of 4096 from 16M 8-B keys up).  Here every key of 16M + 4097
    is the same key, so each full chunk counts 32768 in one half -- the low half for an even rank, the high
    one for an odd rank.  This is the suite's only case that fills a chunk with one rank.  The reference
    needs no sort (index = 0..n-1, one step in the offsets, constant mbits) and is compared on the device;
    only the offsets are copied back."""
    L, nranks, n = 8, 8192, (16 << 20) + 4097
    want_rank = 4096 + 2 * 77 + parity
    k1 = B.keys_with_ranks([want_rank], L, nranks, seed=parity)
    m, p, r, _, _ = B.reference(k1, 3, nranks)
    rank = int(r[0])
    assert rank == want_rank and rank % 2 == parity
    kd = to_dev(k1, dev).expand(n, L).contiguous()
    ko, mb, pt, ix, offs = P.bucket_batch(kd, 3, nranks)
    assert P.last_kernel() == "k_bucket_tl_pass2<8B>"
    assert torch.equal(ix, torch.arange(n, dtype=torch.int32, device=dev))
    assert torch.equal(mb, torch.full((n,), int(m.view(np.int64)[0]), dtype=torch.int64, device=dev))
    assert torch.equal(pt, torch.full((n,), int(p[0]), dtype=torch.int32, device=dev))
    assert torch.equal(ko, kd)
    want = np.where(np.arange(nranks + 1) > rank, n, 0)
    assert (offs.cpu().numpy() == want).all()
