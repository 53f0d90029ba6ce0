"""The 64-B kernel's round-blocked dispatch on the GPU: batches at the edges of
a round and of a workgroup's R rounds against the oracle, one big call against
the same keys hashed in slices of at most one round (which take the
persistent shape), the seeded entry, the histogram path (persistent), output
views, and the tuning build's R / occupancy variants.  G (tiles per round) and
R come from the plan of the device at hand (pdht_amd.xpose64_plan)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

pytestmark = pytest.mark.gpu
M = 1 << 20
DELTAS = (-65, -64, -1, 0, 1, 63, 64, 65)
TAG = "k_fixed_xpose64<nt,d2>@3"
# tuning build: rounds per workgroup of variants 350-360 (pdht_hip_tuning.h)
VARIANT_R = {350: 1, 351: 2, 352: 4, 353: 8, 354: 16, 355: 1, 356: 2, 357: 4, 358: 1, 359: 2, 360: 4}
VARIANT_TAG = {**{v: TAG for v in range(350, 355)}, **{v: "k_fixed_xpose64<nt,d2>@4" for v in range(355, 358)},
               **{v: "k_fixed_xpose64<nt,d2>@unpadded" for v in range(358, 361)}}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def shape(dev):
    """(R, keys per round) of the product's plan on this device."""
    p = P.xpose64_plan(1 << 30)
    assert p.round_blocked and p.rounds_per_wg >= 1, "the product takes the round-blocked shape for big batches"
    return p.rounds_per_wg, 2 * p.waves * 64


@pytest.fixture(scope="module")
def ref(dev, shape, oracle):
    """Keys of the largest batch used here and their reference digests, once:
    every case hashes a prefix."""
    R, gk = shape
    n = (2 * R + 1) * gk + 77
    k = oracle.fixed_keys(n, 64)
    return {"n": n, "k": k, "kd": torch.from_numpy(k).to(dev), "c64": oracle.city64_fixed(k),
            "crc": oracle.city128_fixed(k[:(R + 1) * gk + 65], crc=True).reshape(-1, 2)}


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def rounds_of(n, gk):
    return -(-((n + 63) // 64) // (gk // 64))


@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("kk", ["1", "R", "R+1"])
def test_boundary_sizes_against_oracle(dev, shape, ref, oracle, kk, delta):
    """n = k G 64 + delta: the last round holding only d = 0 tiles or one key,
    a ragged last tile, a last workgroup row cut short."""
    R, gk = shape
    n = {"1": 1, "R": R, "R+1": R + 1}[kk] * gk + delta
    p = P.xpose64_plan(n)
    assert p.round_blocked == (1 if rounds_of(n, gk) > R else 0)
    if kk == "R+1" or (kk == "R" and delta > 0):
        assert p.round_blocked and p.launches == 1
    kd = ref["kd"][:n]
    got = u64(P.city64_batch(kd))
    assert P.last_kernel() == TAG
    assert (got == ref["c64"][:n]).all()
    got = u64(P.citycrc128_batch(kd)).reshape(-1, 2)
    assert P.last_kernel() == TAG
    assert (got == ref["crc"][:n]).all()


def test_one_launch_equals_slices_of_one_round(dev, shape, ref):
    """(2R+1) rounds and a ragged tail as one call against the same keys in
    slices of one round each (the persistent shape)."""
    R, gk = shape
    n, kd = ref["n"], ref["kd"]
    assert P.xpose64_plan(n).round_blocked and not P.xpose64_plan(gk).round_blocked
    for fn, w in ((P.city64_batch, 1), (P.citycrc128_batch, 2)):
        whole = fn(kd)
        parts = torch.cat([fn(kd[a:a + gk]) for a in range(0, n, gk)])
        assert whole.numel() == n * w and torch.equal(whole.reshape(-1), parts.reshape(-1))
    assert (u64(P.city64_batch(kd)) == ref["c64"]).all()


def test_seeded_entry(dev, shape, ref, oracle):
    R, gk = shape
    n = (R + 1) * gk + 65
    assert P.xpose64_plan(n).round_blocked
    s0, s1 = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    kd = ref["kd"][:n]
    whole = P.city64_seeds_batch(kd, s0, s1)
    assert P.last_kernel() == TAG
    parts = torch.cat([P.city64_seeds_batch(kd[a:a + gk], s0, s1) for a in range(0, n, gk)])
    assert torch.equal(whole, parts)
    got = u64(whole)
    for i in list(range(3)) + [gk - 1, gk, R * gk - 1, R * gk, R * gk + 63, n - 66, n - 65, n - 1]:
        assert int(got[i]) == oracle.city64_seeds(ref["k"][i].tobytes(), s0, s1), i


def test_histogram_path_stays_persistent(dev, shape, ref, oracle):
    R, gk = shape
    n = (R + 1) * gk + 65
    assert P.xpose64_plan(n).round_blocked and not P.xpose64_plan(n, hist=True).round_blocked
    hist = torch.zeros(1000, dtype=torch.int64, device=dev)
    mb, pt, rk = P.place_batch(ref["kd"][:n], 7, 1000, hist=hist)
    assert P.last_kernel() in ("k_fixed_xpose64<nt,d2,1024>@1", TAG)
    m2, p2, r2 = oracle.pdht_hash_fixed(ref["k"][:n], 7, 1000)
    assert (u64(mb) == m2).all() and (pt.cpu().numpy().view(np.uint32) == p2).all()
    assert (rk.cpu().numpy().view(np.uint32) == r2).all()
    assert (hist.cpu().numpy() == np.bincount(r2, minlength=1000)).all()
    # the same call without a histogram takes the round-blocked shape: same placement
    mb2, pt2, rk2 = P.place_batch(ref["kd"][:n], 7, 1000)
    assert P.last_kernel() == TAG
    assert torch.equal(mb, mb2) and torch.equal(pt, pt2) and torch.equal(rk, rk2)


def test_output_views(dev, shape, ref):
    """Digests written into the middle of a larger tensor: nothing before or
    after the view is touched."""
    R, gk = shape
    n = (R + 1) * gk + 1
    pad = 1029
    for fn, w, want in ((P.city64_batch, 1, ref["c64"][:n]), (P.citycrc128_batch, 2, None)):
        big = torch.full((n + 2 * pad, w), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
        view = big[pad:pad + n]
        fn(ref["kd"][:n], out=view.view(n) if w == 1 else view)
        assert bool((big[:pad] == -0x5A5A5A5A5A5A5A5B).all()) and bool((big[pad + n:] == -0x5A5A5A5A5A5A5A5B).all())
        assert torch.equal(view.reshape(-1), fn(ref["kd"][:n]).reshape(-1))
        if want is not None:
            assert (u64(view.reshape(-1)) == want).all()


@pytest.mark.tuning
@pytest.mark.parametrize("variant", sorted(VARIANT_R))
def test_round_blocked_variants_bitexact(dev, shape, ref, variant):
    """Tuning 350-360: every R and occupancy cap, at M + 13 keys against the
    oracle and at the edge of its own R + 1 rounds (keys generated on the
    device) against the same keys in slices of one round."""
    _, gk = shape
    R = VARIANT_R[variant]
    n = M + 13
    with P.tuning(variant):
        p = P.xpose64_plan(n)
        got = u64(P.city64_batch(ref["kd"][:n]))
        kern = P.last_kernel()
    assert p.rounds_per_wg == (R if p.round_blocked else 0) and p.round_blocked == (rounds_of(n, gk) > R)
    assert kern == (VARIANT_TAG[variant] if p.round_blocked else TAG)
    assert (got == ref["c64"][:n]).all()
    n = (R + 1) * gk + 65
    kd = P.splitmix64_fill(0x5EED5EED5EED5EED, 0, n * 8, device=dev).view(torch.uint8).view(n, 64)
    for fn in (P.city64_batch, P.citycrc128_batch):
        with P.tuning(variant):
            assert P.xpose64_plan(n).round_blocked
            whole = fn(kd)
            assert P.last_kernel() == VARIANT_TAG[variant]
        parts = torch.cat([fn(kd[a:a + gk]) for a in range(0, n, gk)])
        assert torch.equal(whole.reshape(-1), parts.reshape(-1))


@pytest.mark.tuning
def test_persistent_variant(dev, ref):
    with P.tuning(361):  # the persistent grid in 512 MiB launches
        assert not P.xpose64_plan(1 << 30).round_blocked
        assert (u64(P.city64_batch(ref["kd"])) == ref["c64"]).all()
        assert P.last_kernel() == TAG
