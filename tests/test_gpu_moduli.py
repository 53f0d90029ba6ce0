"""The moduli of placement and bucketing at chosen dividends.

Every rank and every ptindex is a FastMod remainder (Granlund-Montgomery,
kernels.h; magic number and shift from make_fastmod, pdht_hip.hip).  Through
the hash kernels the dividends are CityHash64 digests: with a divisor near
2^31 a digest is a multiple of it once in 2^31 keys, so a magic number off by
one, or a shift wrong for one ceil(log2 d), passes every test that hashes.
pdht_hip_mod_dev runs the same FastMod object over dividends of the caller's
choice: the grid of test_key_length_cases_cpu.py (multiples of the divisor
and their neighbours at the largest quotients) against Python integers; then
the edge divisors once more through place_batch and bucket_batch against the
oracle."""
import numpy as np
import pytest

import bucket_ref as B
import test_key_length_cases_cpu as KC

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_fastmod_on_the_adversarial_grid(dev):
    """Every (divisor, dividend) of the grid: one values tensor, one output tensor, one launch per divisor,
    one comparison."""
    grid = KC.moduli_grid()
    values = np.array([n for _, ns in grid for n in ns], dtype=np.uint64)
    want = np.array([n % d for d, ns in grid for n in ns], dtype=np.uint64)
    vd = to_dev(values.view(np.int64), dev)
    out = torch.full((values.size,), -1, dtype=torch.int32, device=dev)
    at = 0
    for d, ns in grid:
        got = P.mod_batch(vd[at:at + len(ns)], d, out=out[at:at + len(ns)])
        assert got.data_ptr() == out[at:at + len(ns)].data_ptr()
        at += len(ns)
    assert P.last_kernel() == "k_fastmod" and at == values.size
    got = out.cpu().numpy().view(np.uint32).astype(np.uint64)
    bad = np.flatnonzero(got != want)
    ds = np.repeat([d for d, _ in grid], [len(ns) for _, ns in grid])
    print(f"{len(grid)} divisors, {values.size} pairs, {bad.size} mismatches")
    assert bad.size == 0, [(int(ds[i]), int(values[i]), int(got[i]), int(want[i])) for i in bad[:8]]


def test_fastmod_grid_stride(dev):
    """More values than the grid has threads (8 workgroups per CU): every index once, none past n."""
    n = (1 << 21) + 4097
    v = P.splitmix64_fill(0x5EED, 0, n, device=dev)
    out = torch.full((n + 64,), -1, dtype=torch.int32, device=dev)
    for d in (0xFFFFFFFB, 0x80000000, 1):
        P.mod_batch(v, d, out=out[:n])
        got = out.cpu().numpy()
        assert (got[n:] == -1).all()
        assert (got[:n].view(np.uint32) == v.cpu().numpy().view(np.uint64) % np.uint64(d)).all(), d


def test_mod_batch_refuses_bad_arguments(dev):
    v = torch.zeros(8, dtype=torch.int64, device=dev)
    out = torch.zeros(8, dtype=torch.int32, device=dev)
    lib = P.lib()
    s = torch.cuda.current_stream(dev).cuda_stream
    assert lib.pdht_hip_mod_dev(v.data_ptr(), 8, 0, out.data_ptr(), s) != 0
    assert b"divisor" in lib.pdht_hip_last_error()
    assert lib.pdht_hip_mod_dev(None, 8, 3, out.data_ptr(), s) != 0
    assert b"null" in lib.pdht_hip_last_error()
    assert lib.pdht_hip_mod_dev(v.data_ptr(), 8, 3, None, s) != 0
    assert lib.pdht_hip_mod_dev(None, 0, 3, None, s) == 0  # nothing to do
    for d in (0, 1 << 32, -1):
        with pytest.raises(ValueError, match="divisor"):
            P.mod_batch(v, d)
    with pytest.raises(ValueError):
        P.mod_batch(v, 3, out=torch.zeros(7, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        P.mod_batch(v.to(torch.int32), 3)
    torch.cuda.synchronize()
    assert (out == 0).all()  # nothing ran
    assert P.mod_batch(v[:0], 3).numel() == 0


# ------------------------------------------------- through the real kernels ---
@pytest.fixture(scope="module")
def keys8(dev):
    k = np.random.default_rng(0xED6E).integers(0, 256, (KC.MODULI_N, 8), dtype=np.uint8)
    return k, to_dev(k, dev)


def test_place_batch_at_the_modulus_edges(dev, oracle, keys8):
    """(nptes, nranks) down the diagonal of 2^k - 1 | 2^k | 2^k + 1, k = 1..32, and the same for j = 1..31."""
    k, kd = keys8
    out = None
    for nptes, nranks in KC.PLACE_MODULI:
        out = P.place_batch(kd, nptes, nranks, out=out)
        mb, pt, rk = out
        m2, p2, r2 = oracle.pdht_hash_fixed(k, nptes, nranks)
        assert (mb.cpu().numpy().view(np.uint64) == m2).all()
        assert (pt.cpu().numpy().view(np.uint32) == p2).all(), ("nptes", nptes)
        assert (rk.cpu().numpy().view(np.uint32) == r2).all(), ("nranks", nranks)
        assert (m2 % np.uint64(nptes) == p2).all() and (m2 % np.uint64(nranks) == r2).all()


@pytest.mark.parametrize("L", [8, 13])
def test_bucket_batch_at_the_nptes_edges(dev, oracle, keys8, L):
    """OutSoA's own FastMod (ptindex at the bucketed positions), on the staged and on the generic kernel."""
    cases = [c for c in KC.MODULI_BUCKET if c[0] == L]
    assert len(cases) == len(KC.NPTES_EDGES)
    if L == 8:
        k, kd = keys8
    else:
        k = np.random.default_rng(0xED6E + L).integers(0, 256, (KC.MODULI_N, L), dtype=np.uint8)
        kd = to_dev(k, dev)
    out, ws = None, torch.empty(P.bucket_workspace_bytes(KC.MODULI_N, L, 7), dtype=torch.uint8, device=dev)
    for _, nranks, nptes in cases:
        out = P.bucket_batch(kd, nptes, nranks, out=out, workspace=ws)
        assert P.last_kernel() == B._bucket_kernel(L, nranks, 0)
        B.check_arrays(k, nptes, nranks, out)
