"""GPU checks of put records and the row movers (include/pdht_hip_put.h),
bit-exact against numpy.  The expected bucket order is
np.argsort(rank, kind="stable") of oracle.pdht_hash_fixed, as in
test_gpu_parity.py's test_bucket_records."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

pytestmark = pytest.mark.gpu

ROWBYTES = (1, 3, 4, 8, 12, 16, 24, 40, 64, 72, 136, 256, 1000, 4096)
MS = (0, 1, 63, 65, 4097)
GRID = [(B, m) for B in ROWBYTES for m in MS] + [(B, 100003) for B in ROWBYTES if B <= 64]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def piece_of(*parts):
    """The widest of 16 / 8 / 4 / 1 bytes that divides every length, stride and address given."""
    bits = 0
    for p in parts:
        bits |= int(p)
    return 16 if bits % 16 == 0 else 8 if bits % 8 == 0 else 4 if bits % 4 == 0 else 1


def as_index(a, dev):
    return to_dev(np.asarray(a, np.uint32).view(np.int32), dev)


_SRC = {}


def src_rows(rows, B):
    """Random source rows, made once per shape and never written."""
    if (rows, B) not in _SRC:
        _SRC[rows, B] = np.random.default_rng(rows * 131 + B).integers(0, 256, (rows, B), dtype=np.uint8)
    return _SRC[rows, B]


# ------------------------------------------------------------------ gather ---
@pytest.mark.parametrize("B,m", GRID)
def test_gather_rows(dev, B, m):
    rows = max(m, 1) + 5
    x = src_rows(rows, B)
    xd = to_dev(x, dev)
    rng = np.random.default_rng(B * 7 + m)
    for idx in (rng.permutation(rows)[:m], rng.integers(0, rows, m)):  # a permutation; with repeats
        got = P.gather_rows(xd, as_index(idx, dev))
        # torch allocations are 256-B aligned and both strides are B
        assert P.last_kernel() == f"k_rows_gather<{piece_of(B)}>"
        assert tuple(got.shape) == (m, B)
        assert (got.cpu().numpy() == x[idx]).all()


@pytest.mark.parametrize("off", [0, 1, 4])
@pytest.mark.parametrize("pad", [8, 3])
@pytest.mark.parametrize("B,m", [(B, m) for B in ROWBYTES for m in (65, 4097)])
def test_gather_rows_padded_misaligned(dev, B, m, pad, off):
    """Strides of rowbytes + pad and bases off by `off` bytes: the piece width follows, and no byte of dst
    outside its rows is written."""
    rows, S = m + 3, B + pad
    x = src_rows(rows, B)
    sbuf = torch.zeros(rows * S + 16, dtype=torch.uint8, device=dev)
    src = sbuf[off:off + rows * S].view(rows, S)[:, :B]
    src.copy_(to_dev(x, dev))
    dbuf = torch.full((m * S + 16,), 0xA5, dtype=torch.uint8, device=dev)
    dst = dbuf[off:off + m * S].view(m, S)[:, :B]
    idx = np.random.default_rng(B + m + pad).integers(0, rows, m)
    P.gather_rows(src, as_index(idx, dev), out=dst)
    assert P.last_kernel() == f"k_rows_gather<{piece_of(B, S, off)}>"
    d = dbuf.cpu().numpy()
    body = d[off:off + m * S].reshape(m, S)
    assert (body[:, :B] == x[idx]).all()
    assert (body[:, B:] == 0xA5).all() and (d[:off] == 0xA5).all() and (d[off + m * S:] == 0xA5).all()


def test_gather_rows_past_4gib(dev):
    """Row offsets are 64-bit: a source of 2^32 + 2^20 bytes in 4096-B rows (allocated, not filled), 1000
    chosen rows written, the last one among them, and gathered."""
    B = 4096
    rows = ((1 << 32) + (1 << 20)) // B
    src = torch.empty((rows, B), dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(4)
    first_past = (1 << 32) // B  # rows from here on start past 4 GiB
    idx = np.concatenate([rng.choice(first_past, 900, replace=False),
                          first_past + rng.choice(rows - 1 - first_past, 99, replace=False),
                          [rows - 1]]).astype(np.int64)
    assert len(idx) == 1000 and (idx * B >= 1 << 32).sum() == 100
    x = src_rows(1000, B)
    src[to_dev(idx, dev)] = to_dev(x, dev)
    got = P.gather_rows(src, as_index(idx, dev))
    assert P.last_kernel() == "k_rows_gather<16>"
    assert (got.cpu().numpy() == x).all()
    del src, got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("m", [1, 65, 4097])
def test_gather_rows_strided_index_inside_dst(dev, m):
    """The put path's form: the indices are the u32 at +12 of 40-B records, and the rows land at +32 of the same
    records.  Through the C ABI (index_stride = the record stride)."""
    rows, B, S = m + 9, 8, 40
    x = src_rows(rows, B)
    xd = to_dev(x, dev)
    idx = np.random.default_rng(m).integers(0, rows, m)
    rec = np.full((m, S), 0xA5, np.uint8)
    rec[:, 12:16] = idx.astype(np.uint32).view(np.uint8).reshape(m, 4)
    rd = to_dev(rec, dev)
    lib = P.lib()
    s = torch.cuda.current_stream(dev).cuda_stream
    assert lib.pdht_gather_rows_dev(xd.data_ptr(), B, B, rd.data_ptr() + 12, S, m, rd.data_ptr() + 32, S, s) == 0, \
        lib.pdht_hip_last_error()
    assert P.last_kernel() == "k_rows_gather<8>"
    want = rec.copy()
    want[:, 32:40] = x[idx]
    assert (rd.cpu().numpy() == want).all()
    # and through the wrapper: the strided int32 view of the index column is read in place
    w32 = rd.view(-1).view(torch.int32).view(m, S // 4)
    got = P.gather_rows(xd, w32[:, 3])
    assert (got.cpu().numpy() == x[idx]).all()


def test_row_wrappers_refuse_an_index_past_the_rows(dev):
    x = to_dev(src_rows(10, 8), dev)
    with pytest.raises(ValueError, match="past"):
        P.gather_rows(x, as_index([0, 10], dev))
    with pytest.raises(ValueError, match="past"):
        P.scatter_rows(x, as_index(np.arange(1, 11), dev))
    with pytest.raises(ValueError):
        P.gather_rows(x, torch.zeros(3, dtype=torch.int64, device=dev))


# ----------------------------------------------------------------- scatter ---
@pytest.mark.parametrize("B,m", GRID)
def test_scatter_rows(dev, B, m):
    x = src_rows(max(m, 1) + 5, B)[:m]
    xd = to_dev(x, dev)
    p = np.random.default_rng(B * 3 + m).permutation(m)
    pd = as_index(p, dev)
    got = P.scatter_rows(xd, pd)
    assert P.last_kernel() == f"k_rows_scatter<{piece_of(B)}>"
    want = np.empty_like(x)
    want[p] = x
    assert (got.cpu().numpy() == want).all()
    # scatter(gather(x, p), p) == x
    back = P.scatter_rows(P.gather_rows(xd, pd), pd)
    assert (back.cpu().numpy() == x).all()


@pytest.mark.parametrize("pad,off", [(8, 0), (3, 1), (8, 4)])
@pytest.mark.parametrize("B,m", [(B, m) for B in ROWBYTES for m in (65, 4097)])
def test_scatter_rows_padded_dst(dev, B, m, pad, off):
    """A padded destination with more rows than the source: guard bytes and unnamed rows keep their bytes."""
    rows, S = m + 3, B + pad
    x = src_rows(m + 5, B)[:m]
    dbuf = torch.full((rows * S + 16,), 0xA5, dtype=torch.uint8, device=dev)
    dst = dbuf[off:off + rows * S].view(rows, S)[:, :B]
    p = np.random.default_rng(B + m).permutation(rows)[:m]
    P.scatter_rows(to_dev(x, dev), as_index(p, dev), out=dst)
    assert P.last_kernel() == f"k_rows_scatter<{piece_of(B, S, off)}>"
    want = np.full((rows, S), 0xA5, np.uint8)
    want[p, :B] = x
    d = dbuf.cpu().numpy()
    assert (d[off:off + rows * S].reshape(rows, S) == want).all()
    assert (d[:off] == 0xA5).all() and (d[off + rows * S:] == 0xA5).all()


# ------------------------------------------------------------- put records ---
def _bucket_kernel(L, nranks):
    """The product's bucketing kernel for records (bucket_ref.py _bucket_kernel(..., records=True),
    variant 0): the staged scatter for 8/16/32-B keys below 2048 / 1463 / 256 ranks, two passes from there,
    the generic kernel for other lengths.  The staged shape is staged_shape()'s (pdht_bucket.hip): records
    rank by ballots below 512 ranks and by owner tables on 4 x 16 tiles from there while 40960 + 28 B per
    rank of dynamic LDS stay within 80 KiB."""
    wg = "k_bucket_scatter_wg<8>" if nranks <= 4096 else "k_bucket_scatter_wg<4>"
    if L in (8, 16, 32):
        if nranks >= {8: 2048, 16: 1463, 32: 256}[L]:
            return f"k_bucket_tl_pass2<{L}B>"
        if nranks >= 512 and 40960 + 28 * nranks <= 80 * 1024:
            return f"k_bucket_scatter_staged<{L}B,own>"
        return f"k_bucket_scatter_staged<{L}B>"
    return wg


LS, ES, NRANKS, NS = (8, 13, 16, 32, 64), (1, 8, 12, 40, 64, 256), (1, 7, 1000, 2049, 8192), (0, 1, 4095, 100003)


def _put_cases():
    """The product L x nranks x n x key_slot x E thinned to one E per (L, nranks, n, key_slot): E rotates with
    the sum of the other indices, so every E meets every L, every nranks, every n and both key_slot forms."""
    cases = []
    for iL, L in enumerate(LS):
        for inr, nr in enumerate(NRANKS):
            for in_, n in enumerate(NS):
                for islot, slot in enumerate((0, 32) if L <= 32 else (0, 64)):
                    cases.append((L, ES[(iL + inr + in_ + islot) % len(ES)], slot, nr, n))
    return cases


PUT_CASES = _put_cases()

_KEYS = {}


def _keys_and_order(oracle, L, nranks, n):
    """Keys, their digests and the stable bucket order, computed once per (L, nranks, n)."""
    if (L, nranks, n) not in _KEYS:
        k = np.random.default_rng(L * 11 + nranks + n).integers(0, 256, (n, L), dtype=np.uint8)
        if n:
            m2, _, r2 = oracle.pdht_hash_fixed(k, 3, nranks)
        else:
            m2, r2 = np.zeros(0, np.uint64), np.zeros(0, np.uint32)
        order = np.argsort(r2, kind="stable")
        offs = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=nranks))])
        _KEYS[L, nranks, n] = (k, m2, order, offs)
    return _KEYS[L, nranks, n]


def test_put_cases_cover_the_grid():
    assert 150 <= len(PUT_CASES) <= 400
    assert {(c[0], c[3]) for c in PUT_CASES} == {(L, nr) for L in LS for nr in NRANKS}
    for L in LS:
        assert {c[1] for c in PUT_CASES if c[0] == L} == set(ES)
    for slot_on in (False, True):
        assert {c[1] for c in PUT_CASES if bool(c[2]) == slot_on} == set(ES)
    for n in NS:
        assert {c[1] for c in PUT_CASES if c[4] == n} == set(ES)
    for nr in NRANKS:
        assert {c[1] for c in PUT_CASES if c[3] == nr} == set(ES)


@pytest.mark.parametrize("L,E,key_slot,nranks,n", PUT_CASES)
def test_bucket_put_records(dev, oracle, L, E, key_slot, nranks, n):
    k, m2, order, want_offs = _keys_and_order(oracle, L, nranks, n)
    v = np.random.default_rng(E + n).integers(0, 256, (n, E), dtype=np.uint8)
    kd, vd = to_dev(k, dev), to_dev(v, dev)
    rb = P.put_record_bytes(L, E, key_slot)
    slot = key_slot or (L + 7) // 8 * 8
    assert rb == 24 + slot + (E + 7) // 8 * 8
    out = (torch.full((n, rb), 0xA5, dtype=torch.uint8, device=dev),
           torch.full((nranks + 1,), -1, dtype=torch.int64, device=dev))
    rec, offs = P.bucket_put_records(kd, vd, nranks, key_slot=key_slot, src_rank=5, ht_index=3, out=out)
    # the mover's destination row runs from the end of the key to the end of the record: the slot gap, the
    # value (packed rows of E bytes in a 256-B aligned allocation, as the records are) and its pad to 8
    key_end = 24 + (L + 7) // 8 * 8
    piece = piece_of(E, key_end, rb, 24 + slot - key_end, rb - 24 - slot - E)
    if n:
        assert P.last_kernel() == f"{_bucket_kernel(L, nranks)}+k_rows_gather<{piece}>"
    assert rec.data_ptr() == out[0].data_ptr() and tuple(rec.shape) == (n, rb)
    assert (offs.cpu().numpy() == want_offs).all()
    if n == 0:
        return
    R = rec.cpu().numpy()
    w32 = R[:, :16].copy().view(np.uint32)
    assert (w32[:, 0] == P.PDHT_PUT).all() and (w32[:, 1] == 5).all() and (w32[:, 2] == 3).all()
    assert (w32[:, 3] == order).all()
    assert (R[:, 16:24].copy().view(np.uint64).ravel() == m2[order]).all()
    assert (R[:, 24:24 + L] == k[order]).all()
    assert (R[:, 24 + L:24 + slot] == 0).all()  # the key's pad and the slot gap
    assert (R[:, 24 + slot:24 + slot + E] == v[order]).all()
    assert (R[:, 24 + slot + E:] == 0).all()  # the value's pad to 8
    # header, index, mbits and key are bucket_records' own bytes
    plain, offs2 = P.bucket_records(kd, nranks, src_rank=5, ht_index=3)
    assert (plain.cpu().numpy()[:, :24 + L] == R[:, :24 + L]).all()
    assert (offs2.cpu().numpy() == want_offs).all()
    # values as a column slice of a wider tensor (value_stride > E)
    wide = torch.full((n, E + 11), 0x5A, dtype=torch.uint8, device=dev)
    wide[:, 3:3 + E] = vd
    out[0].fill_(0xA5)
    rec2, _ = P.bucket_put_records(kd, wide[:, 3:3 + E], nranks, key_slot=key_slot, src_rank=5, ht_index=3, out=out)
    assert (rec2.cpu().numpy() == R).all()
    # the fields round-trip
    ty, sr, hi, ix, mb, ko, vo = P.put_record_fields(rec2, L, E, key_slot)
    assert (ty.cpu().numpy() == P.PDHT_PUT).all() and (sr.cpu().numpy() == 5).all() and (hi.cpu().numpy() == 3).all()
    assert (ix.cpu().numpy().view(np.uint32) == order).all()
    assert (mb.cpu().numpy().view(np.uint64) == m2[order]).all()
    assert (ko.cpu().numpy() == k[order]).all() and (vo.cpu().numpy() == v[order]).all()


def test_put_is_putget_sbuf(dev, oracle):
    """key_slot = 32 (PDHT_MAXKEYSIZE), elemsize % 8 == 0: message_t (24 B), the key at +24, the value at
    +24 + PDHT_MAXKEYSIZE, sizeof(message_t) + PDHT_MAXKEYSIZE + elemsize bytes in all (putget.c:80-98); and the
    get flow: replies in bucket order scattered by the records' index are back in the caller's order."""
    L, E, nranks, n = 8, 16, 7, 4095
    k, m2, order, _ = _keys_and_order(oracle, L, nranks, n)
    v = np.random.default_rng(1).integers(0, 256, (n, E), dtype=np.uint8)
    rec, _ = P.bucket_put_records(to_dev(k, dev), to_dev(v, dev), nranks, key_slot=32)
    assert rec.shape[1] == 24 + 32 + E
    fields = P.put_record_fields(rec, L, E, 32)
    back = P.scatter_rows(fields[6], fields[3])  # strided views of the records, read in place
    assert (back.cpu().numpy() == v).all()


def test_put_records_needs_the_records_workspace(dev):
    """32-B keys at 1024 ranks take two passes as records: a workspace smaller than the records' size is
    refused before any launch, by the C ABI and by the wrapper."""
    n, L, E, nranks = 4097, 32, 8, 1024
    need = P.bucket_workspace_bytes(n, L, nranks, records=True)
    small = P.bucket_workspace_bytes(n, L, nranks)
    assert small < need
    k = torch.randint(0, 256, (n, L), dtype=torch.uint8, device=dev)
    v = torch.randint(0, 256, (n, E), dtype=torch.uint8, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rb = P.put_record_bytes(L, E)
    rec = torch.full((n * rb // 8,), -1, dtype=torch.int64, device=dev)
    offs = torch.zeros(nranks + 1, dtype=torch.int64, device=dev)
    lib = P.lib()
    s = torch.cuda.current_stream(dev).cuda_stream
    assert lib.pdht_bucket_put_records_dev(k.data_ptr(), L, v.data_ptr(), E, E, n, nranks, P.PDHT_PUT, 0, 0, 0,
                                           ws.data_ptr(), need - 1, rec.data_ptr(), offs.data_ptr(), s) != 0
    assert b"workspace too small" in lib.pdht_hip_last_error()
    torch.cuda.synchronize()
    assert (rec == -1).all()  # nothing ran
    with pytest.raises(ValueError, match="workspace"):
        P.bucket_put_records(k, v, nranks, workspace=ws[:small])
    _, offs = P.bucket_put_records(k, v, nranks, workspace=ws)
    assert P.last_kernel() == "k_bucket_tl_pass2<32B>+k_rows_gather<8>"
    o = offs.cpu().numpy()
    assert o[0] == 0 and o[-1] == n and (np.diff(o) >= 0).all()
