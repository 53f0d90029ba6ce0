"""Bucketing, the put / get flow and the placement sink at every key length.

A key whose size is not an aligned 8, 16 or 32 bytes takes the generic
bucketing path: k_bucket_count, k_bucket_scatter_wg<8|4>, packed_key_hash on
GlobalReader, copy_row, and OutRecT::key_copy with its pad loop.  As in
test_gpu_long_keys.py, a wrong branch there is wrong for one residue class of
lengths and nothing else, so every length 1..72 (pdht keys are any size up to
PDHT_MAXKEYSIZE = 32) and a few long ones run here, byte-exact against
oracle.pdht_hash_fixed plus a stable argsort, at both byte offsets of the
keys, with every output inside a guarded view.  The grids and what they cover
are in test_key_length_cases_cpu.py."""
import numpy as np
import pytest

import bucket_ref as B
import test_key_length_cases_cpu as KC

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

pytestmark = pytest.mark.gpu

N = KC.N
GUARD = 64  # bytes of 0xA5 on both sides of every output (a multiple of 16: the views keep their alignment)
CHUNK_IDS = [f"L{c[0]}-{c[-1]}" for c in KC.CHUNKS]


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


# ------------------------------------------------------- keys and references ---
_BUF, _REF, _VAL = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _BUF.clear()
    _REF.clear()
    _VAL.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def key_views(L, off, dev):
    """(host keys, device keys) [N, L]: the bytes off .. off + N * L of one seeded buffer per length, whose
    device copy starts 16-B aligned."""
    if L not in _BUF:
        host = np.random.default_rng(0x4B3E + L).integers(0, 256, N * L + 16, dtype=np.uint8)
        d = torch.from_numpy(host).to(dev)
        assert d.data_ptr() % 16 == 0
        _BUF[L] = (host, d)
    host, d = _BUF[L]
    kd = d[off:off + N * L].view(N, L)
    assert kd.data_ptr() % 16 == off
    return host[off:off + N * L].reshape(N, L), kd


def ref_of(k, L, off, nptes, nranks):
    """bucket_ref.reference of the batch, once per (L, offset, nptes, nranks)."""
    key = (L, off, nptes, nranks)
    if key not in _REF:
        _REF[key] = B.reference(k, nptes, nranks)
    return _REF[key]


def values_of(E, dev):
    if E not in _VAL:
        v = np.random.default_rng(0x7A1 + E).integers(0, 256, (N, E), dtype=np.uint8)
        _VAL[E] = (v, to_dev(v, dev))
    return _VAL[E]


class Guarded:
    """A tensor of `shape` and `dtype` in the middle of a larger allocation filled with 0xA5."""

    def __init__(self, shape, dtype, dev):
        self.nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((GUARD + self.nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.t = self.buf[GUARD:GUARD + self.nbytes].view(dtype).view(shape)
        self.shape, self.dtype = shape, dtype

    def host(self, where):
        """The body on the host, after checking that no guard byte changed."""
        h = self.buf.cpu()
        a = h.numpy()
        assert (a[:GUARD] == 0xA5).all(), (where, "bytes before the output were written")
        assert (a[GUARD + self.nbytes:] == 0xA5).all(), (where, "bytes past the output were written")
        return h[GUARD:GUARD + self.nbytes].view(self.dtype).view(self.shape)


def cases_of(chunk):
    return [c for c in KC.BUCKET_CASES if c[0] in chunk]


# ------------------------------------------------------------------ arrays ---
@pytest.mark.parametrize("chunk", KC.CHUNKS, ids=CHUNK_IDS)
def test_bucket_batch_every_length(dev, oracle, chunk):
    """Every output of bucket_batch; keys_out's N * L bytes end off a dword for most L."""
    for L, nranks, off, nptes, _E, _slot in cases_of(chunk):
        k, kd = key_views(L, off, dev)
        outs = (Guarded((N, L), torch.uint8, dev), Guarded((N,), torch.int64, dev), Guarded((N,), torch.int32, dev),
                Guarded((N,), torch.int32, dev), Guarded((nranks + 1,), torch.int64, dev))
        got = P.bucket_batch(kd, nptes, nranks, out=tuple(g.t for g in outs))
        where = (L, off, nranks, nptes)
        assert P.last_kernel() == KC.expected_kernel(L, nranks, off, False), (where, P.last_kernel())
        assert all(a.data_ptr() == g.t.data_ptr() for a, g in zip(got, outs))
        host = tuple(g.host(where + (i,)) for i, g in enumerate(outs))
        try:
            B.check_arrays(k, nptes, nranks, host, ref_of(k, L, off, nptes, nranks))
        except AssertionError as e:
            raise AssertionError(f"(L, offset, nranks, nptes) = {where}: {e}") from e


# ----------------------------------------------------------------- records ---
@pytest.mark.parametrize("chunk", KC.CHUNKS, ids=CHUNK_IDS)
def test_bucket_records_every_length(dev, oracle, chunk):
    """Header, index, mbits, key, and zeros in every pad byte up to the stride 24 + round8(L)."""
    for L, nranks, off, nptes, _E, _slot in cases_of(chunk):
        k, kd = key_views(L, off, dev)
        rb = 24 + (L + 7) // 8 * 8
        assert P.bucket_record_bytes(L) == rb
        rec, offs = Guarded((N, rb), torch.uint8, dev), Guarded((nranks + 1,), torch.int64, dev)
        got = P.bucket_records(kd, nranks, src_rank=5, ht_index=3, out=(rec.t, offs.t))
        where = (L, off, nranks)
        assert P.last_kernel() == KC.expected_kernel(L, nranks, off, True), (where, P.last_kernel())
        assert got[0].data_ptr() == rec.t.data_ptr()
        try:
            B.check_records(k, nranks, rec.host(where), offs.host(where), src_rank=5, ht_index=3,
                            ref=ref_of(k, L, off, nptes, nranks))
        except AssertionError as e:
            raise AssertionError(f"(L, offset, nranks) = {where}: {e}") from e


# ------------------------------------------------------------- put records ---
@pytest.mark.parametrize("chunk", KC.CHUNKS, ids=CHUNK_IDS)
def test_bucket_put_records_every_length(dev, oracle, chunk):
    """Put records with key_slot 0 and with the smallest multiple of 8 that holds max(L, 32): the key's pad,
    the slot gap and the value's pad are zeros; the mover's piece follows the layout."""
    for L, nranks, off, nptes, E, key_slot in cases_of(chunk):
        k, kd = key_views(L, off, dev)
        v, vd = values_of(E, dev)
        m, _, _, order, want_offs = ref_of(k, L, off, nptes, nranks)
        slot = key_slot or (L + 7) // 8 * 8
        rb = P.put_record_bytes(L, E, key_slot)
        assert rb == 24 + slot + (E + 7) // 8 * 8
        rec, offs = Guarded((N, rb), torch.uint8, dev), Guarded((nranks + 1,), torch.int64, dev)
        P.bucket_put_records(kd, vd, nranks, key_slot=key_slot, src_rank=5, ht_index=3, out=(rec.t, offs.t))
        where = (L, off, nranks, E, key_slot)
        key_end = 24 + (L + 7) // 8 * 8
        piece = piece_of(E, key_end, rb, 24 + slot - key_end, rb - 24 - slot - E)
        assert P.last_kernel() == f"{KC.expected_kernel(L, nranks, off, True)}+k_rows_gather<{piece}>", \
            (where, P.last_kernel())
        assert (offs.host(where).numpy() == want_offs).all(), where
        R = rec.host(where).numpy()
        w32 = R[:, :16].copy().view(np.uint32)
        assert (w32[:, 0] == P.PDHT_PUT).all() and (w32[:, 1] == 5).all() and (w32[:, 2] == 3).all(), where
        assert (w32[:, 3] == order).all(), where
        assert (R[:, 16:24].copy().view(np.uint64).ravel() == m[order]).all(), where
        assert (R[:, 24:24 + L] == k[order]).all(), where
        assert (R[:, 24 + L:24 + slot] == 0).all(), (where, "key pad / slot gap")
        assert (R[:, 24 + slot:24 + slot + E] == v[order]).all(), where
        assert (R[:, 24 + slot + E:] == 0).all(), (where, "value pad")


# ------------------------------------------- the owner's side and the way back ---
def distinct_keys(L, want, seed):
    """Up to `want` distinct L-byte keys in a seeded order (a 1-byte key has 256 values)."""
    rng = np.random.default_rng(seed)
    k = np.unique(rng.integers(0, 256, (2 * want, L), dtype=np.uint8), axis=0)
    return k[rng.permutation(len(k))][:want]


@pytest.mark.parametrize("chunk", KC.CHUNKS, ids=CHUNK_IDS)
def test_put_get_resolve_every_length(dev, oracle, chunk):
    """bucket_put_records -> DeviceTable.put_records -> bucket_records(get) over the same keys and absent
    ones -> table.get -> get_resolve by the records' index: present keys come back with status 0 and their
    value at the caller's row, absent ones with status 2 and the row untouched."""
    for L in chunk:
        E, key_slot = KC.chain_params(L)
        allk = distinct_keys(L, KC.CHAIN_N + KC.CHAIN_ABSENT, 0xC4A1 + L)
        nabs = min(KC.CHAIN_ABSENT, len(allk) // 4)
        keys, never = allk[:len(allk) - nabs], allk[len(allk) - nabs:]
        n = len(keys)
        assert n >= 192 and (L == 1 or n == KC.CHAIN_N)
        assert len(np.unique(oracle.city64_fixed(allk))) == len(allk)  # no two of them share mbits
        rng = np.random.default_rng(L * 1000 + E)
        values = rng.integers(0, 256, (n, E), dtype=np.uint8)
        records, _ = P.bucket_put_records(to_dev(keys, dev), to_dev(values, dev), 1, key_slot=key_slot)
        tab = P.DeviceTable(8192, records.shape[1] - 24, dev)
        st = tab.put_records(records)
        assert int(st.count_nonzero()) == 0 and tab.counts()[:3] == (n, 0, 1), L
        order = rng.permutation(n + nabs)
        keys2 = np.concatenate([keys, never])[order]
        k2d = to_dev(keys2, dev)
        get_records, _ = P.bucket_records(k2d, 1, msg_type=0)
        index = P.record_fields(get_records, L)[3]
        was_put = order < n
        want = np.full((n + nabs, E), 0xC3, np.uint8)
        want[was_put] = values[order[was_put]]
        for head in KC.HEADS:
            replies = tab.get(get_records, head=head)
            sentinel = torch.full((n + nabs, E), 0xC3, dtype=torch.uint8, device=dev)
            status = torch.full((n + nabs,), 0xEE, dtype=torch.uint8, device=dev)
            vals, status = P.get_resolve(replies, k2d, E, head=head, key_slot=key_slot, index=index,
                                         values=sentinel, status=status)
            assert (status.cpu().numpy() == np.where(was_put, 0, 2)).all(), (L, E, key_slot, head)
            assert (vals.cpu().numpy() == want).all(), (L, E, key_slot, head)


@pytest.mark.parametrize("chunk", KC.CHUNKS, ids=CHUNK_IDS)
def test_a_reply_that_differs_in_any_one_byte_is_a_collision(dev, chunk):
    """Per length, L found replies each with exactly one byte j = 0..L-1 of its key slot changed, among L
    untouched ones: every changed one resolves to status 3 and leaves its value row alone.  At head 1 and 8,
    with one value byte (the key alone sizes the lane group G: 1 for L <= 4, 2 for L <= 8, ...) and with 256
    (G = 64 at head 1), so that the group-strided compare runs with L below, at and above G."""
    for L in chunk:
        slot = (L + 7) // 8 * 8
        for head in KC.HEADS:
            for E in KC.FORGE_ES:
                rng = np.random.default_rng(L * 7919 + head * 31 + E)
                m, n = 2 * L, 2 * L + 3
                keys = rng.integers(0, 256, (n, L), dtype=np.uint8)
                index = rng.permutation(n)[:m].astype(np.uint32)
                rep = rng.integers(0, 256, (m, head + slot + E), dtype=np.uint8)
                rep[:, 0] = 1
                rep[:, head:head + L] = keys[index]
                forged = rng.permutation(m)[:L]  # reply forged[j] differs in byte j
                rep[forged, head + np.arange(L)] ^= rng.integers(1, 256, L).astype(np.uint8)
                is_forged = np.zeros(m, bool)
                is_forged[forged] = True
                want_s = np.full(n, 0xEE, np.uint8)
                want_s[index] = np.where(is_forged, 3, 0)
                want_v = np.full((n, E), 0x5A, np.uint8)
                want_v[index[~is_forged]] = rep[~is_forged, head + slot:head + slot + E]
                vals = torch.full((n, E), 0x5A, dtype=torch.uint8, device=dev)
                stat = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
                v, s = P.get_resolve(to_dev(rep, dev), to_dev(keys, dev), E, head=head,
                                     index=to_dev(index.view(np.int32), dev), values=vals, status=stat)
                where = (L, head, E, "G", KC.resolve_group(L, head, slot, E))
                assert P.last_kernel() == f"k_get_resolve<{KC.resolve_piece(head, slot, E)}>", where
                got_s = s.cpu().numpy()
                missed = np.flatnonzero(got_s[index[forged]] != 3)
                assert missed.size == 0, (where, "changed bytes not noticed", missed[:10])
                assert (got_s == want_s).all(), where
                assert (v.cpu().numpy() == want_v).all(), where


# ------------------------------------------ the placement sink per family ---
def place_keys(L, keyset):
    rng = np.random.default_rng(L * 13 + len(keyset))
    if keyset == "random":
        return rng.integers(0, 256, (KC.PLACE_N, L), dtype=np.uint8)
    few = rng.integers(0, 256, (1 if keyset == "identical" else 2, L), dtype=np.uint8)
    return few[np.arange(KC.PLACE_N) % len(few)]


@pytest.mark.parametrize("L", KC.PLACE_LENGTHS)
def test_place_sink_in_every_kernel_family(dev, oracle, L):
    """SinkPlace in the direct, transpose, window and global kernels: mbits, ptindex and rank without a
    histogram; with one (LDS bins up to 4096 ranks, global atomics above) 5 + bincount, and a second call
    accumulates.  Random keys, one key n times (one bin receives the whole batch) and two keys alternating."""
    PRE = 12345
    for keyset in KC.PLACE_KEYSETS:
        k = place_keys(L, keyset)
        kd = to_dev(k, dev)
        assert kd.data_ptr() % 16 == 0
        for nranks in KC.PLACE_NRANKS:
            m2, p2, r2 = oracle.pdht_hash_fixed(k, 7, nranks)
            count = np.bincount(r2, minlength=nranks)
            if keyset == "identical":
                assert count.max() == KC.PLACE_N
            for with_hist in (False, True):
                hist = torch.full((nranks,), 5, dtype=torch.int64, device=dev) if with_hist else None
                mb, pt, rk = P.place_batch(kd, 7, nranks, hist=hist)
                where = (L, keyset, nranks, with_hist)
                assert P.last_kernel() == KC.place_kernel(L, with_hist), (where, P.last_kernel())
                assert (mb.cpu().numpy().view(np.uint64) == m2).all(), where
                assert (pt.cpu().numpy().view(np.uint32) == p2).all(), where
                assert (rk.cpu().numpy().view(np.uint32) == r2).all(), where
                if with_hist:
                    assert (hist.cpu().numpy() == 5 + count).all(), where
                    P.place_batch(kd[:PRE], 7, nranks, hist=hist)
                    assert (hist.cpu().numpy() == 5 + count + np.bincount(r2[:PRE], minlength=nranks)).all(), where
