"""Destination bucketing on the buffers a caller really hands it: a workspace
full of another call's leftovers or of poison, a workspace and outputs of
exactly the stated size between guard bytes, key pointers that fail the
kernels' vector alignment, side streams, graph capture -- and the refusal of
workspace and output pointers that the kernels could not address.  Uniform
random keys; every output is compared byte for byte with the oracle's stable
order (bucket_ref.py), and the kernel that ran is asserted."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import bucket_ref as B  # noqa: E402
import pdht_amd as P  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
# per key size a one-pass and a two-pass rank count (13-B keys: the generic kernel in 8 and in 4 waves)
ARRAY_CONFIGS = [(8, 1000), (8, 8192), (16, 1000), (16, 2049), (32, 1000), (32, 2049), (13, 1000), (13, 4097)]
RECORD_CONFIGS = [(8, 1000), (8, 8192), (16, 1000), (16, 2049), (32, 7), (32, 1000), (13, 1000), (13, 4097)]
KIND_CONFIGS = [("arrays", L, nr) for (L, nr) in ARRAY_CONFIGS] + [("records", L, nr) for (L, nr) in RECORD_CONFIGS]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_configs_cover_one_and_two_passes():
    for kind, configs in (("arrays", ARRAY_CONFIGS), ("records", RECORD_CONFIGS)):
        for L in (8, 16, 32):
            names = {B._bucket_kernel(L2, nr, 0, kind == "records") for (L2, nr) in configs if L2 == L}
            assert len(names) == 2 and f"k_bucket_tl_pass2<{L}B>" in names
        assert {B._bucket_kernel(13, nr, 0) for (L2, nr) in configs if L2 == 13} == \
            {"k_bucket_scatter_wg<8>", "k_bucket_scatter_wg<4>"}


_KEYS = {}


def keys_and_ref(n, L, nranks, seed=0):
    """Uniform random keys and their reference, made once per shape and never written."""
    key = (n, L, nranks, seed)
    if key not in _KEYS:
        k = np.random.default_rng(n * 7 + L * 1009 + nranks + seed).integers(0, 256, (n, L), dtype=np.uint8)
        _KEYS[key] = (k, B.reference(k, 3, nranks))
    return _KEYS[key]


def run(kind, kd, nranks, **kw):
    if kind == "arrays":
        return P.bucket_batch(kd, 3, nranks, **kw)
    return P.bucket_records(kd, nranks, src_rank=5, ht_index=3, **kw)


def check(kind, k, nranks, got, ref):
    if kind == "arrays":
        B.check_arrays(k, 3, nranks, got, ref)
    else:
        B.check_records(k, nranks, got[0], got[1], P.PDHT_PUT, 5, 3, ref)


def ws_bytes(kind, n, L, nranks):
    return P.bucket_workspace_bytes(n, L, nranks, records=kind == "records")


def host_bytes(got):
    return [None if t is None else t.cpu().numpy().copy() for t in got]


# --------------------------------------------------------------- workspace ---
SEQUENCE = [("arrays", 300_007, 8, 8192),   # two passes
            ("arrays", 70_001, 16, 1000),   # staged scatter, owner tables on 8 x 16 tiles, per-XCD tickets
            ("records", 70_001, 13, 1000),  # generic length
            ("arrays", 0, 8, 8192),         # the two-pass path's n = 0: k_bucket_base alone
            ("records", 100_003, 32, 1024),  # two passes at another n, other tiles and digits
            ("records", 4095, 8, 7),        # staged scatter with ballots, two ragged tiles
            ("arrays", 0, 16, 1000),        # the one-pass path's n = 0
            ("arrays", 70_001, 8, 8192),    # two passes again, fewer tiles than the leftovers describe
            ("arrays", 50_000, 13, 4097),   # generic length in 4 waves
            ("arrays", 70_001, 32, 2049)]   # two passes, 32-B rows


def test_workspace_contents_do_not_matter(dev):
    """The workspace is scratch: what it holds on entry is never read.

    Read in bucket.h / pdht_bucket.hip before this test was written:
    - one pass (k_bucket_count* -> colscan -> chunkscan -> base -> scatter): the count kernel stores
      counts[t][r] for every tile t < ntiles and every rank; the column scan reads exactly those and stores
      chunks[c][r] for every chunk; the chunk scan reads exactly those and stores totals[r] for every rank;
      k_bucket_base reads totals, stores base[r] and zeroes the 16 ticket words before the scatter's first
      atomicAdd on them; the scatter reads base, chunks and counts at the indices written above.
    - two passes: pass 1 stores startsF[t][f] for all F digits of every tile, rows [0, n) of the key rows
      and u16 indices, and chunkcnt[g][r] for every chunk and rank; k_bucket_chunkscan_tl reads exactly
      those and stores totals[r], inpre[r] and bsum[block] for every rank / block of 64; pass 2 reads
      startsF[t][f], startsF[t][f + 1] (or the tile's length), chunkcnt, inpre, bsum and rows < n only.
    - n = 0: only k_bucket_base runs, and it is handed no totals (a null pointer: every total is 0).  Both
      paths used to hipMemsetAsync the totals ahead of it; as a node of a captured graph that memset left
      them as they were (test_bucketing_captures_in_a_hip_graph), so it is gone.
    So this test confirms a reading; it is not a probe.  One caller-owned workspace, sized for the largest
    call, takes a sequence of calls of different (kind, n, L, nranks): once as it comes (each call meets the
    leftovers of the one before), once filled with 0xFF before each call, once zeroed before each call.
    All three equal the oracle and each other bit for bit, bucket_offsets included."""
    ws = torch.empty(max(ws_bytes(*c) for c in SEQUENCE), dtype=torch.uint8, device=dev)
    ws.fill_(0x5A)
    runs = []
    for fill in (None, 0xFF, 0):
        outs = []
        for kind, n, L, nranks in SEQUENCE:
            k, ref = keys_and_ref(n, L, nranks)
            if fill is not None:
                ws.fill_(fill)
            got = run(kind, to_dev(k, dev), nranks, workspace=ws)
            want = "k_bucket_base" if n == 0 else B._bucket_kernel(L, nranks, 0, kind == "records")
            assert P.last_kernel() == want, (kind, n, L, nranks)
            check(kind, k, nranks, got, ref)
            outs.append(host_bytes(got))
        runs.append(outs)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("n", [1, 70_001])
@pytest.mark.parametrize("kind,L,nranks", KIND_CONFIGS)
def test_exact_size_workspace_between_guards(dev, kind, L, nranks, n):
    """A workspace of exactly the queried size inside a 0xA5-filled buffer: no byte before or after it changes."""
    need = ws_bytes(kind, n, L, nranks)
    buf = torch.full((4096 + need + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    k, ref = keys_and_ref(n, L, nranks)
    got = run(kind, to_dev(k, dev), nranks, workspace=buf[4096:4096 + need])
    assert P.last_kernel() == B._bucket_kernel(L, nranks, 0, kind == "records")
    check(kind, k, nranks, got, ref)
    assert bool((buf[:4096] == 0xA5).all()) and bool((buf[4096 + need:] == 0xA5).all())


# ----------------------------------------------------------------- outputs ---
def carve(dev, parts):
    """One 0xA5-filled buffer holding a region per (nbytes, alignment, offset past the alignment) of
    `parts`, GUARD bytes or more before, between and after them -> (buffer, [region starts])."""
    assert torch.empty(1, dtype=torch.uint8, device=dev).data_ptr() % 256 == 0
    off, starts = GUARD, []
    for nbytes, align, phase in parts:
        off = (off + align - 1) // align * align + phase
        starts.append(off)
        off += nbytes + GUARD
    return torch.full((off,), 0xA5, dtype=torch.uint8, device=dev), starts


def guards_intact(buf, spans):
    h = buf.cpu().numpy()
    written = np.zeros(h.size, bool)
    for start, nbytes in spans:
        written[start:start + nbytes] = True
    return bool((h[~written] == 0xA5).all())


@pytest.mark.parametrize("n", [1, 4095, 70_001])
@pytest.mark.parametrize("L,nranks", ARRAY_CONFIGS)
def test_array_outputs_between_guards(dev, L, nranks, n):
    """keys_out, mbits_out, ptindex_out, index_out and bucket_offsets as views of one buffer, each aligned
    as its type needs (the key rows to 16 bytes, so that 8/16/32-B keys stay on their fast kernel) with
    guard bytes around: the call writes its outputs and nothing else.  With keys, ptindex or index left
    out, their regions too stay untouched."""
    k, ref = keys_and_ref(n, L, nranks)
    kd = to_dev(k, dev)
    sizes = [n * L, 8 * n, 4 * n, 4 * n, 8 * (nranks + 1)]
    for wk, wp, wi in ((True, True, True), (False, False, True), (True, False, False), (False, False, False)):
        buf, st = carve(dev, [(sizes[0], 16, 0), (sizes[1], 8, 0), (sizes[2], 4, 4), (sizes[3], 4, 4), (sizes[4], 8, 8)])
        v = [buf[s:s + b] for s, b in zip(st, sizes)]
        out = (v[0].view(n, L) if wk else None, v[1].view(torch.int64), v[2].view(torch.int32) if wp else None,
               v[3].view(torch.int32) if wi else None, v[4].view(torch.int64))
        got = P.bucket_batch(kd, 3, nranks, out=out)
        assert P.last_kernel() == B._bucket_kernel(L, nranks, 0)
        assert all((g is None and o is None) or g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
        B.check_arrays(k, 3, nranks, got, ref)
        assert guards_intact(buf, [(s, b) for s, b, o in zip(st, sizes, out) if o is not None]), (wk, wp, wi)


@pytest.mark.parametrize("n", [1, 4095, 70_001])
@pytest.mark.parametrize("L,nranks", RECORD_CONFIGS)
def test_record_outputs_between_guards(dev, L, nranks, n):
    """The records at an address that is 8 but not 16 bytes aligned (all the ABI asks for) and the offsets,
    with guard bytes around: nothing before the first record, after the last one or around the offsets
    is written."""
    k, ref = keys_and_ref(n, L, nranks)
    rb = P.bucket_record_bytes(L)
    sizes = [n * rb, 8 * (nranks + 1)]
    buf, st = carve(dev, [(sizes[0], 16, 8), (sizes[1], 8, 0)])
    out = (buf[st[0]:st[0] + sizes[0]].view(n, rb), buf[st[1]:st[1] + sizes[1]].view(torch.int64))
    assert out[0].data_ptr() % 16 == 8
    rec, offs = P.bucket_records(to_dev(k, dev), nranks, src_rank=5, ht_index=3, out=out)
    assert P.last_kernel() == B._bucket_kernel(L, nranks, 0, records=True)
    assert rec.data_ptr() == out[0].data_ptr()
    B.check_records(k, nranks, rec, offs, P.PDHT_PUT, 5, 3, ref)
    assert guards_intact(buf, list(zip(st, sizes)))


# ------------------------------------------------- pointers off the vectors ---
def expected_kernel(kind, L, nranks, *ptrs):
    """bucket_impl's `fixed` test: 8-B keys on an 8-byte boundary, 16/32-B keys on a 16-byte one -- the
    input keys and, for arrays, the output keys -- else the generic-length kernel."""
    al = 0
    for p in ptrs:
        al |= p
    fixed = al % 8 == 0 if L == 8 else al % 16 == 0
    return B._bucket_kernel(L, nranks, 0, kind == "records") if fixed else \
        "k_bucket_scatter_wg<8>" if nranks <= 4096 else "k_bucket_scatter_wg<4>"


@pytest.mark.parametrize("off", [1, 4, 8])
@pytest.mark.parametrize("nranks", [1000, 8192])
@pytest.mark.parametrize("L", [8, 16, 32])
def test_keys_off_the_vector_alignment(dev, L, nranks, off):
    """Packed keys that start `off` bytes into an allocation, as inputs, as output keys, and both: 8-B keys
    at offset 8 stay on the fast kernel, every other combination takes the generic-length kernel, and the
    outputs equal the oracle either way.  Records written by the generic kernel carry zero pad bytes."""
    n = 70_001
    k, ref = keys_and_ref(n, L, nranks)
    flat = torch.zeros(n * L + 32, dtype=torch.uint8, device=dev)
    kmis = flat[off:off + n * L].view(n, L)
    kmis.copy_(to_dev(k, dev))
    kd = to_dev(k, dev)
    assert kmis.data_ptr() % 256 == off and kd.data_ptr() % 256 == 0
    slow = not (L == 8 and off == 8)
    assert (expected_kernel("arrays", L, nranks, off) == B._bucket_kernel(L, nranks, 0)) == (not slow)
    # misaligned input keys
    rec, offs = P.bucket_records(kmis, nranks, src_rank=5, ht_index=3)
    assert P.last_kernel() == expected_kernel("records", L, nranks, kmis.data_ptr())
    B.check_records(k, nranks, rec, offs, P.PDHT_PUT, 5, 3, ref)
    got = P.bucket_batch(kmis, 3, nranks)
    assert P.last_kernel() == expected_kernel("arrays", L, nranks, kmis.data_ptr(), got[0].data_ptr())
    B.check_arrays(k, 3, nranks, got, ref)
    # misaligned output keys between guard bytes, from aligned and from misaligned input keys
    for src in (kd, kmis):
        obuf = torch.full((n * L + 32,), 0xA5, dtype=torch.uint8, device=dev)
        out = (obuf[off:off + n * L].view(n, L), torch.empty(n, dtype=torch.int64, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(nranks + 1, dtype=torch.int64, device=dev))
        got = P.bucket_batch(src, 3, nranks, out=out)
        assert P.last_kernel() == expected_kernel("arrays", L, nranks, src.data_ptr(), out[0].data_ptr())
        assert P.last_kernel().startswith("k_bucket_scatter_wg") == slow
        B.check_arrays(k, 3, nranks, got, ref)
        assert bool((obuf[:off] == 0xA5).all()) and bool((obuf[off + n * L:] == 0xA5).all())


# ----------------------------------------------------------------- streams ---
def check_put(k, v, nranks, rec, offs, ref):
    m, _, _, order, want_offs = ref
    L, E = k.shape[1], v.shape[1]
    assert (offs.cpu().numpy() == want_offs).all()
    ty, sr, hi, ix, mb, ko, vo = P.put_record_fields(rec, L, E)
    assert (ty.cpu().numpy() == P.PDHT_PUT).all() and (sr.cpu().numpy() == 5).all() and (hi.cpu().numpy() == 3).all()
    assert (ix.cpu().numpy().view(np.uint32) == order).all()
    assert (mb.cpu().numpy().view(np.uint64) == m[order]).all()
    assert (ko.cpu().numpy() == k[order]).all() and (vo.cpu().numpy() == v[order]).all()
    R = rec.cpu().numpy()
    slot = (L + 7) // 8 * 8
    assert (R[:, 24 + L:24 + slot] == 0).all() and (R[:, 24 + slot + E:] == 0).all()


@pytest.mark.parametrize("L,nranks", [(8, 1000), (8, 8192), (32, 1024), (13, 1000)])
def test_entry_points_on_a_side_stream(dev, L, nranks):
    """Keys and values are copied to the device on a side stream and every entry point runs on it, nothing
    on the current stream: bucket_batch, bucket_records, bucket_put_records, gather_rows, scatter_rows."""
    n, E = 70_001, 12
    k, ref = keys_and_ref(n, L, nranks)
    v = np.random.default_rng(L + nranks).integers(0, 256, (n, E), dtype=np.uint8)
    kh, vh = torch.from_numpy(k).pin_memory(), torch.from_numpy(v).pin_memory()
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        kd = torch.empty((n, L), dtype=torch.uint8, device=dev)
        vd = torch.empty((n, E), dtype=torch.uint8, device=dev)
        kd.copy_(kh, non_blocking=True)
        vd.copy_(vh, non_blocking=True)
        got = P.bucket_batch(kd, 3, nranks, stream=s)
        assert P.last_kernel() == B._bucket_kernel(L, nranks, 0)
        rec = P.bucket_records(kd, nranks, src_rank=5, ht_index=3, stream=s)
        assert P.last_kernel() == B._bucket_kernel(L, nranks, 0, records=True)
        put = P.bucket_put_records(kd, vd, nranks, src_rank=5, ht_index=3, stream=s)
        rows = P.gather_rows(vd, got[3], stream=s)
        back = P.scatter_rows(rows, got[3], stream=s)
    s.synchronize()
    B.check_arrays(k, 3, nranks, got, ref)
    B.check_records(k, nranks, rec[0], rec[1], P.PDHT_PUT, 5, 3, ref)
    check_put(k, v, nranks, put[0], put[1], ref)
    assert (rows.cpu().numpy() == v[ref[3]]).all() and (back.cpu().numpy() == v).all()


@pytest.mark.parametrize("kind", ["arrays", "records"])
def test_two_streams_back_to_back(dev, kind):
    """A one-pass call on one side stream and a two-pass call on another, each with its own keys, workspace
    and outputs, issued back to back without synchronising in between: both are right after one
    torch.cuda.synchronize()."""
    n, L = 300_007, 8
    calls = []
    for nranks in (1000, 8192):
        k, ref = keys_and_ref(n, L, nranks, seed=nranks)
        kd = to_dev(k, dev)
        ws = torch.full((ws_bytes(kind, n, L, nranks),), 0xFF, dtype=torch.uint8, device=dev)
        out = run(kind, kd, nranks, workspace=ws)  # allocates the outputs; warms the kernels up
        for t in out:
            t.fill_(0)
        calls.append((nranks, k, ref, kd, ws, out, torch.cuda.Stream(device=dev)))
    torch.cuda.synchronize()
    for nranks, k, ref, kd, ws, out, s in calls:
        run(kind, kd, nranks, workspace=ws, out=out, stream=s)
    torch.cuda.synchronize()
    for nranks, k, ref, kd, ws, out, s in calls:
        check(kind, k, nranks, out, ref)


# ----------------------------------------------------------------- capture ---
def test_bucketing_captures_in_a_hip_graph(dev):
    """One linear capture on one stream of the entry points the other capture tests leave out: bucket_batch
    at 8192 ranks (two passes), bucket_records of 32-B keys at 1024 ranks (two passes), bucket_put_records
    at 1000 ranks, gather_rows by the captured index output and scatter_rows back -- all through one
    workspace -- replayed twice on new keys and values.  And the two-pass path's n = 0 call, replayed on a
    workspace full of 0xFF: it was a hipMemsetAsync of the rank totals and k_bucket_base, and the replayed
    memset node left the totals as they were (offsets of garbage); now k_bucket_base alone."""
    n, E = 50_001, 16
    k8 = torch.zeros((n, 8), dtype=torch.uint8, device=dev)
    k32 = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    vals = torch.zeros((n, E), dtype=torch.uint8, device=dev)
    k0 = torch.empty((0, 8), dtype=torch.uint8, device=dev)
    ws = torch.empty(max(ws_bytes("arrays", n, 8, 8192), ws_bytes("records", n, 32, 1024),
                         ws_bytes("records", n, 8, 1000)), dtype=torch.uint8, device=dev)

    def calls(outs=None):
        bk, rc, pr, ga, sc, z = outs or (None,) * 6
        bk = P.bucket_batch(k8, 3, 8192, out=bk, workspace=ws)
        rc = P.bucket_records(k32, 1024, src_rank=5, ht_index=3, out=rc, workspace=ws)
        pr = P.bucket_put_records(k8, vals, 1000, src_rank=5, ht_index=3, out=pr, workspace=ws)
        ga = P.gather_rows(vals, bk[3], out=ga)
        sc = P.scatter_rows(ga, bk[3], out=sc)
        return bk, rc, pr, ga, sc, z

    outs = calls()  # eager: allocates the outputs; the kernels' attributes are queried and set
    z = P.bucket_batch(k0, 3, 8192, workspace=ws)
    outs = outs[:5] + (z,)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture, as test_batches_capture_in_hip_graph does
        calls(outs)
        P.bucket_batch(k0, 3, 8192, out=z, workspace=ws)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        calls(outs)
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0):
        P.bucket_batch(k0, 3, 8192, out=z, workspace=ws)
    assert P.last_kernel() == "k_bucket_base"
    bk, rc, pr, ga, sc, _ = outs
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        h8, h32 = rng.integers(0, 256, (n, 8), dtype=np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)
        hv = rng.integers(0, 256, (n, E), dtype=np.uint8)
        k8.copy_(torch.from_numpy(h8))
        k32.copy_(torch.from_numpy(h32))
        vals.copy_(torch.from_numpy(hv))
        for t in bk + rc + pr + (ga, sc):
            t.fill_(0xA5 if t.dtype == torch.uint8 else -1)
        g.replay()
        torch.cuda.synchronize()
        ref = B.reference(h8, 3, 8192)
        B.check_arrays(h8, 3, 8192, bk, ref)
        B.check_records(h32, 1024, rc[0], rc[1], P.PDHT_PUT, 5, 3)
        check_put(h8, hv, 1000, pr[0], pr[1], B.reference(h8, 3, 1000))
        assert (ga.cpu().numpy() == hv[ref[3]]).all()
        assert (sc.cpu().numpy() == hv).all()  # the scatter of the gather: the original rows
        z[4].fill_(-1)
        ws.fill_(0xFF)
        g0.replay()
        torch.cuda.synchronize()
        assert (z[4].cpu().numpy() == 0).all()


# ------------------------------------------------------------------ refusal ---
def test_misaligned_buffers_are_refused(dev):
    """The workspace holds u32 counters, u64 totals, the tickets' atomics and key rows read as 16-byte
    vectors; mbits and the offsets are u64, ptindex and index u32.  A pointer off its alignment is refused
    before any launch by all three entry points, the message names the argument, and the outputs keep
    their bytes; the wrapper refuses a workspace view that starts one byte in."""
    n, L, E, nranks = 4097, 8, 8, 8192
    need = max(ws_bytes("arrays", n, L, nranks), ws_bytes("records", n, L, nranks))
    rb, prb = P.bucket_record_bytes(L), P.put_record_bytes(L, E)
    k = torch.randint(0, 256, (n, L), dtype=torch.uint8, device=dev)
    v = torch.randint(0, 256, (n, E), dtype=torch.uint8, device=dev)
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev)

    def a5(nbytes):
        return torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=dev)

    ko, mb, pt, ix, of, rec = a5(n * L), a5(8 * n), a5(4 * n), a5(4 * n), a5(8 * (nranks + 1)), a5(n * prb)
    lib = P.lib()
    s = torch.cuda.current_stream(dev).cuda_stream
    W, MB, PT, IX, OF = ws.data_ptr(), mb.data_ptr(), pt.data_ptr(), ix.data_ptr(), of.data_ptr()
    assert W % 256 == 0 and MB % 256 == 0 and PT % 256 == 0 and IX % 256 == 0 and OF % 256 == 0

    def arrays(w=W, m=MB, p=PT, i=IX, o=OF):
        return lib.pdht_bucket_batch_dev(k.data_ptr(), L, n, 3, nranks, w, need, ko.data_ptr(), m, p, i, o, s)

    def records(w=W, o=OF):
        return lib.pdht_bucket_records_dev(k.data_ptr(), L, n, nranks, P.PDHT_PUT, 0, 0, w, need, rec.data_ptr(), o, s)

    def put(w=W, o=OF):
        return lib.pdht_bucket_put_records_dev(k.data_ptr(), L, v.data_ptr(), E, E, n, nranks, P.PDHT_PUT, 0, 0, 0,
                                               w, need, rec.data_ptr(), o, s)

    bad = [(f, "workspace", dict(w=W + d)) for f in (arrays, records, put) for d in (1, 4, 8)]
    bad += [(f, "bucket_offsets", dict(o=OF + d)) for f in (arrays, records, put) for d in (1, 4)]
    bad += [(arrays, "mbits_out", dict(m=MB + d)) for d in (1, 4)]
    bad += [(arrays, "ptindex_out", dict(p=PT + d)) for d in (1, 2)]
    bad += [(arrays, "index_out", dict(i=IX + d)) for d in (1, 2)]
    for f, name, kw in bad:
        assert f(**kw) != 0, (f.__name__, kw)
        msg = lib.pdht_hip_last_error()
        assert name.encode() in msg and b"aligned" in msg, (f.__name__, name, msg)
    torch.cuda.synchronize()
    for t in (ko, mb, pt, ix, of, rec):
        assert bool((t == 0xA5).all())  # nothing ran
    with pytest.raises(ValueError, match="workspace"):
        P.bucket_batch(k, 3, nranks, workspace=ws[1:])
    with pytest.raises(ValueError, match="workspace"):
        P.bucket_records(k, nranks, workspace=ws[8:])
    with pytest.raises(ValueError, match="workspace"):
        P.bucket_put_records(k, v, nranks, workspace=ws[4:])
    # a workspace 16 bytes in is as good as any
    kh = k.cpu().numpy()
    B.check_arrays(kh, 3, nranks, P.bucket_batch(k, 3, nranks, workspace=ws[16:]))
    assert P.last_kernel() == "k_bucket_tl_pass2<8B>"
    assert arrays() == 0 and records() == 0, lib.pdht_hip_last_error()
    torch.cuda.synchronize()
    B.check_records(kh, nranks, rec[:n * rb].view(n, rb), of[:8 * (nranks + 1)].view(torch.int64))
