"""The host-resident batches (pdht_amd/csrc/pdht_host.hip) at chunk, slot and
pinning edges.

The copy pipeline cuts a batch into chunks of at most CHUNK key bytes (and,
for offset-indexed keys, at most MAXK keys) and runs them round-robin through
three slots; pinned buffers are copied by DMA in place, pageable ones through
staging, and all-pinned batches run zero-copy kernels.  Every case here
crosses at least one chunk edge (or names the edge it aims at) and compares
EVERY output element with the compiled oracle; every output array is
pre-filled with a sentinel and carries 8 trailing elements that must keep it.

CHUNK and MAXK restate kChunkBytes and max_keys (= kChunkBytes / 16) of
pdht_host.hip.  Should those constants change, the tests still compare every
digest; only their aim at the edges moves (tests/test_host_chunks_cpu.py
pins the two values in the source).

Left out on purpose: a single key longer than a chunk on the GPU
(city64_batch_host with L > 32 MiB, or one 33-MiB variable-length key).  One
lane walks such a key serially; nobody has measured how long that takes, and
it does not belong in a seconds-long test.  Its planning is covered on the
CPU (tests/test_host_chunks_cpu.py: the 500-byte keys over 64-byte chunks).
"""
import ctypes as C
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import pdht_amd as P  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 32 << 20     # kChunkBytes
MAXK = CHUNK // 16   # max_keys of the variable-length planner
SENT = {np.dtype(np.uint64): 0xA5A5A5A5A5A5A5A5, np.dtype(np.uint32): 0xA5A5A5A5}
TAIL = 8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------- helpers ---
def pinned(n, dt):
    """torch pin_memory() storage viewed as numpy."""
    return torch.zeros(max(n, 1) * np.dtype(dt).itemsize, dtype=torch.uint8).pin_memory().numpy().view(dt)[:n]


def pin_copy(a):
    p = pinned(a.size, a.dtype).reshape(a.shape)
    p[...] = a
    return p


def sink(n, dt, pin=False):
    """A flat output array of n + TAIL sentinels."""
    a = pinned(n + TAIL, dt) if pin else np.empty(n + TAIL, dt)
    a[:] = SENT[np.dtype(dt)]
    return a


def same(got, want, what=""):
    """Every element equal; on a mismatch name the first index and the count."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {int(bad[0])}: " \
                          f"{int(got[bad[0]]):#x} != {int(want[bad[0]]):#x}"


def kept(a, used, what=""):
    """The elements past `used` still hold the sentinel."""
    tail = a.reshape(-1)[used:]
    assert tail.size >= TAIL and (tail == SENT[a.dtype]).all(), f"{what}: sentinel after the output overwritten"


def per_of(L):
    return CHUNK // L


class Batches:
    """Keys and oracle results, computed once per key length and shared: key i
    of length L is bytes [i*L, (i+1)*L) of one byte stream, so a batch of n
    keys is a prefix of a longer one."""

    def __init__(self, oracle):
        self.o = oracle
        self._keys, self._pin, self._c64, self._crc, self._place = {}, {}, {}, {}, {}

    def n_max(self, L):
        return 6 * per_of(L) + 1 if L == 64 else 3 * per_of(L) + 17

    def keys(self, L, n, pin=False):
        if L not in self._keys:
            self._keys[L] = self.o.fixed_keys(self.n_max(L), L)
        if pin:
            if L not in self._pin:  # the 4-chunk prefix
                self._pin[L] = pin_copy(self._keys[L][:3 * per_of(L) + 17])
            return self._pin[L][:n]
        return self._keys[L][:n]

    def city64(self, L, n):
        if L not in self._c64:
            self._c64[L] = self.o.city64_fixed(self.keys(L, self.n_max(L)))
        return self._c64[L][:n]

    def crc128(self, L, n):
        if L not in self._crc:
            self._crc[L] = self.o.city128_fixed(self.keys(L, 3 * per_of(L) + 17), crc=True)
        return self._crc[L][:n]

    def place(self, L, n, nptes, nranks):
        k = (L, nptes, nranks)
        if k not in self._place:
            self._place[k] = self.o.pdht_hash_fixed(self.keys(L, 3 * per_of(L) + 17), nptes, nranks)
        return tuple(a[:n] for a in self._place[k])


@pytest.fixture(scope="module")
def B(oracle):
    return Batches(oracle)


# -------------------------------------- a. fixed keys over chunk edges ---
# keys -> out: pageable -> pageable (staged both ways), pinned -> pageable
# (chunk_in's direct DMA, harvest out), pageable -> pinned (staged in,
# chunk_out's direct DMA)
PINNING = [(False, False), (True, False), (False, True)]
PIN_IDS = ["pageable-pageable", "pinned-pageable", "pageable-pinned"]


@pytest.mark.parametrize("pin", PINNING, ids=PIN_IDS)
@pytest.mark.parametrize("L", [8, 13, 64, 1000])
def test_city64_four_chunks(dev, B, L, pin):
    """n = 3*per + 17: 4 chunks, slot 0 reused, the last chunk ragged.  For
    L = 13 and 1000, per is no multiple of 64 (2 581 110, 33 554): every chunk
    after the first starts mid-tile in the caller's buffer."""
    n = 3 * per_of(L) + 17
    out = sink(n, np.uint64, pin[1])
    got = P.city64_batch_host(B.keys(L, n, pin[0]), out=out)
    assert got is out
    same(out[:n], B.city64(L, n), f"city64 L={L}")
    kept(out, n)


@pytest.mark.parametrize("pin", PINNING, ids=PIN_IDS)
@pytest.mark.parametrize("L", [64, 1000])
def test_crc128_four_chunks(dev, B, L, pin):
    """16 B of output per key; L = 1000 takes the keylen > 900 launcher
    (CrcLds<AlgoCrc128>) on the host path."""
    n = 3 * per_of(L) + 17
    out = sink(2 * n, np.uint64, pin[1])
    P.citycrc128_batch_host(B.keys(L, n, pin[0]), out=out)
    same(out[:2 * n], B.crc128(L, n), f"crc128 L={L}")
    kept(out, 2 * n)


PER64 = CHUNK // 64


@pytest.mark.parametrize("n", [1, PER64 - 1, PER64, PER64 + 1, 2 * PER64])
def test_city64_exact_multiples(dev, B, n):
    """Batches that end on, one before and one after a chunk edge: on an
    exact multiple the plan must not emit an empty chunk."""
    out = sink(n, np.uint64)
    P.city64_batch_host(B.keys(64, n), out=out)
    same(out[:n], B.city64(64, n), f"n={n}")
    kept(out, n)


def test_city64_seven_chunks(dev, B):
    """6*per + 1 keys: 7 chunks, so slot 0 is used three times and slots 1, 2
    twice; the harvest list of each is drained and refilled."""
    n = 6 * PER64 + 1
    out = sink(n, np.uint64)
    P.city64_batch_host(B.keys(64, n), out=out)
    same(out[:n], B.city64(64, n), "7 chunks")
    kept(out, n)


def test_empty_batch_leaves_output_untouched(dev):
    k = np.zeros((0, 64), np.uint8)
    out = sink(0, np.uint64)
    P.city64_batch_host(k, out=out)
    P.citycrc128_batch_host(k, out=out)
    outs = (sink(0, np.uint64), sink(0, np.uint32), sink(0, np.uint32))
    P.place_batch_host(k, 3, 10, out=outs)
    P.city64_var_batch_host(np.zeros(5, np.uint8), np.zeros(1, np.uint64), out=out)
    for a in (out,) + outs:
        kept(a, 0)


# --------------------------------- b. fused placement over chunk edges ---
# (keys, mbits, ptindex, rank) pinned?
PLACE_PIN = {"pageable": (False, False, False, False), "keys-pinned": (True, False, False, False),
             "mbits-pinned": (False, True, False, False), "all-pinned": (True, True, True, True)}


def run_place(B, L, nptes, nranks, form):
    pk, pm, pp, pr = PLACE_PIN[form]
    n = 3 * per_of(L) + 17
    mb, pt, rk = sink(n, np.uint64, pm), sink(n, np.uint32, pp), sink(n, np.uint32, pr)
    P.place_batch_host(B.keys(L, n, pk), nptes, nranks, out=(mb, pt, rk))
    m2, p2, r2 = B.place(L, n, nptes, nranks)
    same(mb[:n], m2, f"mbits L={L} {form}")
    same(pt[:n], p2, f"ptindex L={L} {form}")
    same(rk[:n], r2, f"rank L={L} {form}")
    for a in (mb, pt, rk):
        kept(a, n, form)


@pytest.mark.parametrize("form", list(PLACE_PIN))
@pytest.mark.parametrize("L", [8, 13, 64])
def test_place_four_chunks(dev, B, L, form):
    """The three output arrays sit at [0, 8*per, 12*per) of one device buffer;
    the ragged last chunk copies cnt < per elements of each.  mbits-pinned:
    one direct DMA and two harvests in the same chunk; all-pinned: the
    zero-copy kernel."""
    run_place(B, L, 3, 1000, form)


def test_place_four_chunks_large_moduli(dev, B):
    run_place(B, 13, 0xFFFFFFFB, 0x7FFFFFED, "pageable")


def place_abi(lib, keys, L, n, nptes, nranks, mb, pt, rk, stride):
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    rc = lib.pdht_place_batch_host(ptr(keys), L, n, nptes, nranks, ptr(mb), ptr(pt), ptr(rk), stride, 0)
    assert rc == 0, lib.pdht_hip_last_error()


@pytest.mark.parametrize("form", ["pageable", "rank-pinned", "all-pinned"])
def test_place_strided_ranks_four_chunks(dev, B, form):
    """rank_stride = 8 (ptl_process_t[]): the 2-D copy of the rank column
    across 4 chunks into pageable memory, the same as a direct DMA into a
    pinned array, and the zero-copy kernel's strided sink.  The second u32 of
    every element keeps its sentinel."""
    L = 64
    n = 3 * per_of(L) + 17
    allp = form == "all-pinned"
    mb, pt = sink(n, np.uint64, allp), sink(n, np.uint32, allp)
    rk = sink(2 * n, np.uint32, form != "pageable")
    place_abi(P.lib(), B.keys(L, n, allp), L, n, 3, 1000, mb, pt, rk, 8)
    m2, p2, r2 = B.place(L, n, 3, 1000)
    same(mb[:n], m2, "mbits")
    same(pt[:n], p2, "ptindex")
    same(rk[:2 * n:2], r2, "rank")
    assert (rk[1:2 * n:2] == SENT[rk.dtype]).all(), "nid/pid half of a ptl_process_t overwritten"
    for a, used in ((mb, n), (pt, n), (rk, 2 * n)):
        kept(a, used, form)


@pytest.mark.parametrize("absent", ["ptindex", "rank"])
def test_place_null_output(dev, B, absent):
    """ptindex = NULL, and rank = NULL, at the host entry point: the other
    outputs are complete across the chunk edges, the absent one's array (not
    passed) is untouched."""
    L = 64
    n = 3 * per_of(L) + 17
    mb, pt, rk = sink(n, np.uint64), sink(n, np.uint32), sink(n, np.uint32)
    place_abi(P.lib(), B.keys(L, n), L, n, 3, 1000, mb, None if absent == "ptindex" else pt,
              None if absent == "rank" else rk, 4)
    m2, p2, r2 = B.place(L, n, 3, 1000)
    same(mb[:n], m2, "mbits")
    if absent == "ptindex":
        same(rk[:n], r2, "rank")
        kept(pt, 0)
    else:
        same(pt[:n], p2, "ptindex")
        kept(rk, 0)
    kept(mb, n)


def test_pdht_hash_batch_over_a_chunk_edge(dev, B, oracle):
    """pdht_hash_batch (the pdht_hash.c shim) on 2*per + 5 13-byte keys: 3
    chunks into ptl_process_t[] ranks.  The libmpipdht flavour writes mbits
    and rank only: ptindex and the nid/pid halves keep their sentinel across
    the chunk edges."""
    n = 2 * per_of(13) + 5
    k = B.keys(13, n)
    m2, p2, r2 = oracle.pdht_hash_fixed(k, 4, 10)
    mb, pt, rk = P.PdhtTable(keysize=13, nptes=4, nranks=10).hash_batch(k)
    same(mb, m2, "mbits")
    same(pt, p2, "ptindex")
    same(rk, r2, "rank")
    L = P.mpi_lib()
    t = P._PdhtT()
    L.pdht_hip_table_init(C.byref(t), 13, 4)
    C.c_int.in_dll(L, "pdht_hip_shim_nranks").value = 10
    mb, pt, rk = sink(n, np.uint64), sink(n, np.uint32), sink(2 * n, np.uint32)
    assert L.pdht_hash_batch(C.byref(t), k.ctypes.data, n, mb.ctypes.data, pt.ctypes.data, rk.ctypes.data,
                             0) == 0, L.pdht_hip_last_error()
    same(mb[:n], m2, "mpi mbits")
    same(rk[:2 * n:2], r2, "mpi rank")
    assert (rk[1:2 * n:2] == SENT[rk.dtype]).all() and (pt == SENT[pt.dtype]).all()
    kept(mb, n)
    kept(rk, 2 * n)


# ------------------------------ c. variable-length keys: planner edges ---
def plan(offsets, chunk=CHUNK, maxk=MAXK):
    """The greedy rule of host_var_chunks, restated: from key a, the most
    keys b - a <= maxk with offsets[b] - offsets[a] <= chunk, at least one."""
    n, a, out = len(offsets) - 1, 0, []
    while a < n:
        hi = min(n, a + maxk)
        fit = int(np.searchsorted(offsets[a + 1:hi + 1], offsets[a] + np.uint64(chunk), side="right"))
        b = max(a + 1, a + fit)
        out.append((a, b))
        a = b
    return out


def offsets_of(lens, first=0):
    off = np.empty(len(lens) + 1, np.uint64)
    off[0] = first
    np.cumsum(lens, out=off[1:])
    off[1:] += np.uint64(first)
    return off


def run_var(oracle, data, off):
    n = off.size - 1
    want = oracle.city64_var(data, off)
    out = sink(n, np.uint64)
    P.city64_var_batch_host(data, off, out=out)
    same(out[:n], want, "var")
    kept(out, n)


def test_var_key_cap_then_regrowth(dev, oracle):
    """5 000 000 keys of 0-7 bytes, then 740 000 keys of 16-256 bytes, then
    three empty keys; offsets[0] = 37.
      chunk 0 = keys [0, MAXK) and chunk 1 = [MAXK, 2*MAXK): cut by the key
        count, about 7 MB of bytes each;
      chunk 2 starts at key 2*MAXK = 4 194 304 inside the short keys, runs
        into the long ones and ends on the byte limit, as do chunks 3 and 4;
      chunk 5 is the rest and ends with the three empty keys.
    Chunks 3 and 4 reuse the slots of chunks 0 and 1 with about 4.5 times
    their bytes: the slots' input buffers grow in the middle of the batch,
    while the other slots are busy."""
    rng = np.random.default_rng(0xC0FFEE)
    short = rng.integers(0, 8, 5_000_000).astype(np.uint64)
    long_ = oracle.mixed_lengths(740_000)
    lens = np.concatenate([short, long_, np.zeros(3, np.uint64)])
    off = offsets_of(lens, 37)
    chunks = plan(off)
    nbytes = [int(off[b] - off[a]) for a, b in chunks]
    assert chunks[0] == (0, MAXK) and chunks[1] == (MAXK, 2 * MAXK) and len(chunks) == 6
    assert max(nbytes[:2]) < 8 << 20
    assert all(b - a < MAXK and CHUNK - 256 < nb <= CHUNK for (a, b), nb in zip(chunks[2:5], nbytes[2:5]))
    assert chunks[2][0] < 5_000_000 < chunks[2][1] and chunks[5][1] == lens.size
    data = oracle.splitmix64(oracle.SEED_KEYS, 11, (int(off[-1]) + 7) // 8).view(np.uint8)[:int(off[-1])]
    run_var(oracle, data, off)


def test_var_exact_byte_limit(dev, oracle):
    """20 000 keys of 4096 bytes: chunk c = keys [8192*c, 8192*(c+1)) holds
    exactly CHUNK bytes, offsets[b] == lim must be included.  With one
    4097-byte key first every edge falls one key earlier: [0, 8191),
    [8191, 16383), [16383, 20001)."""
    lens = np.full(20_000, 4096, np.uint64)
    off = offsets_of(lens)
    assert plan(off) == [(0, 8192), (8192, 16384), (16384, 20000)]
    data = oracle.fixed_keys(20_002, 4096).reshape(-1)
    run_var(oracle, data[:int(off[-1])], off)
    off = offsets_of(np.concatenate([np.array([4097], np.uint64), lens]))
    assert plan(off) == [(0, 8191), (8191, 16383), (16383, 20001)]
    run_var(oracle, data[:int(off[-1])], off)


def test_var_empty_keys_at_the_edge(dev, oracle):
    """The 4096-byte batch with runs of 70 empty keys (an empty key adds no
    byte, so the byte limit never splits a run: a chunk takes every empty key
    that follows its last full one):
      8160 full keys [0, 8160), then 70 empty keys [8160, 8230): the run
        straddles key 8192, the first edge of the batch without empty keys;
      32 full keys [8230, 8262): the chunk now holds exactly CHUNK bytes;
      70 empty keys [8262, 8332) exactly after the edge: their offsets equal
        the limit, so chunk 0 = [0, 8332) takes them all (140 keys of the
        chunk read no byte, the last 70 at d_in + CHUNK);
      8192 full keys [8332, 16524) and 70 empty ones: chunk 1 = [8332, 16594),
        exactly CHUNK bytes again;
      100 full and 70 empty keys: chunk 2 = [16594, 16764)."""
    F, E = 4096, 0
    lens = np.array([F] * 8160 + [E] * 70 + [F] * 32 + [E] * 70 + [F] * 8192 + [E] * 70 + [F] * 100 + [E] * 70,
                    np.uint64)
    off = offsets_of(lens)
    assert plan(off) == [(0, 8332), (8332, 16594), (16594, 16764)]
    assert int(off[8332] - off[0]) == CHUNK and int(off[8262]) == CHUNK
    data = oracle.fixed_keys(int(off[-1]) // F, F).reshape(-1)
    run_var(oracle, data, off)


@pytest.fixture(scope="module")
def mixed(oracle):
    """oracle.mixed_keys(1 << 20): about 136 MB in 5 chunks; the oracle's
    digests are computed once."""
    data, off = oracle.mixed_keys(1 << 20)
    assert len(plan(off)) == 5
    return data, off, oracle.city64_var(data, off)


@pytest.mark.parametrize("form", ["data-pinned", "out-pinned", "data-out-pinned"])
def test_var_pinning(dev, mixed, form):
    """Pageable offsets keep every form out of the zero-copy path: pinned
    data is DMA'd in place, pinned out is DMA'd in place, and with both
    pinned the pipeline runs with both DMA branches.  uint64 and int64
    offsets."""
    data, off, want = mixed
    n = off.size - 1
    d = pin_copy(data) if form != "out-pinned" else data
    for o in (off, off.astype(np.int64)):
        out = sink(n, np.uint64, form != "data-pinned")
        P.city64_var_batch_host(d, o, out=out)
        same(out[:n], want, f"{form} {o.dtype}")
        kept(out, n)


@pytest.mark.parametrize("pin", [False, True], ids=["pageable", "pinned"])
def test_var_misaligned_base(dev, mixed, pin):
    """The same keys from data[3:] of a buffer: every chunk starts at an odd
    host address, and on the device its first key at d_in + 0."""
    data, off, want = mixed
    n = off.size - 1
    buf = pinned(data.size + 3, np.uint8) if pin else np.empty(data.size + 3, np.uint8)
    buf[:3] = 0xEE
    buf[3:] = data
    assert buf[3:].ctypes.data % 2 == 1
    out = sink(n, np.uint64)
    P.city64_var_batch_host(buf[3:], off, out=out)
    same(out[:n], want, "data[3:]")
    kept(out, n)


# --------------------------------------------------- d. registered memory ---
def test_registered_memory(dev, B):
    """hipHostRegister'ed numpy buffers (the header's "registered"): whichever
    path the runtime's answer for such memory selects, every digest is right."""
    rt = torch.cuda.cudart()
    if not hasattr(rt, "cudaHostRegister") or not hasattr(rt, "cudaHostUnregister"):
        pytest.skip("torch.cuda.cudart() has no cudaHostRegister")
    L = 64
    n = per_of(L) + 5

    def page_aligned(nbytes):
        raw = np.empty(nbytes + 8192, np.uint8)
        skip = -raw.ctypes.data % 4096
        return raw[skip:skip + (nbytes + 4095) // 4096 * 4096]

    kb = page_aligned(n * L)
    ob = page_aligned((n + TAIL) * 8)
    kb[:n * L] = B.keys(L, n).reshape(-1)
    keys = kb[:n * L].reshape(n, L)
    out = ob[:(n + TAIL) * 8].view(np.uint64)
    out[:] = SENT[out.dtype]
    done = []
    try:
        for a in (kb, ob):
            rc = rt.cudaHostRegister(a.ctypes.data, a.nbytes, 0)
            assert int(rc) == 0, f"cudaHostRegister: {rc}"
            done.append(a)
        P.city64_batch_host(keys, out=out)
        same(out[:n], B.city64(L, n), "registered")
        kept(out, n)
    finally:
        for a in done:
            rt.cudaHostUnregister(a.ctypes.data)


# --------------------------------------------------- e. slots across calls ---
def test_slots_across_calls(dev, B, oracle):
    """One context, calls of different input and output widths in a row: the
    slots' buffers grow between calls (8 -> 16 -> 16*per bytes of output),
    shrink never, and no call sees what an earlier one left."""
    k1000 = B.keys(1000, 1000)
    out = sink(1000, np.uint64)
    first = P.city64_batch_host(k1000, out=out)[:1000].copy()          # 1
    same(first, B.city64(1000, 1000), "step 1")
    n = PER64 + 1
    o128 = sink(2 * n, np.uint64)
    P.citycrc128_batch_host(B.keys(64, n), out=o128)                   # 2
    same(o128[:2 * n], B.crc128(64, n), "step 2")
    kept(o128, 2 * n)
    n8 = per_of(8) + 1
    outs = (sink(n8, np.uint64), sink(n8, np.uint32), sink(n8, np.uint32))
    P.place_batch_host(B.keys(8, n8), 3, 1000, out=outs)               # 3
    for got, want, name in zip(outs, B.place(8, n8, 3, 1000), ("mbits", "ptindex", "rank")):
        same(got[:n8], want, "step 3 " + name)
        kept(got, n8)
    data, off = oracle.mixed_keys(300_000)
    ov = sink(300_000, np.uint64)
    P.city64_var_batch_host(data, off, out=ov)                         # 4
    same(ov[:300_000], oracle.city64_var(data, off), "step 4")
    kept(ov, 300_000)
    out[:] = SENT[out.dtype]
    P.city64_batch_host(B.keys(8, 1), out=out)                         # 5
    same(out[:1], B.city64(8, 1), "step 5")
    kept(out, 1)
    P.city64_batch_host(np.zeros((0, 8), np.uint8), out=out)           # 6
    same(out[:1], B.city64(8, 1), "step 6")
    kept(out, 1)
    kd = torch.from_numpy(B.keys(64, 5000)).to(dev)                    # 7
    same(P.city64_batch(kd).cpu().numpy().view(np.uint64), B.city64(64, 5000), "step 7")
    out[:] = SENT[out.dtype]
    P.city64_batch_host(k1000, out=out)
    same(out[:1000], first, "step 1 again")
    kept(out, 1000)


# ------------------------------------------------------------ f. two threads ---
def test_two_threads(dev, B, oracle):
    """Two threads enter the host path together (ctypes releases the GIL):
    one runs the pageable 4-chunk batch through the pipeline, the other a
    pinned zero-copy batch and then a pageable variable-length batch that
    waits for the pipeline's mutex.  Both run twice."""
    n = 3 * PER64 + 17
    ka, kb = B.keys(64, n), B.keys(64, PER64, pin=True)
    data, off = oracle.mixed_keys(300_000)
    want_a, want_b, want_v = B.city64(64, n), B.city64(64, PER64), oracle.city64_var(data, off)
    oa = [sink(n, np.uint64) for _ in range(2)]
    ob = [sink(PER64, np.uint64, pin=True) for _ in range(2)]
    ov = [sink(300_000, np.uint64) for _ in range(2)]
    gate = threading.Barrier(2, timeout=30)
    errors = []

    def guarded(fn):
        def run():
            try:
                gate.wait()
                for i in range(2):
                    fn(i)
            except BaseException as e:  # noqa: BLE001 -- reported by the main thread
                errors.append(repr(e))
        return threading.Thread(target=run, daemon=True)

    def a(i):
        P.city64_batch_host(ka, out=oa[i])

    def b(i):
        P.city64_batch_host(kb, out=ob[i])
        P.city64_var_batch_host(data, off, out=ov[i])

    threads = [guarded(a), guarded(b)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), "a host batch is still running after 60 s"
    assert not errors, errors
    for i in range(2):
        same(oa[i][:n], want_a, f"pipeline thread, run {i}")
        same(ob[i][:PER64], want_b, f"zero-copy, run {i}")
        same(ov[i][:300_000], want_v, f"var, run {i}")
        kept(oa[i], n)
        kept(ob[i], PER64)
        kept(ov[i], 300_000)


# ----------------------------------- g. errors leave the pipeline usable ---
@pytest.mark.parametrize("device", [64, -1])
def test_device_out_of_range_then_a_normal_batch(dev, B, device):
    n = PER64 + 1
    keys = B.keys(64, n)
    out = sink(n, np.uint64)
    with pytest.raises(P.PdhtError, match="out of range"):
        P.city64_batch_host(keys, out=out, device=device)
    kept(out, 0)
    # the zero-copy path checks the index too, before it switches devices
    pout = sink(1000, np.uint64, pin=True)
    with pytest.raises(P.PdhtError, match="out of range"):
        P.city64_batch_host(B.keys(64, 1000, pin=True), out=pout, device=device)
    kept(pout, 0)
    P.city64_batch_host(keys, out=out)
    same(out[:n], B.city64(64, n), "after the error")
    kept(out, n)
