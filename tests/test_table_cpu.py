"""CPU-side checks of the device-resident table (no GPU needed): the size
queries, the argument checks of the C ABI -- every one refused with a message
before any device call, so they hold on a machine without a GPU -- the exports
of the three libraries (include/pdht_hip_table.h), the Python wrappers' own
checks, and dist.exchange_replies as the inverse of dist.exchange_records
under gloo."""
import ctypes as C
import os
import re
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

import pdht_amd as P


# ----------------------------------------------------------- size queries ---
@pytest.mark.parametrize("capacity", [64, 16384, 1 << 25, 1 << 31])
@pytest.mark.parametrize("rowbytes", [8, 16, 40, 64, 288])
def test_table_bytes(capacity, rowbytes):
    want = 64 + (capacity + 1) * (16 + rowbytes)  # counters | tags | winner words | rows, one private slot
    assert P.table_bytes(capacity, rowbytes) == want
    assert P.lib().pdht_table_bytes(capacity, rowbytes) == want


@pytest.mark.parametrize("capacity,rowbytes", [(0, 8), (32, 8), (63, 8), (96, 8), (1 << 32, 8), ((1 << 31) + 64, 8),
                                               (64, 0), (64, 4), (64, 12), (64, 1 << 31), (64, (1 << 31) + 8)])
def test_table_bytes_refuses(capacity, rowbytes):
    assert P.lib().pdht_table_bytes(capacity, rowbytes) == 0
    with pytest.raises(ValueError):
        P.table_bytes(capacity, rowbytes)


def test_reply_and_workspace_bytes():
    lib = P.lib()
    for head in (1, 8):
        for B in (8, 16, 40, 288):
            assert P.table_reply_bytes(head, B) == lib.pdht_table_reply_bytes(head, B) == head + B
    assert P.table_reply_bytes(1, 32 + 8) == 41  # reply_t {char status; char key[32]} + an 8-byte value
    for head, B in ((0, 8), (2, 8), (4, 8), (16, 8), (8, 0), (8, 12), (1, 1 << 31)):
        assert lib.pdht_table_reply_bytes(head, B) == 0
        with pytest.raises(ValueError):
            P.table_reply_bytes(head, B)
    for m in (0, 1, 65, (1 << 32) - 1):
        assert lib.pdht_table_put_workspace_bytes(m) == 4 * m


# ------------------------------------------------------------- refusals ---
# Fake device addresses: every case below must be refused before anything dereferences them
TAB, REC, WS, MB, REP, KEYS, IDX, VALS, ST = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, \
    0x700000, 0x800000, 0x900000

GEOM = [
    (dict(capacity=0), b"capacity must be a power of two"),
    (dict(capacity=32), b"capacity must be a power of two"),
    (dict(capacity=100), b"capacity must be a power of two"),
    (dict(capacity=1 << 32), b"capacity must be a power of two"),
    (dict(rowbytes=0), b"rowbytes must be a multiple of 8"),
    (dict(rowbytes=12), b"rowbytes must be a multiple of 8"),
    (dict(rowbytes=1 << 31), b"rowbytes must be a multiple of 8"),
    (dict(table=None), b"table must not be NULL"),
    (dict(table=TAB + 8), b"table must be 16-byte aligned"),
]


def _init(lib, *, table=TAB, table_bytes=None, capacity=64, rowbytes=16):
    if table_bytes is None:
        table_bytes = 64 + (capacity + 1) * (16 + rowbytes)
    return lib.pdht_table_init_dev(table, table_bytes, capacity, rowbytes, None)


@pytest.mark.parametrize("kw,msg", GEOM + [(dict(table_bytes=64 + 65 * 32 - 1), b"table_bytes too small")])
def test_table_init_abi_refuses(kw, msg):
    lib = P.lib()
    assert _init(lib, **kw) != 0
    assert msg in lib.pdht_hip_last_error(), lib.pdht_hip_last_error()


def _put(lib, *, table=TAB, capacity=64, rowbytes=16, records=REC, record_stride=40, m=10, workspace=WS,
         ws_bytes=1 << 20, status=ST):
    return lib.pdht_table_put_records_dev(table, capacity, rowbytes, records, record_stride, m, workspace, ws_bytes,
                                          status, None)


@pytest.mark.parametrize("kw,msg", GEOM + [
    (dict(m=1 << 32, ws_bytes=1 << 40), b"m must be < 2^32"),
    (dict(record_stride=32), b"record_stride must be a multiple of 8 and >= 24 + rowbytes"),
    (dict(record_stride=44), b"record_stride must be a multiple of 8 and >= 24 + rowbytes"),
    (dict(records=REC + 4), b"records must be 8-byte aligned"),
    (dict(records=None), b"records must not be NULL"),
    (dict(workspace=None), b"workspace must not be NULL"),
    (dict(ws_bytes=39), b"workspace too small"),
])
def test_table_put_abi_refuses(kw, msg):
    lib = P.lib()
    assert _put(lib, **kw) != 0
    assert msg in lib.pdht_hip_last_error(), lib.pdht_hip_last_error()


def _get(lib, *, table=TAB, capacity=64, rowbytes=16, mbits=MB, mbits_stride=8, m=10, replies=REP, reply_stride=24,
         head=8):
    return lib.pdht_table_get_dev(table, capacity, rowbytes, mbits, mbits_stride, m, replies, reply_stride, head,
                                  None)


@pytest.mark.parametrize("kw,msg", GEOM + [
    (dict(m=1 << 32), b"m must be < 2^32"),
    (dict(mbits=MB + 4), b"mbits must be 8-byte aligned"),
    (dict(mbits_stride=0), b"mbits_stride must be a multiple of 8 and >= 8"),
    (dict(mbits_stride=4), b"mbits_stride must be a multiple of 8 and >= 8"),
    (dict(mbits_stride=12), b"mbits_stride must be a multiple of 8 and >= 8"),
    (dict(head=0), b"head must be 1 or 8"),
    (dict(head=4), b"head must be 1 or 8"),
    (dict(reply_stride=23), b"reply_stride must be >= head + rowbytes"),
    (dict(head=1, reply_stride=16), b"reply_stride must be >= head + rowbytes"),
    (dict(mbits=None), b"mbits must not be NULL"),
    (dict(replies=None), b"replies must not be NULL"),
])
def test_table_get_abi_refuses(kw, msg):
    lib = P.lib()
    assert _get(lib, **kw) != 0
    assert msg in lib.pdht_hip_last_error(), lib.pdht_hip_last_error()


def _resolve(lib, *, replies=REP, reply_stride=24, head=8, value_offset=8, keys=KEYS, keysize=8, index=IDX,
             index_stride=4, m=10, values=VALS, elemsize=8, value_stride=8, status=ST):
    return lib.pdht_get_resolve_dev(replies, reply_stride, head, value_offset, keys, keysize, index, index_stride, m,
                                    values, elemsize, value_stride, status, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(m=1 << 32), b"m must be < 2^32"),
    (dict(head=2), b"head must be 1 or 8"),
    (dict(keysize=0), b"keysize must be >= 1"),
    (dict(elemsize=0, value_stride=0), b"elemsize must be >= 1"),
    (dict(elemsize=16, value_stride=12, reply_stride=32), b"value_stride must be >= elemsize"),
    (dict(reply_stride=23), b"reply_stride must hold"),
    (dict(keysize=32), b"reply_stride must hold"),
    (dict(index_stride=0), b"index_stride"),
    (dict(index_stride=2), b"index_stride"),
    (dict(index_stride=6), b"index_stride"),
    (dict(index=IDX + 2), b"index must be 4-byte aligned"),
    (dict(replies=None), b"null replies, keys, values or status"),
    (dict(keys=None), b"null replies, keys, values or status"),
    (dict(values=None), b"null replies, keys, values or status"),
    (dict(status=None), b"null replies, keys, values or status"),
])
def test_get_resolve_abi_refuses(kw, msg):
    lib = P.lib()
    assert _resolve(lib, **kw) != 0
    assert msg in lib.pdht_hip_last_error(), lib.pdht_hip_last_error()


def test_empty_batches_launch_nothing():
    """m == 0 returns 0 without a device call (none is possible here), and names what would have run."""
    lib = P.lib()
    assert _put(lib, m=0, records=None, workspace=None, ws_bytes=0, status=None) == 0
    assert lib.pdht_hip_last_kernel() == b"k_table_claim+k_table_write<8>"
    assert _get(lib, m=0, mbits=None, replies=None) == 0
    assert lib.pdht_hip_last_kernel() == b"k_table_get<8>"
    assert _get(lib, m=0, mbits=None, replies=None, head=1, reply_stride=17) == 0
    assert lib.pdht_hip_last_kernel() == b"k_table_get_bytes"
    assert _resolve(lib, m=0, replies=None, keys=None, values=None, status=None, index=None) == 0
    assert lib.pdht_hip_last_kernel() == b"k_get_resolve<8>"


# ------------------------------------------------------ exports and header ---
NEW_SYMS = {"pdht_table_bytes", "pdht_table_init_dev", "pdht_table_put_workspace_bytes",
            "pdht_table_put_records_dev", "pdht_table_reply_bytes", "pdht_table_get_dev", "pdht_table_counts_dev",
            "pdht_get_resolve_dev"}


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


@pytest.mark.parametrize("path", [P.LIB_PATH, P.MPI_LIB_PATH, P.TUNING_LIB_PATH])
def test_every_library_exports_the_table_entry_points(path):
    assert NEW_SYMS <= _exports(path)
    v = C.CDLL(path).pdht_hip_version
    v.restype = C.c_char_p
    assert b"abi 4" in v()


def test_table_header_declares_what_the_libraries_export():
    src = open(os.path.join(ROOT, "include", "pdht_hip_table.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{)]*\)\s*;", src))
    assert names == NEW_SYMS
    top = open(os.path.join(ROOT, "include", "pdht_hip.h")).read()
    assert top.count('#include "pdht_hip_table.h"') == 1
    assert "#define PDHT_HIP_ABI_VERSION 4" in top


def test_table_header_compiles_as_c99_either_way_round(tmp_path):
    for first, second in (("pdht_hip.h", "pdht_hip_table.h"), ("pdht_hip_table.h", "pdht_hip.h")):
        c = tmp_path / "t.c"
        c.write_text(f'#include "{first}"\n#include "{second}"\n'
                     "int main(void) { pdht_hip_stream_t s = 0; return pdht_table_bytes(64, 8) == 1624 && "
                     "pdht_table_reply_bytes(8, 8) == 16 && pdht_table_put_workspace_bytes(1) == 4 "
                     "? pdht_table_init_dev(0, 0, 64, 8, s) + pdht_table_put_records_dev(0, 64, 8, 0, 32, 0, 0, 0, 0, s) "
                     "+ pdht_table_get_dev(0, 64, 8, 0, 8, 0, 0, 16, 8, s) + pdht_table_counts_dev(0, 0, s) "
                     "+ pdht_get_resolve_dev(0, 16, 8, 8, 0, 8, 0, 4, 0, 0, 8, 8, 0, s) : 1; }\n")
        p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                            "-I" + os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr


# ------------------------------------------------------------- wrappers ---
def test_wrappers_check_before_c():
    """Device, dtype and shape are checked in Python (no GPU needed)."""
    for name in ("table_bytes", "table_reply_bytes", "DeviceTable", "get_resolve"):
        assert name in P.__all__
    with pytest.raises(ValueError):
        P.DeviceTable(64, 16, device="cpu")
    with pytest.raises(ValueError):
        P.DeviceTable(64, 16, storage=torch.zeros(P.table_bytes(64, 16), dtype=torch.uint8))  # a CPU tensor
    with pytest.raises(ValueError):
        P.DeviceTable(100, 16)  # geometry is refused before any allocation
    with pytest.raises(ValueError):
        P.DeviceTable(64, 12)
    t = object.__new__(P.DeviceTable)  # the methods' own checks, without a device behind them
    t.capacity, t.rowbytes, t.device = 64, 16, torch.device("cuda:0")
    with pytest.raises(ValueError):
        t.put_records(torch.zeros((4, 40), dtype=torch.uint8))  # CPU records
    with pytest.raises(ValueError):
        t.get(torch.zeros(4, dtype=torch.int64))  # CPU mbits
    with pytest.raises(ValueError, match="1-D int64"):
        t.get(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="1-D int64"):
        t.get(torch.zeros((4, 2), dtype=torch.int64))
    with pytest.raises(ValueError):
        t.get(torch.zeros(4, dtype=torch.int64), head=4)
    k = torch.zeros((4, 8), dtype=torch.uint8)
    with pytest.raises(ValueError):
        P.get_resolve(torch.zeros((4, 24), dtype=torch.uint8), k, 8)  # CPU replies
    with pytest.raises(ValueError):
        P.get_resolve(torch.zeros(96, dtype=torch.uint8), k, 8)  # not [m, reply bytes]


# --------------------------------------------------------- exchange_replies ---
N_PER = 500
RB = 40  # bucket_record_bytes(8) + 8: a record with a little payload
REPLY = 24


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _records(rank, world):
    """Rank `rank`'s forged record batch in bucket order and its offsets: mbits = a splitmix-like mix of
    the global index, owner = mbits % world."""
    g = np.arange(N_PER, dtype=np.uint64) + np.uint64(rank * N_PER)
    mb = (g + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) ^ (g << np.uint64(7))
    rk = (mb % np.uint64(world)).astype(np.int64)
    order = np.argsort(rk, kind="stable")
    offs = np.concatenate([[0], np.cumsum(np.bincount(rk, minlength=world))]).astype(np.int64)
    rec = np.zeros((N_PER, RB), np.uint8)
    rec[:, 4:8] = np.frombuffer(np.uint32(rank).tobytes(), np.uint8)
    rec[:, 12:16] = order.astype(np.uint32).view(np.uint8).reshape(-1, 4)
    rec[:, 16:24] = mb[order].view(np.uint8).reshape(-1, 8)
    return rec, offs


def _worker(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pdht_amd import dist as D
        rec, offs = _records(rank, world)
        offs_t = torch.from_numpy(offs)
        mine, counts = D.exchange_records(torch.from_numpy(rec), offs_t)
        # the owner's answer to each record where it stands: {owner, source rank, source index, mbits}
        a = mine.numpy()
        rep = np.zeros((a.shape[0], REPLY), np.uint8)
        rep[:, 0:4] = np.frombuffer(np.uint32(rank).tobytes(), np.uint8)
        rep[:, 4:8] = a[:, 4:8]
        rep[:, 8:16] = a[:, 16:24]
        rep[:, 16:20] = a[:, 12:16]
        back = D.exchange_replies(torch.from_numpy(rep), offs_t, counts)
        q.put({"rank": rank, "back": back.numpy(), "received": a.shape[0]})
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("WORLD", [1, 3])
def test_exchange_replies_inverts_exchange_records(WORLD):
    """Each rank gets back one reply per record it sent, in its bucket order: reply p answers record p."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(WORLD)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sum(r["received"] for r in res) == WORLD * N_PER
    for r in res:
        rec, offs = _records(r["rank"], WORLD)
        back = r["back"]
        assert back.shape == (N_PER, REPLY)
        owner = back[:, 0:4].copy().view(np.uint32).ravel()
        assert (owner == np.repeat(np.arange(WORLD), np.diff(offs))).all()  # answered by the bucket's rank
        assert (back[:, 4:8].copy().view(np.uint32).ravel() == r["rank"]).all()
        assert (back[:, 8:16] == rec[:, 16:24]).all()   # the mbits of record p
        assert (back[:, 16:20] == rec[:, 12:16]).all()  # and its source index

