"""CPU-side checks of the table's put and get by key (include/pdht_hip_table_keys.h; no GPU needed): the
exports of the three libraries, the header, the workspace sizes, every refusal of the two entry points --
each with its message and before any device call, so they hold on a machine without a GPU --, the empty
batch and its kernel tags, and the Python wrappers' own checks."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

import pdht_amd as P

NEW_SYMS = {"pdht_table_put_keys_workspace_bytes", "pdht_table_put_keys_dev", "pdht_table_get_keys_dev"}


# ------------------------------------------------------ exports and header ---
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


@pytest.mark.parametrize("path", [P.LIB_PATH, P.MPI_LIB_PATH, P.TUNING_LIB_PATH])
def test_every_library_exports_the_keys_entry_points(path):
    assert NEW_SYMS <= _exports(path)
    v = C.CDLL(path).pdht_hip_version
    v.restype = C.c_char_p
    assert b"abi 4" in v()


def test_keys_header_declares_what_the_libraries_export():
    text = open(os.path.join(ROOT, "include", "pdht_hip_table_keys.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{)]*\)\s*;", src))
    assert names == NEW_SYMS
    flat = re.sub(r"[\s*]+", " ", text)
    for tag in ('"k_table_claim_keys+k_table_write_keys<P>"', '"k_table_get_keys<P>"'):
        assert tag in flat
    assert "pdht_table_put_keys_workspace_bytes(m) = 4*m bytes" in re.sub(r"\s+\*?\s*", " ", text)
    top = open(os.path.join(ROOT, "include", "pdht_hip.h")).read()
    assert top.count('#include "pdht_hip_table_keys.h"') == 1
    assert "#define PDHT_HIP_ABI_VERSION 4" in top
    assert "_keys_dev" not in re.sub(r'#include "pdht_hip_table_keys.h"', "", top)  # no declaration of its own
    # the headers that list the kinds of batches behind counts4[2] name the keyed put
    for h in ("pdht_hip_table.h", "pdht_hip_table_rmw.h", "pdht_hip_table_acc.h", "pdht_hip_table_add.h"):
        assert "pdht_hip_table_keys.h" in open(os.path.join(ROOT, "include", h)).read(), h


def test_keys_header_compiles_as_c99_on_its_own_and_either_way_round(tmp_path):
    body = ("int main(void) { pdht_hip_stream_t s = 0; return pdht_table_put_keys_workspace_bytes(1) == 4 "
            "? pdht_table_put_keys_dev(0, 64, 16, 0, 8, 0, 0, 8, 8, 0, 0, 0, 0, 0, s) "
            ": pdht_table_get_keys_dev(0, 64, 16, 0, 8, 0, 0, 0, 8, 8, 0, 0, s); }\n")
    for heads in (("pdht_hip_table_keys.h",), ("pdht_hip.h", "pdht_hip_table_keys.h"),
                  ("pdht_hip_table_keys.h", "pdht_hip.h")):
        c = tmp_path / "t.c"
        c.write_text("".join(f'#include "{h}"\n' for h in heads) + body)
        p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                            "-I" + os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr


def test_workspace_bytes():
    for L in (P.lib(), P.mpi_lib()):
        for m in (0, 1, 3, 4, 5, 65, 4097, (1 << 32) - 1):
            assert L.pdht_table_put_keys_workspace_bytes(m) == 4 * m
            assert L.pdht_table_put_keys_workspace_bytes(m) == L.pdht_table_put_workspace_bytes(m)
    assert P.table_put_keys_workspace_bytes(0) == 0
    assert P.table_put_keys_workspace_bytes(4097) == 4 * 4097
    assert P.table_put_keys_workspace_bytes((1 << 32) - 1) == 4 * ((1 << 32) - 1)
    for m in (-1, 1 << 32):
        with pytest.raises(ValueError):
            P.table_put_keys_workspace_bytes(m)


# ------------------------------------------------------------- refusals ---
# Fake device addresses: every case below must be refused before anything dereferences them
TAB, KEYS, VALS, WS, ST, MB = 0x100000, 0x200000, 0x300000, 0x400000, 0x900000, 0xA00000


def _put(lib, *, table=TAB, capacity=64, rowbytes=24, keys=KEYS, keysize=13, key_slot=0, values=VALS, elemsize=8,
         value_stride=8, m=10, workspace=WS, ws_bytes=1 << 20, mbits=None, status=ST):
    return lib.pdht_table_put_keys_dev(table, capacity, rowbytes, keys, keysize, key_slot, values, elemsize,
                                       value_stride, m, workspace, ws_bytes, mbits, status, None)


def _get(lib, *, table=TAB, capacity=64, rowbytes=24, keys=KEYS, keysize=13, key_slot=0, values=VALS, elemsize=8,
         value_stride=8, m=10, mbits=None, status=ST):
    return lib.pdht_table_get_keys_dev(table, capacity, rowbytes, keys, keysize, key_slot, m, values, elemsize,
                                       value_stride, mbits, status, None)


GEOM = [
    (dict(capacity=0), "table: capacity must be a power of two"),
    (dict(capacity=100), "table: capacity must be a power of two"),
    (dict(capacity=32), "table: capacity must be a power of two"),
    (dict(capacity=1 << 32), "table: capacity must be a power of two"),
    (dict(rowbytes=0), "table: rowbytes must be a multiple of 8"),
    (dict(rowbytes=12), "table: rowbytes must be a multiple of 8"),
    (dict(rowbytes=1 << 31), "table: rowbytes must be a multiple of 8"),
    (dict(table=None), "table: table must not be NULL"),
    (dict(table=TAB + 8), "table: table must be 16-byte aligned"),
]
ROW = "table {}: rowbytes must be slot + elemsize rounded up to 8"
SLOT = "table {}: key_slot must be 0 or a multiple of 8 that is >= keysize"
# refusals that both calls share; {} = the call's name
BOTH = GEOM + [
    (dict(m=1 << 32, ws_bytes=1 << 40), "table {}: m must be < 2^32"),
    (dict(keysize=0), "table {}: keysize must be >= 1"),
    (dict(keysize=65, rowbytes=80), "table {}: keysize must be <= 64; longer keys go through pdht_bucket_put_records_dev"),
    (dict(keysize=65, key_slot=72, rowbytes=80), "table {}: keysize must be <= 64"),
    (dict(key_slot=12), SLOT),
    (dict(key_slot=20), SLOT),
    (dict(key_slot=8), SLOT),       # a multiple of 8, but < keysize 13
    (dict(keysize=33, key_slot=32, rowbytes=40), SLOT),
    (dict(elemsize=0), "table {}: elemsize must be >= 1"),
    (dict(elemsize=0, rowbytes=16), "table {}: elemsize must be >= 1"),
    (dict(rowbytes=16), ROW),       # slot 16 + 8
    (dict(rowbytes=32), ROW),
    (dict(elemsize=9, value_stride=9), ROW),   # 16 + 9 -> 32
    (dict(key_slot=32), ROW),       # 32 + 8 = 40
    (dict(keysize=17), ROW),        # (keysize 16 holds: 16 + 8 = 24) slot 24 + 8 = 32
    (dict(value_stride=7), "table {}: value_stride must be >= elemsize"),
    (dict(value_stride=0), "table {}: value_stride must be >= elemsize"),
    (dict(mbits=MB + 4), "table {}: mbits_out must be 8-byte aligned"),
    (dict(keys=None), "table {}: keys must not be NULL"),
    (dict(values=None), "table {}: values must not be NULL"),
]


@pytest.mark.parametrize("kw,msg", BOTH + [
    (dict(workspace=WS + 2), "table {}: workspace must be 4-byte aligned"),
    (dict(workspace=WS + 1), "table {}: workspace must be 4-byte aligned"),
    (dict(ws_bytes=39), "table {}: workspace too small (40 bytes needed)"),
    (dict(ws_bytes=0), "table {}: workspace too small (40 bytes needed)"),
    (dict(m=4097, ws_bytes=4 * 4097 - 1), "table {}: workspace too small (16388 bytes needed)"),
    (dict(workspace=None), "table {}: workspace must not be NULL"),
])
def test_put_keys_abi_refuses(kw, msg):
    lib = P.lib()
    assert _put(lib, **kw) != 0
    assert lib.pdht_hip_last_error().startswith(msg.format("put_keys").encode()), lib.pdht_hip_last_error()


@pytest.mark.parametrize("kw,msg", BOTH + [
    (dict(status=None), "table {}: status must not be NULL"),
])
def test_get_keys_abi_refuses(kw, msg):
    lib = P.lib()
    kw = {k: v for k, v in kw.items() if k != "ws_bytes"}
    assert _get(lib, **kw) != 0
    assert lib.pdht_hip_last_error().startswith(msg.format("get_keys").encode()), lib.pdht_hip_last_error()


def test_the_long_key_refusal_names_the_record_route():
    lib = P.lib()
    assert _put(lib, keysize=65, rowbytes=80) != 0
    for name in (b"pdht_bucket_put_records_dev", b"pdht_table_put_records_dev"):
        assert name in lib.pdht_hip_last_error()
    assert _get(lib, keysize=65, rowbytes=80) != 0
    for name in (b"pdht_bucket_records_dev", b"pdht_table_get_dev", b"pdht_get_resolve_dev"):
        assert name in lib.pdht_hip_last_error()


def test_geometries_that_pass():
    """What the refusals above must not catch: every key length of 1 .. 64 with its own slot and with the
    slots 32 and 64, status and mbits_out as they may be."""
    lib = P.lib()
    for L in range(1, 65):
        for key_slot in (0, 32, 64):
            if key_slot and key_slot < L:
                continue
            slot = key_slot or (L + 7) // 8 * 8
            for E in (1, 8, 24):
                kw = dict(keysize=L, key_slot=key_slot, elemsize=E, value_stride=E, rowbytes=(slot + E + 7) // 8 * 8, m=0)
                assert _put(lib, **kw) == 0, lib.pdht_hip_last_error()
                assert _get(lib, **kw) == 0, lib.pdht_hip_last_error()
    assert _put(lib, m=0, status=None, mbits=MB) == 0


def test_empty_batches_launch_nothing_and_name_their_kernels():
    """m == 0 returns 0 without a device call (none is possible here) and names what would have run: the put's
    row pieces by rowbytes alone (the table's rows are the only vector accesses with an alignment of their
    own), the get's value pieces by rowbytes, slot, values, value_stride and elemsize."""
    lib = P.lib()
    pair = b"k_table_claim_keys+k_table_write_keys<%d>"
    assert _put(lib, m=0) == 0 and lib.pdht_hip_last_kernel() == pair % 8        # rowbytes 24
    assert _put(lib, m=0, keys=None, values=None, workspace=None, ws_bytes=0, status=None) == 0
    assert lib.pdht_hip_last_kernel() == pair % 8
    assert _put(lib, m=0, rowbytes=32, elemsize=16, value_stride=16) == 0 and lib.pdht_hip_last_kernel() == pair % 16
    assert _put(lib, m=0, rowbytes=32, elemsize=9, value_stride=11, values=VALS + 1) == 0
    assert lib.pdht_hip_last_kernel() == pair % 16
    get = b"k_table_get_keys<%d>"
    for kw, piece in ((dict(), 8),                                                     # slot 16, rowbytes 24
                      (dict(rowbytes=32, elemsize=16, value_stride=16), 16),
                      (dict(rowbytes=32, elemsize=16, value_stride=24), 8),
                      (dict(rowbytes=32, elemsize=16, value_stride=16, values=VALS + 8), 8),
                      (dict(rowbytes=48, elemsize=32, value_stride=32), 16),
                      (dict(keysize=8, rowbytes=24, elemsize=16, value_stride=16), 8),  # slot 8
                      (dict(rowbytes=32, elemsize=12, value_stride=12), 4),
                      (dict(value_stride=12), 4),
                      (dict(values=VALS + 4), 4),
                      (dict(values=VALS + 1), 1),
                      (dict(value_stride=9), 1),
                      (dict(rowbytes=32, elemsize=9, value_stride=16), 1)):
        assert _get(lib, m=0, **kw) == 0, lib.pdht_hip_last_error()
        assert lib.pdht_hip_last_kernel() == get % piece, kw
    assert _get(lib, m=0, keys=None, values=None, status=None) == 0


# ------------------------------------------------------------- wrappers ---
def _bare_table(rowbytes=24):
    t = object.__new__(P.DeviceTable)  # the methods' own checks, without a device behind them
    t.capacity, t.rowbytes, t.device = 64, rowbytes, torch.device("cuda:0")
    return t


def test_keys_wrappers_check_their_arguments_before_c():
    t = _bare_table()
    u8 = torch.uint8
    with pytest.raises(ValueError, match="values"):
        t.put_keys(torch.zeros((4, 13), dtype=u8), torch.zeros((4, 8), dtype=u8))  # CPU values
    with pytest.raises(ValueError, match="values"):
        t.put_keys(None, torch.zeros(32, dtype=u8))  # not [m, E]
    with pytest.raises(ValueError, match="values"):
        t.put_keys(None, None)
    for call in (lambda k: t.get_keys(k, 8), lambda k: t.get_keys(k, 8, key_slot=16)):
        with pytest.raises(ValueError, match="keys"):
            call(torch.zeros((4, 13), dtype=u8))  # CPU keys
        with pytest.raises(ValueError, match="keys"):
            call(torch.zeros(52, dtype=u8))
        with pytest.raises(ValueError, match="keys"):
            call(torch.zeros((4, 13), dtype=torch.int64))
        with pytest.raises(ValueError, match="keys"):
            call(None)
    def shape(f):  # (name, kind, default) of every parameter
        return [(p.name, p.kind.name, p.default) for p in inspect.signature(f).parameters.values()]

    pos, kw, none = "POSITIONAL_OR_KEYWORD", "KEYWORD_ONLY", inspect.Parameter.empty
    assert shape(P.DeviceTable.put_keys) == [
        ("self", pos, none), ("keys", pos, none), ("values", pos, none), ("key_slot", kw, 0), ("status", kw, True),
        ("mbits", kw, None), ("workspace", kw, None), ("stream", kw, None)]
    assert shape(P.DeviceTable.get_keys) == [
        ("self", pos, none), ("keys", pos, none), ("elemsize", pos, none), ("key_slot", kw, 0), ("values", kw, None),
        ("status", kw, None), ("mbits", kw, None), ("stream", kw, None)]
    assert "table_put_keys_workspace_bytes" in P.__all__
