"""CPU-side checks of the table's update, insert-if-absent and compare-and-swap by key
(include/pdht_hip_table_keys_rmw.h; no GPU needed): the exports of the three libraries, the header, the
workspace sizes, every refusal of the three entry points -- each with its message and before any device
call, so they hold on a machine without a GPU --, the empty batches and their kernel tags, and the Python
wrappers' own checks."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

import pdht_amd as P

NEW_SYMS = {"pdht_table_update_keys_workspace_bytes", "pdht_table_update_keys_dev",
            "pdht_table_add_keys_workspace_bytes", "pdht_table_add_keys_dev",
            "pdht_table_cswap_keys_workspace_bytes", "pdht_table_cswap_keys_dev"}
HEADER = "pdht_hip_table_keys_rmw.h"


# ------------------------------------------------------ exports and header ---
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


@pytest.mark.parametrize("path", [P.LIB_PATH, P.MPI_LIB_PATH, P.TUNING_LIB_PATH])
def test_every_library_exports_the_six_entry_points(path):
    assert NEW_SYMS <= _exports(path)
    v = C.CDLL(path).pdht_hip_version
    v.restype = C.c_char_p
    assert b"abi 4" in v()


def test_header_declares_what_the_libraries_export():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{)]*\)\s*;", src))
    assert names == NEW_SYMS
    flat = re.sub(r"[\s*]+", " ", text)
    for tag in ('"k_table_locate_keys<last>+k_table_write_keys<P>"', '"k_table_locate_keys<first>+k_table_cswap"',
                '"k_table_add_claim_keys+k_table_add_write_keys<P>"'):
        assert tag in flat
    top = open(os.path.join(ROOT, "include", "pdht_hip.h")).read()
    assert top.count(f'#include "{HEADER}"') == 1
    assert "#define PDHT_HIP_ABI_VERSION 4" in top
    assert "_keys_dev" not in top  # no declaration of its own, and none in a comment
    # the headers that list the kinds of batches behind counts4[2] name the three new kinds
    for h in ("pdht_hip_table.h", "pdht_hip_table_rmw.h", "pdht_hip_table_acc.h", "pdht_hip_table_add.h",
              "pdht_hip_table_keys.h"):
        assert HEADER in open(os.path.join(ROOT, "include", h)).read(), h


def test_header_compiles_as_c99_on_its_own_and_either_way_round(tmp_path):
    body = ("int main(void) { pdht_hip_stream_t s = 0; return pdht_table_update_keys_workspace_bytes(1) == 4 "
            "? pdht_table_update_keys_dev(0, 64, 16, 0, 8, 0, 0, 8, 8, 0, 0, 0, 0, 0, s) "
            "+ pdht_table_add_keys_dev(0, 64, 16, 0, 8, 0, 0, 8, 8, 0, 0, pdht_table_add_keys_workspace_bytes(0), 0, 0, s) "
            ": pdht_table_cswap_keys_dev(0, 64, 16, 0, 8, 0, 8, 1u, 2u, 0, 16, 0, "
            "pdht_table_cswap_keys_workspace_bytes(0), 0, s); }\n")
    for heads in ((HEADER,), ("pdht_hip.h", HEADER), (HEADER, "pdht_hip.h")):
        c = tmp_path / "t.c"
        c.write_text("".join(f'#include "{h}"\n' for h in heads) + body)
        p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                            "-I" + os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr


def test_workspace_bytes():
    for L in (P.lib(), P.mpi_lib()):
        for m in (0, 1, 3, 4, 5, 65, 4097, (1 << 32) - 1):
            assert L.pdht_table_update_keys_workspace_bytes(m) == 4 * m
            assert L.pdht_table_update_keys_workspace_bytes(m) == L.pdht_table_update_workspace_bytes(m)
            assert L.pdht_table_cswap_keys_workspace_bytes(m) == 4 * m
            assert L.pdht_table_cswap_keys_workspace_bytes(m) == L.pdht_table_cswap_workspace_bytes(m)
            assert L.pdht_table_add_keys_workspace_bytes(m) == 4 * m + ((m + 3) & ~3)
            assert L.pdht_table_add_keys_workspace_bytes(m) == L.pdht_table_add_workspace_bytes(m)
    for f, want in ((P.table_update_keys_workspace_bytes, lambda m: 4 * m),
                    (P.table_cswap_keys_workspace_bytes, lambda m: 4 * m),
                    (P.table_add_keys_workspace_bytes, lambda m: 4 * m + (m + 3) // 4 * 4)):
        for m in (0, 1, 4097, (1 << 32) - 1):
            assert f(m) == want(m)
        for m in (-1, 1 << 32):
            with pytest.raises(ValueError):
                f(m)
        assert f.__name__ in P.__all__


# ------------------------------------------------------------- refusals ---
# Fake device addresses: every case below must be refused before anything dereferences them
TAB, KEYS, VALS, WS, ST, MB, REP = 0x100000, 0x200000, 0x300000, 0x400000, 0x900000, 0xA00000, 0xB00000


def _rows(op, lib, *, table=TAB, capacity=64, rowbytes=24, keys=KEYS, keysize=13, key_slot=0, values=VALS,
          elemsize=8, value_stride=8, m=10, workspace=WS, ws_bytes=1 << 20, mbits=None, status=ST):
    f = getattr(lib, f"pdht_table_{op}_dev")
    return f(table, capacity, rowbytes, keys, keysize, key_slot, values, elemsize, value_stride, m, workspace, ws_bytes,
             mbits, status, None)


def _cswap(lib, *, table=TAB, capacity=64, rowbytes=24, keys=KEYS, keysize=13, m=10, word_offset=16, compare=0,
           desired=1, replies=REP, reply_stride=16, workspace=WS, ws_bytes=1 << 20, mbits=None):
    return lib.pdht_table_cswap_keys_dev(table, capacity, rowbytes, keys, keysize, m, word_offset, compare, desired,
                                         replies, reply_stride, workspace, ws_bytes, mbits, None)


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
# what update_keys and add_keys share with put_keys; {} = the call's name
ROWS = GEOM + [
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
    (dict(keysize=17), ROW),        # slot 24 + 8 = 32
    (dict(value_stride=7), "table {}: value_stride must be >= elemsize"),
    (dict(value_stride=0), "table {}: value_stride must be >= elemsize"),
    (dict(mbits=MB + 4), "table {}: mbits_out must be 8-byte aligned"),
    (dict(keys=None), "table {}: keys must not be NULL"),
    (dict(values=None), "table {}: values must not be NULL"),
    (dict(workspace=WS + 2), "table {}: workspace must be 4-byte aligned"),
    (dict(workspace=WS + 1), "table {}: workspace must be 4-byte aligned"),
    (dict(workspace=None), "table {}: workspace must not be NULL"),
]


@pytest.mark.parametrize("kw,msg", ROWS + [
    (dict(ws_bytes=39), "table {}: workspace too small (40 bytes needed)"),
    (dict(ws_bytes=0), "table {}: workspace too small (40 bytes needed)"),
    (dict(m=4097, ws_bytes=4 * 4097 - 1), "table {}: workspace too small (16388 bytes needed)"),
])
def test_update_keys_abi_refuses(kw, msg):
    lib = P.lib()
    assert _rows("update_keys", lib, **kw) != 0
    assert lib.pdht_hip_last_error().startswith(msg.format("update_keys").encode()), lib.pdht_hip_last_error()


@pytest.mark.parametrize("kw,msg", ROWS + [
    (dict(ws_bytes=51), "table {}: workspace too small (52 bytes needed)"),   # 40 + 10 -> 12
    (dict(ws_bytes=40), "table {}: workspace too small (52 bytes needed)"),   # the update's size is not enough
    (dict(ws_bytes=0), "table {}: workspace too small (52 bytes needed)"),
    (dict(m=4097, ws_bytes=5 * 4097 + 2), "table {}: workspace too small (20488 bytes needed)"),
])
def test_add_keys_abi_refuses(kw, msg):
    lib = P.lib()
    assert _rows("add_keys", lib, **kw) != 0
    assert lib.pdht_hip_last_error().startswith(msg.format("add_keys").encode()), lib.pdht_hip_last_error()


WORD = "table cswap_keys: word_offset must be a multiple of 8 and <= rowbytes - 8"
STRIDE = "table cswap_keys: reply_stride must be a multiple of 8 and >= 16"


@pytest.mark.parametrize("kw,msg", GEOM + [
    (dict(m=1 << 32, ws_bytes=1 << 40), "table cswap_keys: m must be < 2^32"),
    (dict(keysize=0), "table cswap_keys: keysize must be >= 1"),
    (dict(keysize=65), "table cswap_keys: keysize must be <= 64; longer keys go through pdht_bucket_records_dev"),
    (dict(word_offset=4), WORD),
    (dict(word_offset=24), WORD),
    (dict(word_offset=(1 << 64) - 8), WORD),
    (dict(rowbytes=8, word_offset=8), WORD),
    (dict(replies=REP + 4), "table cswap_keys: replies must be 8-byte aligned"),
    (dict(reply_stride=8), STRIDE),
    (dict(reply_stride=0), STRIDE),
    (dict(reply_stride=20), STRIDE),
    (dict(workspace=WS + 2), "table cswap_keys: workspace must be 4-byte aligned"),
    (dict(ws_bytes=39), "table cswap_keys: workspace too small (40 bytes needed)"),
    (dict(mbits=MB + 4), "table cswap_keys: mbits_out must be 8-byte aligned"),
    (dict(keys=None), "table cswap_keys: keys must not be NULL"),
    (dict(replies=None), "table cswap_keys: replies must not be NULL"),
    (dict(workspace=None), "table cswap_keys: workspace must not be NULL"),
])
def test_cswap_keys_abi_refuses(kw, msg):
    lib = P.lib()
    assert _cswap(lib, **kw) != 0
    assert lib.pdht_hip_last_error().startswith(msg.encode()), lib.pdht_hip_last_error()


def test_the_long_key_refusals_name_the_record_route():
    lib = P.lib()
    for op in ("update_keys", "add_keys"):
        assert _rows(op, lib, keysize=65, rowbytes=80) != 0
        for name in (b"pdht_bucket_put_records_dev", b"pdht_table_put_records_dev"):
            assert name in lib.pdht_hip_last_error()
    assert _cswap(lib, keysize=65) != 0
    for name in (b"pdht_bucket_records_dev", b"pdht_table_cswap_dev"):
        assert name in lib.pdht_hip_last_error()


def test_put_and_get_keys_keep_their_messages():
    """keys_check moved to where both units reach it: the messages of put_keys and get_keys stay."""
    lib = P.lib()
    assert lib.pdht_table_put_keys_dev(TAB, 64, 24, KEYS, 13, 12, VALS, 8, 8, 10, WS, 40, None, ST, None) != 0
    assert lib.pdht_hip_last_error() == SLOT.format("put_keys").encode()
    assert lib.pdht_table_put_keys_dev(TAB, 64, 24, KEYS, 13, 0, VALS, 8, 8, 10, WS, 39, None, ST, None) != 0
    assert lib.pdht_hip_last_error() == b"table put_keys: workspace too small (40 bytes needed)"
    assert lib.pdht_table_put_keys_dev(TAB, 64, 24, KEYS, 13, 0, VALS, 8, 8, 10, WS + 2, 40, None, ST, None) != 0
    assert lib.pdht_hip_last_error() == b"table put_keys: workspace must be 4-byte aligned"
    assert lib.pdht_table_get_keys_dev(TAB, 64, 32, KEYS, 13, 0, 10, VALS, 8, 8, None, ST, None) != 0
    assert lib.pdht_hip_last_error().startswith(ROW.format("get_keys").encode())


def test_geometries_that_pass():
    """What the refusals above must not catch: every key length of 1 .. 64 with its own slot and with the
    slots 32 and 64, status and mbits_out as they may be."""
    lib = P.lib()
    for L in range(1, 65):
        assert _cswap(lib, keysize=L, m=0) == 0, lib.pdht_hip_last_error()
        for key_slot in (0, 32, 64):
            if key_slot and key_slot < L:
                continue
            slot = key_slot or (L + 7) // 8 * 8
            for E in (1, 8, 24):
                kw = dict(keysize=L, key_slot=key_slot, elemsize=E, value_stride=E, rowbytes=(slot + E + 7) // 8 * 8, m=0)
                assert _rows("update_keys", lib, **kw) == 0, lib.pdht_hip_last_error()
                assert _rows("add_keys", lib, **kw) == 0, lib.pdht_hip_last_error()
    for op in ("update_keys", "add_keys"):
        assert _rows(op, lib, m=0, status=None, mbits=MB) == 0
    assert _cswap(lib, m=0, mbits=MB, word_offset=0, reply_stride=24, replies=REP + 8) == 0


def test_empty_batches_launch_nothing_and_name_their_kernels():
    """m == 0 returns 0 without a device call (none is possible here) and names what would have run, the row
    pieces by rowbytes alone."""
    lib = P.lib()
    empty = dict(m=0, keys=None, values=None, workspace=None, ws_bytes=0, status=None)
    for op, pair in (("update_keys", b"k_table_locate_keys<last>+k_table_write_keys<%d>"),
                     ("add_keys", b"k_table_add_claim_keys+k_table_add_write_keys<%d>")):
        assert _rows(op, lib, m=0) == 0 and lib.pdht_hip_last_kernel() == pair % 8        # rowbytes 24
        assert _rows(op, lib, **empty) == 0 and lib.pdht_hip_last_kernel() == pair % 8
        assert _rows(op, lib, m=0, rowbytes=32, elemsize=16, value_stride=16) == 0
        assert lib.pdht_hip_last_kernel() == pair % 16
        assert _rows(op, lib, m=0, rowbytes=32, elemsize=9, value_stride=11, values=VALS + 1) == 0
        assert lib.pdht_hip_last_kernel() == pair % 16
    assert _cswap(lib, m=0) == 0 and lib.pdht_hip_last_kernel() == b"k_table_locate_keys<first>+k_table_cswap"
    assert _rows("update_keys", lib, m=0) == 0
    assert _cswap(lib, m=0, keys=None, replies=None, workspace=None, ws_bytes=0) == 0
    assert lib.pdht_hip_last_kernel() == b"k_table_locate_keys<first>+k_table_cswap"
    # the keyed put's tag stays
    assert lib.pdht_table_put_keys_dev(TAB, 64, 24, None, 13, 0, None, 8, 8, 0, None, 0, None, None, None) == 0
    assert lib.pdht_hip_last_kernel() == b"k_table_claim_keys+k_table_write_keys<8>"
    assert lib.pdht_table_put_keys_dev(TAB, 64, 32, None, 13, 0, None, 16, 16, 0, None, 0, None, None, None) == 0
    assert lib.pdht_hip_last_kernel() == b"k_table_claim_keys+k_table_write_keys<16>"


# ------------------------------------------------------------- wrappers ---
def _bare_table(rowbytes=24):
    t = object.__new__(P.DeviceTable)  # the methods' own checks, without a device behind them
    t.capacity, t.rowbytes, t.device = 64, rowbytes, torch.device("cuda:0")
    return t


def test_wrappers_check_their_arguments_before_c():
    t = _bare_table()
    u8 = torch.uint8
    for call in (t.update_keys, t.add_keys):
        with pytest.raises(ValueError, match="values"):
            call(torch.zeros((4, 13), dtype=u8), torch.zeros((4, 8), dtype=u8))  # CPU values
        with pytest.raises(ValueError, match="values"):
            call(None, torch.zeros(32, dtype=u8))  # not [m, E]
        with pytest.raises(ValueError, match="values"):
            call(None, None)
    for keys in (torch.zeros((4, 13), dtype=u8), torch.zeros(52, dtype=u8), torch.zeros((4, 13), dtype=torch.int64),
                 None):
        with pytest.raises(ValueError, match="keys"):
            t.cswap_keys(keys, 16, 0, 1)


@pytest.mark.parametrize("kw,match", [
    (dict(word_offset=4), "word_offset"),
    (dict(word_offset=24), "word_offset"),
    (dict(word_offset=-8), "word_offset"),
    (dict(word_offset=8.0), "word_offset"),
    (dict(compare=1 << 64), "compare"),
    (dict(compare=-(1 << 63) - 1), "compare"),
    (dict(compare=1.0), "compare"),
    (dict(desired=1 << 64), "desired"),
    (dict(desired=None), "desired"),
])
def test_cswap_keys_wrapper_refuses_operands(kw, match, monkeypatch):
    """The operand checks come after the keys checks, which need a CUDA tensor: stand in for them."""
    t = _bare_table()
    monkeypatch.setattr(P.DeviceTable, "_packed_keys_arg", lambda self, keys, route: (4, 13))
    args = dict(word_offset=8, compare=0, desired=1)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        t.cswap_keys(None, args["word_offset"], args["compare"], args["desired"])


def test_wrapper_signatures():
    def shape(f):  # (name, kind, default) of every parameter
        return [(p.name, p.kind.name, p.default) for p in inspect.signature(f).parameters.values()]

    pos, kw, none = "POSITIONAL_OR_KEYWORD", "KEYWORD_ONLY", inspect.Parameter.empty
    rows = [("self", pos, none), ("keys", pos, none), ("values", pos, none), ("key_slot", kw, 0), ("status", kw, True),
            ("mbits", kw, None), ("workspace", kw, None), ("stream", kw, None)]
    assert shape(P.DeviceTable.update_keys) == rows
    assert shape(P.DeviceTable.add_keys) == rows
    assert shape(P.DeviceTable.put_keys) == rows
    assert shape(P.DeviceTable.cswap_keys) == [
        ("self", pos, none), ("keys", pos, none), ("word_offset", pos, none), ("compare", pos, none),
        ("desired", pos, none), ("out", kw, None), ("mbits", kw, None), ("workspace", kw, None), ("stream", kw, None)]
    for name in ("table_update_keys_workspace_bytes", "table_add_keys_workspace_bytes",
                 "table_cswap_keys_workspace_bytes"):
        assert name in P.__all__
