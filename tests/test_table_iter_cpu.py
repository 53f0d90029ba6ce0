"""CPU-side checks of the table export (include/pdht_hip_table_iter.h; no GPU needed): the workspace
query, every refusal of the C ABI -- each with its message and before any device call, so they hold on a
machine without a GPU -- the exports of the three libraries, the header, the Python wrappers' own checks,
and the numpy model of tests/table_iter_ref.py against a storage image built by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import pdht_amd as P

import table_iter_ref as IR

TILE = 1024


# ------------------------------------------------------------ workspace ---
@pytest.mark.parametrize("nslots", [1, 64, 65, TILE, TILE + 1, 4 * TILE, 4 * TILE + 1, (1 << 25) + 1, (1 << 31) + 1])
def test_export_workspace_bytes(nslots):
    """4 bytes per tile of 1024 slots, rounded up to 16: a function of nslots only."""
    want = (-(-nslots // TILE) * 4 + 15) // 16 * 16
    assert P.lib().pdht_table_export_workspace_bytes(nslots) == want
    assert P.table_export_workspace_bytes(nslots) == want
    assert IR.TILE == TILE


@pytest.mark.parametrize("nslots", [0, (1 << 31) + 2, 1 << 32, 1 << 63])
def test_export_workspace_bytes_refuses(nslots):
    assert P.lib().pdht_table_export_workspace_bytes(nslots) == 0
    with pytest.raises(ValueError):
        P.table_export_workspace_bytes(nslots)
    with pytest.raises(ValueError):
        P.table_export_workspace_bytes(-1)


# ------------------------------------------------------------- refusals ---
# Fake device addresses: every case below must be refused before anything dereferences them
TAB, MB, ROWS, SLOT, CNT, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000

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


def _export(lib, *, table=TAB, capacity=64, rowbytes=16, first_slot=0, nslots=65, mbits=MB, mbits_stride=8,
            rows=ROWS, row_stride=16, slots=SLOT, slot_stride=4, max_entries=10, count2=CNT, workspace=WS,
            ws_bytes=1 << 20):
    return lib.pdht_table_export_dev(table, capacity, rowbytes, first_slot, nslots, mbits, mbits_stride, rows,
                                     row_stride, slots, slot_stride, max_entries, count2, workspace, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", GEOM + [
    (dict(nslots=0), b"nslots must be >= 1"),
    (dict(nslots=66), b"first_slot + nslots must be <= capacity + 1"),
    (dict(first_slot=1), b"first_slot + nslots must be <= capacity + 1"),
    (dict(first_slot=65, nslots=1), b"first_slot + nslots must be <= capacity + 1"),
    (dict(first_slot=(1 << 64) - 1, nslots=2), b"first_slot + nslots must be <= capacity + 1"),
    (dict(first_slot=2, nslots=(1 << 64) - 1), b"first_slot + nslots must be <= capacity + 1"),
    (dict(mbits=None), b"mbits_out must not be NULL when max_entries > 0"),
    (dict(mbits=MB + 4), b"mbits_out must be 8-byte aligned"),
    (dict(mbits_stride=0), b"mbits_stride must be a multiple of 8 and >= 8"),
    (dict(mbits_stride=4), b"mbits_stride must be a multiple of 8 and >= 8"),
    (dict(mbits_stride=12), b"mbits_stride must be a multiple of 8 and >= 8"),
    (dict(rows=ROWS + 4), b"rows_out must be 8-byte aligned"),
    (dict(row_stride=8), b"row_stride must be a multiple of 8 and >= rowbytes"),
    (dict(row_stride=20), b"row_stride must be a multiple of 8 and >= rowbytes"),
    (dict(slots=SLOT + 2), b"slot_out must be 4-byte aligned"),
    (dict(slot_stride=0), b"slot_stride must be a multiple of 4 and >= 4"),
    (dict(slot_stride=2), b"slot_stride must be a multiple of 4 and >= 4"),
    (dict(slot_stride=6), b"slot_stride must be a multiple of 4 and >= 4"),
    (dict(count2=None), b"count2 must not be NULL"),
    (dict(count2=CNT + 4), b"count2 must be 8-byte aligned"),
    (dict(max_entries=0, mbits=None, rows=None, slots=None, count2=None), b"count2 must not be NULL"),
    (dict(workspace=None), b"workspace must not be NULL"),
    (dict(workspace=WS + 8), b"workspace must be 16-byte aligned"),
    (dict(ws_bytes=15), b"workspace too small (16 bytes needed)"),
    (dict(capacity=4096, nslots=4097, ws_bytes=16), b"workspace too small (32 bytes needed)"),
])
def test_table_export_abi_refuses(kw, msg):
    lib = P.lib()
    assert _export(lib, **kw) != 0
    assert msg in lib.pdht_hip_last_error(), lib.pdht_hip_last_error()


def test_geometry_is_checked_first():
    """A call wrong in every way names the geometry."""
    lib = P.lib()
    assert _export(lib, capacity=100, nslots=0, mbits=None, count2=None, workspace=None) != 0
    assert b"capacity must be a power of two" in lib.pdht_hip_last_error()


# ------------------------------------------------------ exports and header ---
NEW_SYMS = {"pdht_table_export_workspace_bytes", "pdht_table_export_dev"}


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


@pytest.mark.parametrize("path", [P.LIB_PATH, P.MPI_LIB_PATH, P.TUNING_LIB_PATH])
def test_every_library_exports_the_export_entry_points(path):
    assert NEW_SYMS <= _exports(path)
    v = C.CDLL(path).pdht_hip_version
    v.restype = C.c_char_p
    assert b"abi 4" in v()


def test_iter_header_declares_what_the_libraries_export():
    src = open(os.path.join(ROOT, "include", "pdht_hip_table_iter.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{)]*\)\s*;", code))
    assert names == NEW_SYMS
    top = open(os.path.join(ROOT, "include", "pdht_hip.h")).read()
    assert top.count('#include "pdht_hip_table_iter.h"') == 1
    assert "#define PDHT_HIP_ABI_VERSION 4" in top
    # the kernel tags the GPU tests assert are the ones the header documents
    for tag in ("k_table_export_count+k_table_export_scan+k_table_export_write<16>",
                "k_table_export_count+k_table_export_scan+k_table_export_write<8>",
                "k_table_export_count+k_table_export_scan+k_table_export_write<0>",
                "k_table_export_count+k_table_export_scan<0>"):
        assert '"' + tag + '"' in src


def test_iter_header_compiles_as_c99_either_way_round(tmp_path):
    for first, second in (("pdht_hip.h", "pdht_hip_table_iter.h"), ("pdht_hip_table_iter.h", "pdht_hip.h")):
        c = tmp_path / "t.c"
        c.write_text(f'#include "{first}"\n#include "{second}"\n'
                     "int main(void) { pdht_hip_stream_t s = 0; return pdht_table_export_workspace_bytes(65) == 16 "
                     "? pdht_table_export_dev(0, 64, 8, 0, 65, 0, 8, 0, 8, 0, 4, 0, 0, 0, 0, s) : 1; }\n")
        p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                            "-I" + os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr


# ------------------------------------------------------------- wrappers ---
def _table(capacity=64, rowbytes=16):
    """A DeviceTable's methods without a device behind them: their own checks run before anything else."""
    t = object.__new__(P.DeviceTable)
    t.capacity, t.rowbytes, t.device = capacity, rowbytes, torch.device("cuda:0")
    return t


def test_wrappers_check_before_c():
    assert "table_export_workspace_bytes" in P.__all__
    t = _table()
    for kw in (dict(first_slot=-1), dict(first_slot=65), dict(nslots=0), dict(nslots=66), dict(first_slot=1, nslots=65)):
        with pytest.raises(ValueError, match="range"):
            t.export(None, **kw)
        with pytest.raises(ValueError, match="range"):
            t.entries(**kw)
    with pytest.raises(ValueError, match="mbits"):
        t.export(torch.zeros(4, dtype=torch.int64))  # CPU mbits
    with pytest.raises(ValueError, match="mbits"):
        t.export(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="mbits"):
        t.export(torch.zeros((4, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="records"):
        t.export_records(torch.zeros((4, 40), dtype=torch.uint8))  # CPU records
    with pytest.raises(ValueError, match="records"):
        t.export_records(torch.zeros(160, dtype=torch.uint8))


def test_rehash_refuses_before_any_device_work():
    t = _table()
    t.counts = lambda: (67, 0, 1, 67)  # more entries than 64 slots and the private one can hold
    with pytest.raises(ValueError, match="do not fit"):
        t.rehash(64)
    t.counts = lambda: (300, 0, 1, 300)
    with pytest.raises(ValueError, match="do not fit"):
        t.rehash(128)
    for cap in (0, 100, 1 << 32):
        with pytest.raises(ValueError, match="power of two"):
            t.rehash(cap)
    with pytest.raises(ValueError, match="chunk_bytes"):
        t.rehash(128, chunk_bytes=0)


# ---------------------------------------------------------------- model ---
def test_model_on_hand_built_storage():
    """Capacity 64, rowbytes 8, three ordinary entries and mbits 0, written byte by byte by the layout of
    DESIGN.md 4.7."""
    C_, B = 64, 8
    st = np.zeros(64 + 65 * (16 + B), np.uint8)

    def put(slot, tag, row):
        st[64 + 8 * slot:64 + 8 * slot + 8] = np.frombuffer(np.uint64(tag).tobytes(), np.uint8)
        at = 64 + 16 * 65 + B * slot
        st[at:at + B] = row

    put(3, 0xAAAA, 3)
    put(4, 0xFFFFFFFFFFFFFFFF, 4)
    put(63, 7, 63)
    put(64, 1, 64)  # the private slot: present
    rows_at = 64 + 16 * 65
    st[rows_at + B * 10:rows_at + B * 11] = 0xEE  # a row behind an empty tag is not an entry
    assert IR.layout(C_, B) == (64, 64 + 8 * 65, rows_at, st.size)
    mb, rows, slots, cnt = IR.export_ref(st, C_, B)
    assert mb.tolist() == [0xAAAA, 0xFFFFFFFFFFFFFFFF, 7, 0] and slots.tolist() == [3, 4, 63, 64]
    assert rows.tolist() == [[3] * 8, [4] * 8, [63] * 8, [64] * 8] and cnt == (4, 4)
    assert mb.dtype == np.uint64 and slots.dtype == np.uint32 and rows.dtype == np.uint8
    mb, rows, slots, cnt = IR.export_ref(st, C_, B, first_slot=4, nslots=60)
    assert mb.tolist() == [0xFFFFFFFFFFFFFFFF, 7] and slots.tolist() == [4, 63] and cnt == (2, 2)
    mb, rows, slots, cnt = IR.export_ref(st, C_, B, max_entries=1)
    assert mb.tolist() == [0xAAAA] and rows.tolist() == [[3] * 8] and cnt == (4, 1)
    mb, rows, slots, cnt = IR.export_ref(st, C_, B, max_entries=0)
    assert len(mb) == 0 and rows.shape == (0, 8) and cnt == (4, 0)
    mb, rows, slots, cnt = IR.export_ref(st, C_, B, first_slot=64, nslots=1)
    assert mb.tolist() == [0] and slots.tolist() == [64] and cnt == (1, 1)
    assert IR.export_ref(st, C_, B, first_slot=5, nslots=58)[3] == (0, 0)
    # forge_storage builds the same kind of image
    img = IR.forge_storage(C_, B, [0, 5, 64], seed=1)
    mb, rows, slots, cnt = IR.export_ref(img, C_, B)
    assert slots.tolist() == [0, 5, 64] and mb[2] == 0 and (mb[:2] != 0).all() and cnt == (3, 3)
    tags, allrows = IR.split(img, C_, B)
    assert (rows == allrows[[0, 5, 64]]).all() and tags[64] == 1 and int((tags != 0).sum()) == 3
