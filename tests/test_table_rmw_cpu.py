"""CPU-side checks of the table's update and compare-and-swap (include/pdht_hip_table_rmw.h; no GPU
needed): the exports of the three libraries, the header, the workspace sizes, every refusal of the two
entry points -- each with its message and before any device call, so they hold on a machine without a
GPU --, the empty batch, the Python wrappers' own checks, and the sequential models of
tests/table_rmw_ref.py on hand-worked cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import pdht_amd as P
import table_rmw_ref as R

NEW_SYMS = {"pdht_table_update_workspace_bytes", "pdht_table_update_records_dev",
            "pdht_table_cswap_workspace_bytes", "pdht_table_cswap_dev"}


# ------------------------------------------------------ exports and header ---
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


@pytest.mark.parametrize("path", [P.LIB_PATH, P.MPI_LIB_PATH, P.TUNING_LIB_PATH])
def test_every_library_exports_the_rmw_entry_points(path):
    assert NEW_SYMS <= _exports(path)
    v = C.CDLL(path).pdht_hip_version
    v.restype = C.c_char_p
    assert b"abi 4" in v()


def test_rmw_header_declares_what_the_libraries_export():
    src = open(os.path.join(ROOT, "include", "pdht_hip_table_rmw.h")).read()
    assert "batches that used the winner words (put, update, cswap)" in re.sub(r"[\s*]+", " ", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{)]*\)\s*;", src))
    assert names == NEW_SYMS
    top = open(os.path.join(ROOT, "include", "pdht_hip.h")).read()
    assert top.count('#include "pdht_hip_table_rmw.h"') == 1
    assert "#define PDHT_HIP_ABI_VERSION 4" in top


def test_rmw_header_compiles_as_c99_on_its_own_and_either_way_round(tmp_path):
    body = ("int main(void) { pdht_hip_stream_t s = 0; return pdht_table_update_workspace_bytes(1) == 4 && "
            "pdht_table_cswap_workspace_bytes(2) == 8 "
            "? pdht_table_update_records_dev(0, 64, 8, 0, 32, 0, 0, 0, 0, s) "
            "+ pdht_table_cswap_dev(0, 64, 8, 0, 8, 0, 0, 1u, 2u, 0, 16, 0, 0, s) : 1; }\n")
    for heads in (("pdht_hip_table_rmw.h",), ("pdht_hip.h", "pdht_hip_table_rmw.h"),
                  ("pdht_hip_table_rmw.h", "pdht_hip.h")):
        c = tmp_path / "t.c"
        c.write_text("".join(f'#include "{h}"\n' for h in heads) + body)
        p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                            "-I" + os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr


def test_workspace_bytes():
    for L in (P.lib(), P.mpi_lib()):
        for m in (0, 1, 65, 4097, (1 << 32) - 1):
            assert L.pdht_table_update_workspace_bytes(m) == 4 * m
            assert L.pdht_table_cswap_workspace_bytes(m) == 4 * m


# ------------------------------------------------------------- refusals ---
# Fake device addresses: every case below must be refused before anything dereferences them
TAB, REC, WS, MB, REP, ST = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x900000

GEOM = [
    (dict(capacity=0), b"table: capacity must be a power of two"),
    (dict(capacity=32), b"table: capacity must be a power of two"),
    (dict(capacity=100), b"table: capacity must be a power of two"),
    (dict(capacity=1 << 32), b"table: capacity must be a power of two"),
    (dict(rowbytes=0), b"table: rowbytes must be a multiple of 8"),
    (dict(rowbytes=12), b"table: rowbytes must be a multiple of 8"),
    (dict(rowbytes=1 << 31), b"table: rowbytes must be a multiple of 8"),
    (dict(table=None), b"table: table must not be NULL"),
    (dict(table=TAB + 8), b"table: table must be 16-byte aligned"),
]


def _update(lib, *, table=TAB, capacity=64, rowbytes=16, records=REC, record_stride=40, m=10, workspace=WS,
            ws_bytes=1 << 20, status=ST):
    return lib.pdht_table_update_records_dev(table, capacity, rowbytes, records, record_stride, m, workspace,
                                             ws_bytes, status, None)


@pytest.mark.parametrize("kw,msg", GEOM + [
    (dict(m=1 << 32, ws_bytes=1 << 40), b"table update: m must be < 2^32"),
    (dict(record_stride=32), b"table update: record_stride must be a multiple of 8 and >= 24 + rowbytes"),
    (dict(record_stride=44), b"table update: record_stride must be a multiple of 8 and >= 24 + rowbytes"),
    (dict(records=REC + 4), b"table update: records must be 8-byte aligned"),
    (dict(workspace=WS + 2), b"table update: workspace must be 4-byte aligned"),
    (dict(ws_bytes=39), b"table update: workspace too small (40 bytes needed)"),
    (dict(records=None), b"table update: records must not be NULL"),
    (dict(workspace=None), b"table update: workspace must not be NULL"),
])
def test_table_update_abi_refuses(kw, msg):
    lib = P.lib()
    assert _update(lib, **kw) != 0
    assert lib.pdht_hip_last_error().startswith(msg), lib.pdht_hip_last_error()


def _cswap(lib, *, table=TAB, capacity=64, rowbytes=16, mbits=MB, mbits_stride=8, m=10, word_offset=8, compare=0,
           desired=1, replies=REP, reply_stride=16, workspace=WS, ws_bytes=1 << 20):
    return lib.pdht_table_cswap_dev(table, capacity, rowbytes, mbits, mbits_stride, m, word_offset, compare, desired,
                                    replies, reply_stride, workspace, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", GEOM + [
    (dict(m=1 << 32, ws_bytes=1 << 40), b"table cswap: m must be < 2^32"),
    (dict(mbits=MB + 4), b"table cswap: mbits must be 8-byte aligned"),
    (dict(mbits_stride=0), b"table cswap: mbits_stride must be a multiple of 8 and >= 8"),
    (dict(mbits_stride=4), b"table cswap: mbits_stride must be a multiple of 8 and >= 8"),
    (dict(mbits_stride=12), b"table cswap: mbits_stride must be a multiple of 8 and >= 8"),
    (dict(word_offset=4), b"table cswap: word_offset must be a multiple of 8 and <= rowbytes - 8"),
    (dict(word_offset=16), b"table cswap: word_offset must be a multiple of 8 and <= rowbytes - 8"),
    (dict(word_offset=(1 << 64) - 8), b"table cswap: word_offset must be a multiple of 8 and <= rowbytes - 8"),
    (dict(rowbytes=8, word_offset=8), b"table cswap: word_offset must be a multiple of 8 and <= rowbytes - 8"),
    (dict(replies=REP + 4), b"table cswap: replies must be 8-byte aligned"),
    (dict(reply_stride=8), b"table cswap: reply_stride must be a multiple of 8 and >= 16"),
    (dict(reply_stride=0), b"table cswap: reply_stride must be a multiple of 8 and >= 16"),
    (dict(reply_stride=20), b"table cswap: reply_stride must be a multiple of 8 and >= 16"),
    (dict(workspace=WS + 2), b"table cswap: workspace must be 4-byte aligned"),
    (dict(ws_bytes=39), b"table cswap: workspace too small (40 bytes needed)"),
    (dict(mbits=None), b"table cswap: mbits must not be NULL"),
    (dict(replies=None), b"table cswap: replies must not be NULL"),
    (dict(workspace=None), b"table cswap: workspace must not be NULL"),
])
def test_table_cswap_abi_refuses(kw, msg):
    lib = P.lib()
    assert _cswap(lib, **kw) != 0
    assert lib.pdht_hip_last_error().startswith(msg), lib.pdht_hip_last_error()


def test_empty_batches_launch_nothing():
    """m == 0 returns 0 without a device call (none is possible here), and names what would have run."""
    lib = P.lib()
    assert _update(lib, m=0, records=None, workspace=None, ws_bytes=0, status=None) == 0
    assert lib.pdht_hip_last_kernel() == b"k_table_locate<last>+k_table_write<8>"
    # rowbytes 48, stride 80, records + 24 16-byte aligned: the put's <16> rule
    assert _update(lib, m=0, rowbytes=48, record_stride=80, records=REC + 8, workspace=None, ws_bytes=0) == 0
    assert lib.pdht_hip_last_kernel() == b"k_table_locate<last>+k_table_write<16>"
    assert _update(lib, m=0, rowbytes=48, record_stride=80, records=REC, workspace=None, ws_bytes=0) == 0
    assert lib.pdht_hip_last_kernel() == b"k_table_locate<last>+k_table_write<8>"
    assert _cswap(lib, m=0, mbits=None, replies=None, workspace=None, ws_bytes=0) == 0
    assert lib.pdht_hip_last_kernel() == b"k_table_locate<first>+k_table_cswap"


# ------------------------------------------------------------- wrappers ---
def test_wrappers_check_before_c():
    """Device, dtype, shape and operands are checked in Python (no GPU needed)."""
    t = object.__new__(P.DeviceTable)  # the methods' own checks, without a device behind them
    t.capacity, t.rowbytes, t.device = 64, 16, torch.device("cuda:0")
    with pytest.raises(ValueError):
        t.update_records(torch.zeros((4, 40), dtype=torch.uint8))  # CPU records
    with pytest.raises(ValueError):
        t.update_records(torch.zeros(160, dtype=torch.uint8))  # not [m, stride]
    with pytest.raises(ValueError):
        t.cswap(torch.zeros(4, dtype=torch.int64), 0, 0, 1)  # CPU mbits
    with pytest.raises(ValueError, match="1-D int64"):
        t.cswap(torch.zeros(4, dtype=torch.int32), 0, 0, 1)
    with pytest.raises(ValueError, match="1-D int64"):
        t.cswap(torch.zeros((4, 2), dtype=torch.int64), 0, 0, 1)
    with pytest.raises(ValueError):
        t.cswap(torch.zeros((4, 32), dtype=torch.uint8), 0, 0, 1)  # CPU records


@pytest.mark.parametrize("kw,match", [
    (dict(word_offset=4), "word_offset"),
    (dict(word_offset=16), "word_offset"),
    (dict(word_offset=-8), "word_offset"),
    (dict(word_offset=8.0), "word_offset"),
    (dict(compare=1 << 64), "compare"),
    (dict(compare=-(1 << 63) - 1), "compare"),
    (dict(compare=1.0), "compare"),
    (dict(desired=1 << 64), "desired"),
    (dict(desired=-(1 << 63) - 1), "desired"),
    (dict(desired=None), "desired"),
])
def test_cswap_wrapper_refuses_operands(kw, match, monkeypatch):
    """The operand checks come after the request checks, which need a CUDA tensor: stand in for them."""
    t = object.__new__(P.DeviceTable)
    t.capacity, t.rowbytes, t.device = 64, 16, torch.device("cuda:0")
    monkeypatch.setattr(P.DeviceTable, "_requests", lambda self, r: (4, 0x400000, 8))
    args = dict(word_offset=8, compare=0, desired=1)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        t.cswap(None, args["word_offset"], args["compare"], args["desired"])


# ----------------------------------------------- the models, by hand ---
def _row(*words):
    return np.array(words, np.uint64).view(np.uint8).copy()


def _word(row, k):
    return int(row.view(np.uint64)[k])


def test_update_ref_by_hand():
    state = {5: _row(1, 2), 7: _row(3, 4)}
    rows = np.stack([_row(10, 11), _row(20, 21), _row(30, 31), _row(40, 41), _row(50, 51)])
    st = R.update_ref(state, [5, 9, 5, 7, 9], rows)
    assert st.tolist() == [1, 3, 0, 0, 3]
    assert sorted(state) == [5, 7]  # 9 was not inserted
    assert (state[5] == rows[2]).all() and (state[7] == rows[3]).all()
    assert R.update_ref(state, [], rows[:0]).tolist() == []


def test_cswap_ref_by_hand():
    U, D = 0, (1 << 63) | 5
    state = {5: _row(77, U), 7: _row(88, 9), 0: _row(99, U)}
    rep = R.cswap_ref(state, [5, 7, 5, 11, 0, 5, 0], 8, U, D)
    found = rep[:, 0].tolist()
    old = [int(x) for x in rep[:, 8:16].copy().view(np.uint64).ravel()]
    assert found == [1, 1, 1, 0, 1, 1, 1] and int(rep[:, 1:8].sum()) == 0
    assert old == [U, 9, D, 0, U, D, D]  # only the first claimant of 5 and of 0 sees UNUSED
    assert _word(state[5], 1) == D and _word(state[7], 1) == 9 and _word(state[0], 1) == D
    assert _word(state[5], 0) == 77 and _word(state[7], 0) == 88 and 11 not in state
    # negative operands are their 64-bit pattern
    state = {1: _row((1 << 64) - 1)}
    rep = R.cswap_ref(state, [1, 1], 0, -1, -2)
    assert [int(x) for x in rep[:, 8:16].copy().view(np.uint64).ravel()] == [(1 << 64) - 1, (1 << 64) - 2]
    # compare == desired: nothing changes, everybody sees the word
    rep = R.cswap_ref(state, [1, 1], 0, -2, -2)
    assert [int(x) for x in rep[:, 8:16].copy().view(np.uint64).ravel()] == [(1 << 64) - 2] * 2
