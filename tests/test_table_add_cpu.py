"""CPU-side checks of the table's insert-if-absent (include/pdht_hip_table_add.h; no GPU needed): the
exports of the three libraries, the header, the workspace sizes, every refusal of the entry point -- each
with its message and before any device call, so they hold on a machine without a GPU --, the empty batch
and its kernel tags, the Python wrapper's own checks, and the sequential model of tests/table_add_ref.py
on hand-worked cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import pdht_amd as P
import table_add_ref as A

NEW_SYMS = {"pdht_table_add_workspace_bytes", "pdht_table_add_records_dev"}


# ------------------------------------------------------ exports and header ---
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


@pytest.mark.parametrize("path", [P.LIB_PATH, P.MPI_LIB_PATH, P.TUNING_LIB_PATH])
def test_every_library_exports_the_add_entry_points(path):
    assert NEW_SYMS <= _exports(path)
    v = C.CDLL(path).pdht_hip_version
    v.restype = C.c_char_p
    assert b"abi 4" in v()


def test_add_header_declares_what_the_libraries_export():
    text = open(os.path.join(ROOT, "include", "pdht_hip_table_add.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{)]*\)\s*;", src))
    assert names == NEW_SYMS
    flat = re.sub(r"[\s*]+", " ", text)
    for tag in ('"k_table_add_claim+k_table_add_write<P>"', '"k_table_add_claim+k_table_add_write<P>+k_table_add_reply<W>"'):
        assert tag in flat
    assert "4*m + ((m + 3) & ~3)" in re.sub(r"\s+", " ", text)
    assert "head-1 wire form (reply_t + value) is a pdht_table_get_dev away" in flat
    top = open(os.path.join(ROOT, "include", "pdht_hip.h")).read()
    assert top.count('#include "pdht_hip_table_add.h"') == 1
    assert "#define PDHT_HIP_ABI_VERSION 4" in top
    assert "pdht_table_add" not in re.sub(r'#include "pdht_hip_table_add.h"', "", top)  # no declaration of its own
    # the headers that list the kinds of batches behind counts4[2] name the add
    for h in ("pdht_hip_table.h", "pdht_hip_table_rmw.h", "pdht_hip_table_acc.h"):
        assert "pdht_hip_table_add.h" in open(os.path.join(ROOT, "include", h)).read(), h


def test_add_header_compiles_as_c99_on_its_own_and_either_way_round(tmp_path):
    body = ("int main(void) { pdht_hip_stream_t s = 0; return pdht_table_add_workspace_bytes(1) == 8 "
            "? pdht_table_add_records_dev(0, 64, 8, 0, 32, 0, 0, 0, 0, 0, 0, s) : 1; }\n")
    for heads in (("pdht_hip_table_add.h",), ("pdht_hip.h", "pdht_hip_table_add.h"),
                  ("pdht_hip_table_add.h", "pdht_hip.h")):
        c = tmp_path / "t.c"
        c.write_text("".join(f'#include "{h}"\n' for h in heads) + body)
        p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                            "-I" + os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr


def test_workspace_bytes():
    for L in (P.lib(), P.mpi_lib()):
        for m in (0, 1, 3, 4, 5, 65, 4097, (1 << 32) - 1):
            assert L.pdht_table_add_workspace_bytes(m) == 4 * m + (m + 3) // 4 * 4
            assert L.pdht_table_add_workspace_bytes(m) == L.pdht_table_acc_workspace_bytes(m, 1)
    assert P.table_add_workspace_bytes(0) == 0
    assert P.table_add_workspace_bytes(4097) == 4 * 4097 + 4100
    for m in (-1, 1 << 32):
        with pytest.raises(ValueError):
            P.table_add_workspace_bytes(m)


# ------------------------------------------------------------- refusals ---
# Fake device addresses: every case below must be refused before anything dereferences them
TAB, REC, WS, ST, REP = 0x100000, 0x200000, 0x300000, 0x900000, 0xA00000

GEOM = [
    (dict(capacity=0), b"table: capacity must be a power of two"),
    (dict(capacity=100), b"table: capacity must be a power of two"),
    (dict(capacity=32), b"table: capacity must be a power of two"),
    (dict(capacity=1 << 32), b"table: capacity must be a power of two"),
    (dict(rowbytes=0), b"table: rowbytes must be a multiple of 8"),
    (dict(rowbytes=12), b"table: rowbytes must be a multiple of 8"),
    (dict(rowbytes=1 << 31), b"table: rowbytes must be a multiple of 8"),
    (dict(table=None), b"table: table must not be NULL"),
    (dict(table=TAB + 8), b"table: table must be 16-byte aligned"),
]
STRIDE = b"table add: record_stride must be a multiple of 8 and >= 24 + rowbytes"
REPLY_STRIDE = b"table add: reply_stride must be a multiple of 8 and >= 8 + rowbytes"


def _add(lib, *, table=TAB, capacity=64, rowbytes=16, records=REC, record_stride=40, m=10, workspace=WS,
         ws_bytes=1 << 20, status=ST, replies=None, reply_stride=0):
    return lib.pdht_table_add_records_dev(table, capacity, rowbytes, records, record_stride, m, workspace, ws_bytes,
                                          status, replies, reply_stride, None)


@pytest.mark.parametrize("kw,msg", GEOM + [
    (dict(m=1 << 32, ws_bytes=1 << 40), b"table add: m must be < 2^32"),
    (dict(record_stride=32), STRIDE),
    (dict(record_stride=44), STRIDE),
    (dict(record_stride=0), STRIDE),
    (dict(records=REC + 4), b"table add: records must be 8-byte aligned"),
    (dict(records=REC + 1), b"table add: records must be 8-byte aligned"),
    (dict(workspace=WS + 2), b"table add: workspace must be 4-byte aligned"),
    (dict(workspace=WS + 1), b"table add: workspace must be 4-byte aligned"),
    (dict(ws_bytes=51), b"table add: workspace too small (52 bytes needed)"),  # 40 + 12, one byte short
    (dict(ws_bytes=0), b"table add: workspace too small (52 bytes needed)"),
    (dict(m=4097, ws_bytes=4 * 4097 + 4100 - 1), b"table add: workspace too small (20488 bytes needed)"),
    (dict(replies=REP + 4, reply_stride=24), b"table add: replies must be 8-byte aligned"),
    (dict(replies=REP + 1, reply_stride=24), b"table add: replies must be 8-byte aligned"),
    (dict(replies=REP, reply_stride=0), REPLY_STRIDE),
    (dict(replies=REP, reply_stride=16), REPLY_STRIDE),   # < 8 + rowbytes
    (dict(replies=REP, reply_stride=23), REPLY_STRIDE),
    (dict(replies=REP, reply_stride=28), REPLY_STRIDE),   # no multiple of 8
    (dict(replies=REP, reply_stride=33), REPLY_STRIDE),
    (dict(records=None), b"table add: records must not be NULL"),
    (dict(workspace=None), b"table add: workspace must not be NULL"),
])
def test_table_add_abi_refuses(kw, msg):
    lib = P.lib()
    assert _add(lib, **kw) != 0
    assert lib.pdht_hip_last_error().startswith(msg), lib.pdht_hip_last_error()


PAIR8, PAIR16 = b"k_table_add_claim+k_table_add_write<8>", b"k_table_add_claim+k_table_add_write<16>"


def test_empty_batches_launch_nothing_and_name_their_kernels():
    """m == 0 returns 0 without a device call (none is possible here) and names what would have run: the row
    pieces by the put's rule (rowbytes, record_stride and records + 24 multiples of 16), the reply pieces by the
    get's (replies, reply_stride and 8 + rowbytes multiples of 16).  Without replies any reply_stride passes."""
    lib = P.lib()
    for stride in (0, 1, 7, 16, 24, 1 << 40):
        assert _add(lib, m=0, reply_stride=stride) == 0, lib.pdht_hip_last_error()
        assert lib.pdht_hip_last_kernel() == PAIR8  # REC + 24 is no multiple of 16
    assert _add(lib, m=0, records=None, workspace=None, ws_bytes=0, status=None) == 0
    assert lib.pdht_hip_last_kernel() == PAIR8
    assert _add(lib, m=0, records=REC + 8, record_stride=48) == 0
    assert lib.pdht_hip_last_kernel() == PAIR16
    assert _add(lib, m=0, records=REC + 8, record_stride=40) == 0    # the stride is odd in 8s
    assert lib.pdht_hip_last_kernel() == PAIR8
    assert _add(lib, m=0, records=REC + 8, record_stride=48, rowbytes=24) == 0  # the row is
    assert lib.pdht_hip_last_kernel() == PAIR8
    for kw, tag in ((dict(rowbytes=24, record_stride=48, reply_stride=32), b"16"),    # 4 reply words
                    (dict(rowbytes=24, record_stride=48, reply_stride=40), b"8"),     # stride odd in 8s
                    (dict(rowbytes=24, record_stride=48, replies=REP + 8, reply_stride=32), b"8"),
                    (dict(rowbytes=16, reply_stride=32), b"8"),                       # 3 reply words
                    (dict(rowbytes=8, record_stride=32, reply_stride=16), b"16")):
        kw.setdefault("replies", REP)
        assert _add(lib, m=0, **kw) == 0, lib.pdht_hip_last_error()
        assert lib.pdht_hip_last_kernel() == PAIR8 + b"+k_table_add_reply<" + tag + b">"
    assert _add(lib, m=0, records=REC + 8, record_stride=48, replies=REP, reply_stride=24) == 0
    assert lib.pdht_hip_last_kernel() == PAIR16 + b"+k_table_add_reply<8>"


# ------------------------------------------------------------- wrappers ---
def _bare_table():
    t = object.__new__(P.DeviceTable)  # the method's own checks, without a device behind them
    t.capacity, t.rowbytes, t.device = 64, 16, torch.device("cuda:0")
    return t


def test_add_wrapper_checks_its_arguments_before_c():
    t = _bare_table()
    with pytest.raises(ValueError, match="records"):
        t.add_records(torch.zeros((4, 40), dtype=torch.uint8))  # CPU records
    with pytest.raises(ValueError, match="records"):
        t.add_records(torch.zeros(160, dtype=torch.uint8))  # not [m, stride]
    with pytest.raises(ValueError, match="records"):
        t.add_records(torch.zeros((4, 40), dtype=torch.int64), replies=True)
    with pytest.raises(ValueError, match="records"):
        t.add_records(None)
    assert "replies=None" in str(__import__("inspect").signature(P.DeviceTable.add_records))


# ----------------------------------------------- the model, by hand ---
def _row(*words):
    return np.array(words, np.uint64).view(np.uint8).copy()


def _words(row):
    return [int(x) for x in np.ascontiguousarray(row).view(np.uint64)]


def test_add_ref_leaves_an_existing_entry_untouched():
    state = {5: _row(1, 2), 7: _row(3, 4)}
    rows = np.stack([_row(100, 10), _row(200, 20), _row(300, 30)])
    st, rep = A.add_ref(state, [5, 9, 7], rows, capacity=64)
    assert st.tolist() == [4, 0, 4]
    assert _words(state[5]) == [1, 2] and _words(state[7]) == [3, 4] and _words(state[9]) == [200, 20]
    assert [_words(r) for r in rep] == [[1, 1, 2], [1, 200, 20], [1, 3, 4]]
    assert A.add_ref(state, [], rows[:0])[0].tolist() == []


def test_add_ref_first_of_three_wins():
    state = {}
    rows = np.stack([_row(100, 10), _row(200, 20), _row(300, 30), _row(400, 40)])
    st, rep = A.add_ref(state, [9, 9, 8, 9], rows, capacity=64)
    assert st.tolist() == [0, 4, 0, 4]
    assert _words(state[9]) == [100, 10] and _words(state[8]) == [300, 30]
    assert [_words(r) for r in rep] == [[1, 100, 10], [1, 100, 10], [1, 300, 30], [1, 100, 10]]


def test_add_ref_mbits_zero_is_an_ordinary_key_with_a_slot_of_its_own():
    state = {k: _row(k, k) for k in range(1, 65)}  # 64 ordinary entries: the table is full
    st, rep = A.add_ref(state, [0, 0, 3], np.stack([_row(7, 7), _row(8, 8), _row(9, 9)]), capacity=64)
    assert st.tolist() == [0, 4, 4] and _words(state[0]) == [7, 7] and _words(rep[1]) == [1, 7, 7]
    with pytest.raises(AssertionError):
        A.add_ref(state, [0], _row(1, 1)[None], dropped={0})


def test_add_ref_drops_by_hand():
    state = {k: _row(k, k) for k in range(1, 64)}  # 63 of 64
    rows = np.stack([_row(100 + i, i) for i in range(5)])
    mb = [70, 71, 3, 70, 71]
    st, rep = A.add_ref(state, mb, rows, capacity=64, dropped={71})  # the device said 71 lost
    assert st.tolist() == [0, 2, 4, 4, 2] and 71 not in state and _words(state[70]) == [100, 0]
    assert _words(rep[1]) == [0, 0, 0] and _words(rep[3]) == [1, 100, 0] and _words(rep[2]) == [1, 3, 3]
    for bad in ({3}, {70, 71}, set()):  # a present one; one more than has to go; short while a slot is free
        with pytest.raises(AssertionError):
            A.add_ref({k: _row(k, k) for k in range(1, 64)}, mb, rows, capacity=64, dropped=bad)
