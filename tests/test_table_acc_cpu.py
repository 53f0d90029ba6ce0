"""CPU-side checks of the table's accumulate (include/pdht_hip_table_acc.h; no GPU needed): the exports of
the three libraries, the header, the workspace sizes, every refusal of the entry point -- each with its
message and before any device call, so they hold on a machine without a GPU --, the empty batch, the
Python wrapper's own checks, and the sequential model of tests/table_acc_ref.py on hand-worked cases."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import pdht_amd as P
import table_acc_ref as A

NEW_SYMS = {"pdht_table_acc_workspace_bytes", "pdht_table_acc_records_dev"}


# ------------------------------------------------------ exports and header ---
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


@pytest.mark.parametrize("path", [P.LIB_PATH, P.MPI_LIB_PATH, P.TUNING_LIB_PATH])
def test_every_library_exports_the_acc_entry_points(path):
    assert NEW_SYMS <= _exports(path)
    v = C.CDLL(path).pdht_hip_version
    v.restype = C.c_char_p
    assert b"abi 4" in v()


def test_acc_header_declares_what_the_libraries_export():
    text = open(os.path.join(ROOT, "include", "pdht_hip_table_acc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{)]*\)\s*;", src))
    assert names == NEW_SYMS
    defs = dict(re.findall(r"#define (PDHT_ACC_[A-Z0-9]+) (\w+)", src))
    assert defs == {"PDHT_ACC_INT32": "0", "PDHT_ACC_INT64": "1", "PDHT_ACC_DOUBLE": "2", "PDHT_ACC_ADD": "0",
                    "PDHT_ACC_INSERT": "1u"}  # the reference's enums (libpdht/pdht.h:282-295)
    assert (P.PDHT_ACC_INT32, P.PDHT_ACC_INT64, P.PDHT_ACC_DOUBLE, P.PDHT_ACC_ADD, P.PDHT_ACC_INSERT) == (0, 1, 2, 0, 1)
    flat = re.sub(r"[\s*]+", " ", text)
    # what the header has to say about doubles
    assert "gamma_n = n u / (1 - n u), u = 2^-53" in flat.replace("*", "")
    assert "ordinary (coarse-grained) device memory" in flat and "fine-grained" in flat
    for name in ("k_table_acc<T>", "k_table_acc_claim+k_table_acc<T,insert>"):
        assert name in flat
    top = open(os.path.join(ROOT, "include", "pdht_hip.h")).read()
    assert top.count('#include "pdht_hip_table_acc.h"') == 1
    assert "#define PDHT_HIP_ABI_VERSION 4" in top
    assert "pdht_table_acc" not in re.sub(r'#include "pdht_hip_table_acc.h"', "", top)  # no declaration of its own


def test_acc_header_compiles_as_c99_on_its_own_and_either_way_round(tmp_path):
    body = ("int main(void) { pdht_hip_stream_t s = 0; return pdht_table_acc_workspace_bytes(1, PDHT_ACC_INSERT) == 8 "
            "? pdht_table_acc_records_dev(0, 64, 8, 0, 32, 0, PDHT_ACC_INT64, PDHT_ACC_ADD, 0, 1, 0u, 0, 0, 0, s) "
            "+ PDHT_ACC_INT32 + PDHT_ACC_DOUBLE : 1; }\n")
    for heads in (("pdht_hip_table_acc.h",), ("pdht_hip.h", "pdht_hip_table_acc.h"),
                  ("pdht_hip_table_acc.h", "pdht_hip.h")):
        c = tmp_path / "t.c"
        c.write_text("".join(f'#include "{h}"\n' for h in heads) + body)
        p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                            "-I" + os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr


def test_workspace_bytes():
    for L in (P.lib(), P.mpi_lib()):
        for m in (0, 1, 2, 3, 4, 5, 65, 4097, (1 << 32) - 1):
            assert L.pdht_table_acc_workspace_bytes(m, 0) == 0
            assert L.pdht_table_acc_workspace_bytes(m, 1) == 4 * m + (m + 3) // 4 * 4
    assert P.table_acc_workspace_bytes(4097) == 0
    assert P.table_acc_workspace_bytes(4097, insert=True) == 4 * 4097 + 4100
    for m in (-1, 1 << 32):
        with pytest.raises(ValueError):
            P.table_acc_workspace_bytes(m, True)


# ------------------------------------------------------------- refusals ---
# Fake device addresses: every case below must be refused before anything dereferences them
TAB, REC, WS, ST = 0x100000, 0x200000, 0x300000, 0x900000

GEOM = [
    (dict(capacity=0), b"table: capacity must be a power of two"),
    (dict(capacity=100), b"table: capacity must be a power of two"),
    (dict(rowbytes=0), b"table: rowbytes must be a multiple of 8"),
    (dict(rowbytes=12), b"table: rowbytes must be a multiple of 8"),
    (dict(table=None), b"table: table must not be NULL"),
    (dict(table=TAB + 8), b"table: table must be 16-byte aligned"),
]
REGION = b"table acc: elems must be >= 1 and value_offset + elems * size <= rowbytes"
OFFSET = b"table acc: value_offset must be a multiple of the element size"
DATATYPE = b"table acc: datatype must be PDHT_ACC_INT32, PDHT_ACC_INT64 or PDHT_ACC_DOUBLE"


def _acc(lib, *, table=TAB, capacity=64, rowbytes=16, records=REC, record_stride=40, m=10, datatype=1, op=0,
         value_offset=8, elems=1, flags=0, workspace=WS, ws_bytes=1 << 20, status=ST):
    return lib.pdht_table_acc_records_dev(table, capacity, rowbytes, records, record_stride, m, datatype, op,
                                          value_offset, elems, flags, workspace, ws_bytes, status, None)


@pytest.mark.parametrize("kw,msg", GEOM + [
    (dict(m=1 << 32, ws_bytes=1 << 40), b"table acc: m must be < 2^32"),
    (dict(record_stride=32), b"table acc: record_stride must be a multiple of 8 and >= 24 + rowbytes"),
    (dict(record_stride=44), b"table acc: record_stride must be a multiple of 8 and >= 24 + rowbytes"),
    (dict(records=REC + 4), b"table acc: records must be 8-byte aligned"),
    (dict(datatype=3), DATATYPE),   # CharType
    (dict(datatype=4), DATATYPE),   # BoolType
    (dict(datatype=-1), DATATYPE),
    (dict(datatype=5), DATATYPE),
    (dict(op=1), b"table acc: op must be PDHT_ACC_ADD"),
    (dict(op=-1), b"table acc: op must be PDHT_ACC_ADD"),
    (dict(flags=2), b"table acc: unknown flags"),
    (dict(flags=3), b"table acc: unknown flags"),
    (dict(flags=1 << 31), b"table acc: unknown flags"),
    (dict(value_offset=4), OFFSET),               # i64 at 4
    (dict(datatype=2, value_offset=4), OFFSET),   # f64 at 4
    (dict(datatype=0, value_offset=2), OFFSET),   # i32 at 2
    (dict(datatype=0, value_offset=7), OFFSET),
    (dict(elems=0), REGION),
    (dict(value_offset=16), REGION),              # starts at the row's end
    (dict(value_offset=8, elems=2), REGION),      # one element past it
    (dict(value_offset=24), REGION),
    (dict(datatype=0, value_offset=12, elems=2), REGION),
    (dict(value_offset=0, elems=(1 << 61) + 1), REGION),   # elems * 8 wraps to 8
    (dict(value_offset=(1 << 64) - 8, elems=2), REGION),   # the sum wraps to 8
    (dict(flags=1, workspace=WS + 2), b"table acc: workspace must be 4-byte aligned"),
    (dict(flags=1, ws_bytes=51), b"table acc: workspace too small (52 bytes needed)"),  # 40 + 12
    (dict(flags=1, ws_bytes=0), b"table acc: workspace too small (52 bytes needed)"),
    (dict(records=None), b"table acc: records must not be NULL"),
    (dict(flags=1, workspace=None), b"table acc: workspace must not be NULL"),
])
def test_table_acc_abi_refuses(kw, msg):
    lib = P.lib()
    assert _acc(lib, **kw) != 0
    assert lib.pdht_hip_last_error().startswith(msg), lib.pdht_hip_last_error()


def test_i32_regions_need_no_8_byte_alignment():
    """What is NOT refused: i32 at offset 4 and 12 (m == 0, so nothing is launched)."""
    lib = P.lib()
    for vo, elems in ((4, 1), (4, 3), (12, 1), (0, 4)):
        assert _acc(lib, m=0, datatype=0, value_offset=vo, elems=elems) == 0, lib.pdht_hip_last_error()
    # nor is the workspace looked at where none is needed: flags 0, or an empty batch
    assert _acc(lib, m=0, workspace=WS + 1, ws_bytes=0) == 0, lib.pdht_hip_last_error()
    assert _acc(lib, m=0, flags=1, workspace=WS + 2, ws_bytes=0) == 0, lib.pdht_hip_last_error()


def test_empty_batches_launch_nothing():
    """m == 0 returns 0 without a device call (none is possible here), and names what would have run.  flags 0
    needs no workspace at any m; with INSERT an empty batch needs none either."""
    lib = P.lib()
    for dt, tag in ((0, b"i32"), (1, b"i64"), (2, b"f64")):
        assert _acc(lib, m=0, datatype=dt, records=None, workspace=None, ws_bytes=0, status=None) == 0
        assert lib.pdht_hip_last_kernel() == b"k_table_acc<" + tag + b">"
        assert _acc(lib, m=0, datatype=dt, flags=1, records=None, workspace=None, ws_bytes=0, status=None) == 0
        assert lib.pdht_hip_last_kernel() == b"k_table_acc_claim+k_table_acc<" + tag + b",insert>"


# ------------------------------------------------------------- wrappers ---
def _bare_table():
    t = object.__new__(P.DeviceTable)  # the method's own checks, without a device behind them
    t.capacity, t.rowbytes, t.device = 64, 16, torch.device("cuda:0")
    return t


@pytest.mark.parametrize("kw,match", [
    (dict(dtype=torch.int8), "dtype"),
    (dict(dtype=torch.bool), "dtype"),
    (dict(dtype=torch.float32), "dtype"),
    (dict(dtype=torch.uint8), "dtype"),
    (dict(dtype=np.int64), "dtype"),
    (dict(value_offset=4), "region"),
    (dict(value_offset=-8), "value_offset"),
    (dict(value_offset=8.0), "value_offset"),
    (dict(value_offset=16), "region"),
    (dict(elems=0), "region"),
    (dict(elems=2), "region"),
    (dict(elems=True), "elems"),
    (dict(elems=1.0), "elems"),
    (dict(dtype=torch.int32, value_offset=2), "region"),
    (dict(dtype=torch.int32, value_offset=12, elems=2), "region"),
])
def test_acc_wrapper_refuses_operands(kw, match):
    """dtype and region are checked first, in Python: CPU records never get as far as being looked at."""
    args = dict(dtype=torch.int64, value_offset=8, elems=1)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        _bare_table().acc_records(torch.zeros((4, 40), dtype=torch.uint8), **args)


def test_acc_wrapper_checks_records_before_c():
    t = _bare_table()
    with pytest.raises(ValueError):
        t.acc_records(torch.zeros((4, 40), dtype=torch.uint8), torch.int64, 8)  # CPU records
    with pytest.raises(ValueError):
        t.acc_records(torch.zeros(160, dtype=torch.uint8), torch.float64, 8, insert=True)  # not [m, stride]


# ----------------------------------------------- the model, by hand ---
def _row(*words):
    return np.array(words, np.uint64).view(np.uint8).copy()


def _words(row):
    return [int(x) for x in row.view(np.uint64)]


def test_acc_ref_i64_by_hand():
    state = {5: _row(1, 2), 7: _row(3, 4)}
    rows = np.stack([_row(100, 10), _row(200, 20), _row(300, 30), _row(400, (1 << 64) - 5), _row(500, 50)])
    st, sums = A.acc_ref(state, [5, 9, 5, 7, 9], rows, np.int64, 8, 1, False)
    assert st.tolist() == [0, 3, 0, 0, 3] and sums == {}
    assert sorted(state) == [5, 7]  # 9 was not inserted
    assert _words(state[5]) == [1, 42] and _words(state[7]) == [3, (1 << 64) - 1]  # word 0 untouched; 4 - 5 = -1
    st, _ = A.acc_ref(state, [7, 7], rows[:2], np.int64, 8, 1, False)
    assert st.tolist() == [0, 0] and _words(state[7]) == [3, 29]  # -1 + 10 + 20 wraps through 2^64
    assert A.acc_ref(state, [], rows[:0], np.int64, 8, 1, False)[0].tolist() == []


def test_acc_ref_insert_by_hand():
    state = {5: _row(1, 2)}
    rows = np.stack([_row(100, 10), _row(200, 20), _row(300, 30), _row(400, 40), _row(500, 50)])
    st, _ = A.acc_ref(state, [9, 5, 9, 0, 9], rows, np.int64, 8, 1, True, capacity=64)
    assert st.tolist() == [0, 0, 0, 0, 0]
    assert _words(state[9]) == [100, 90]  # the FIRST record's word 0, the sum of all three
    assert _words(state[5]) == [1, 22] and _words(state[0]) == [400, 40]
    # overflow: the device said 11 and 12 lost
    st, _ = A.acc_ref(state, [11, 9, 12, 11, 13], rows, np.int64, 8, 1, True, dropped={11, 12})
    assert st.tolist() == [2, 0, 2, 2, 0] and 11 not in state and 12 not in state
    assert _words(state[9]) == [100, 110] and _words(state[13]) == [500, 50]


def test_acc_ref_i32_by_hand():
    """Three i32 at offset 4: words 1, 2, 3 of four; element 0 and the bytes of its neighbours stay."""
    def r32(*w):
        return np.array(w, np.uint32).view(np.uint8).copy()
    state = {5: r32(7, 0x7FFFFFFF, 0xFFFFFFFF, 5)}
    rows = np.stack([r32(99, 1, 1, 0xFFFFFFFF), r32(98, 1, 2, 3)])
    st, _ = A.acc_ref(state, [5, 5], rows, np.int32, 4, 3, False)
    assert st.tolist() == [0, 0]
    assert state[5].view(np.uint32).tolist() == [7, 0x80000001, 2, 7]  # past 2^31, past 2^32, -1 + 5 + 3


def test_acc_ref_f64_by_hand():
    def rf(*w):
        return np.array(w, np.float64).view(np.uint8).copy()
    state = {5: rf(1.0, 1e16)}
    rows = np.stack([rf(9.0, 1.0), rf(9.0, -1e16), rf(9.0, 1.0)])
    st, sums = A.acc_ref(state, [5, 5, 5], rows, np.float64, 8, 1, False)
    assert st.tolist() == [0, 0, 0] and set(sums) == {(5, 0)}
    s = sums[(5, 0)]
    assert s["n"] == 4 and s["exact"] == 2.0 and s["abs"] == 2e16 + 2
    assert s["seq"] == (1e16 + 1.0 - 1e16) + 1.0 == 1.0  # position order loses the first 1.0
    assert state[5].view(np.float64).tolist() == [1.0, 1.0]
    assert abs(s["seq"] - s["exact"]) <= A.gamma(s["n"]) * s["abs"]
    assert A.gamma(4) == 4 * 2.0 ** -53 / (1 - 4 * 2.0 ** -53) and math.isclose(A.gamma(1000), 1000 * 2.0 ** -53, rel_tol=1e-12)
    # an inserted entry starts from its first record
    st, sums = A.acc_ref(state, [6, 6], rows[:2], np.float64, 8, 1, True)
    assert state[6].view(np.float64).tolist() == [9.0, 1.0 - 1e16] and sums[(6, 0)]["n"] == 2
