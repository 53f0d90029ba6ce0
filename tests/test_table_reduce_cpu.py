"""CPU-side checks of the table's reduce (include/pdht_hip_table_reduce.h; no GPU needed): the exports of the
three libraries, the header, the workspace sizes, every refusal of the entry point -- each with its message
and before any device call, so they hold on a machine without a GPU --, the empty batch and its kernel
names, the Python wrapper's own checks, and the sequential model of tests/table_reduce_ref.py on hand-worked
cases: signedness, the double order on every kind of special value, and "the result is one operand's bits"."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import pdht_amd as P
import table_reduce_ref as R

NEW_SYMS = {"pdht_table_reduce_workspace_bytes", "pdht_table_reduce_records_dev"}
OPS = ["add", "min", "max", "and", "or", "xor"]


# ------------------------------------------------------ exports and header ---
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


@pytest.mark.parametrize("path", [P.LIB_PATH, P.MPI_LIB_PATH, P.TUNING_LIB_PATH])
def test_every_library_exports_the_reduce_entry_points(path):
    assert NEW_SYMS <= _exports(path)
    v = C.CDLL(path).pdht_hip_version
    v.restype = C.c_char_p
    assert b"abi 4" in v()


def test_reduce_header_declares_what_the_libraries_export():
    text = open(os.path.join(ROOT, "include", "pdht_hip_table_reduce.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{)]*\)\s*;", src))
    assert names == NEW_SYMS
    defs = dict(re.findall(r"#define (PDHT_[A-Z0-9]+_[A-Z0-9]+) (\w+)", src))
    assert defs == {"PDHT_RED_ADD": "0", "PDHT_RED_MIN": "1", "PDHT_RED_MAX": "2", "PDHT_RED_AND": "3",
                    "PDHT_RED_OR": "4", "PDHT_RED_XOR": "5"}  # datatypes and INSERT are the acc header's
    assert '#include "pdht_hip_table_acc.h"' in src
    assert (P.PDHT_RED_ADD, P.PDHT_RED_MIN, P.PDHT_RED_MAX, P.PDHT_RED_AND, P.PDHT_RED_OR, P.PDHT_RED_XOR) == \
        (0, 1, 2, 3, 4, 5)
    assert [R.OPS[o] for o in OPS] == [0, 1, 2, 3, 4, 5] and P.PDHT_RED_ADD == P.PDHT_ACC_ADD
    flat = re.sub(r"[\s*]+", " ", text)
    # what the header has to say about doubles
    assert "totalOrder" in flat and "one of its operands, bit for bit" in flat
    assert "signalling NaN is not quieted" in flat and "subnormal is not flushed" in flat
    assert "-NaN (larger payload first) < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN (larger payload last)" in flat
    for name in ("k_table_acc<T,op>", "k_table_acc_claim+k_table_acc<T,op,insert>", "+k_table_add_reply<W>"):
        assert name in flat
    top = open(os.path.join(ROOT, "include", "pdht_hip.h")).read()
    assert top.count('#include "pdht_hip_table_reduce.h"') == 1
    assert "#define PDHT_HIP_ABI_VERSION 4" in top
    assert "pdht_table_reduce" not in re.sub(r'#include "pdht_hip_table_reduce.h"', "", top)  # no declaration of its own


def test_reduce_header_compiles_as_c99_on_its_own_and_either_way_round(tmp_path):
    body = ("int main(void) { pdht_hip_stream_t s = 0; return pdht_table_reduce_workspace_bytes(1, PDHT_ACC_INSERT, 0) == 8 "
            "? pdht_table_reduce_records_dev(0, 64, 8, 0, 32, 0, PDHT_ACC_INT64, PDHT_RED_MIN, 0, 1, 0u, 0, 0, 0, 0, 0, s) "
            "+ PDHT_ACC_INT32 + PDHT_ACC_DOUBLE + PDHT_RED_ADD + PDHT_RED_MAX + PDHT_RED_AND + PDHT_RED_OR "
            "+ PDHT_RED_XOR : 1; }\n")
    for heads in (("pdht_hip_table_reduce.h",), ("pdht_hip.h", "pdht_hip_table_reduce.h"),
                  ("pdht_hip_table_reduce.h", "pdht_hip.h"), ("pdht_hip_table_reduce.h", "pdht_hip_table_acc.h")):
        c = tmp_path / "t.c"
        c.write_text("".join(f'#include "{h}"\n' for h in heads) + body)
        p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                            "-I" + os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr


def test_workspace_bytes():
    for L in (P.lib(), P.mpi_lib()):
        for m in (0, 1, 2, 3, 4, 5, 65, 4097, (1 << 32) - 1):
            assert L.pdht_table_reduce_workspace_bytes(m, 0, 0) == 0
            assert L.pdht_table_reduce_workspace_bytes(m, 0, 1) == 4 * m
            for rep in (0, 1, 7):
                assert L.pdht_table_reduce_workspace_bytes(m, 1, rep) == 4 * m + (m + 3) // 4 * 4
                assert L.pdht_table_reduce_workspace_bytes(m, 1, rep) == L.pdht_table_acc_workspace_bytes(m, 1)
    assert P.table_reduce_workspace_bytes(4097) == 0
    assert P.table_reduce_workspace_bytes(4097, replies=True) == 4 * 4097
    assert P.table_reduce_workspace_bytes(4097, insert=True) == 4 * 4097 + 4100
    assert P.table_reduce_workspace_bytes(4097, insert=True, replies=True) == 4 * 4097 + 4100
    assert "table_reduce_workspace_bytes" in P.__all__
    for m in (-1, 1 << 32):
        with pytest.raises(ValueError):
            P.table_reduce_workspace_bytes(m, True)


# ------------------------------------------------------------- refusals ---
# Fake device addresses: every case below must be refused before anything dereferences them
TAB, REC, WS, ST, REP = 0x100000, 0x200000, 0x300000, 0x900000, 0xA00000

GEOM = [
    (dict(capacity=0), b"table: capacity must be a power of two"),
    (dict(capacity=100), b"table: capacity must be a power of two"),
    (dict(rowbytes=0), b"table: rowbytes must be a multiple of 8"),
    (dict(rowbytes=12), b"table: rowbytes must be a multiple of 8"),
    (dict(table=None), b"table: table must not be NULL"),
    (dict(table=TAB + 8), b"table: table must be 16-byte aligned"),
]
REGION = b"table reduce: elems must be >= 1 and value_offset + elems * size <= rowbytes"
OFFSET = b"table reduce: value_offset must be a multiple of the element size"
DATATYPE = b"table reduce: datatype must be PDHT_ACC_INT32, PDHT_ACC_INT64 or PDHT_ACC_DOUBLE"
OP = b"table reduce: op must be PDHT_RED_ADD .. PDHT_RED_XOR"
BITWISE = b"table reduce: PDHT_RED_AND, _OR and _XOR are not defined for PDHT_ACC_DOUBLE"
STRIDE = b"table reduce: record_stride must be a multiple of 8 and >= 24 + rowbytes"
RSTRIDE = b"table reduce: reply_stride must be a multiple of 8 and >= 8 + rowbytes"


def _red(lib, *, table=TAB, capacity=64, rowbytes=16, records=REC, record_stride=40, m=10, datatype=1, op=1,
         value_offset=8, elems=1, flags=0, workspace=WS, ws_bytes=1 << 20, status=ST, replies=None, reply_stride=0):
    return lib.pdht_table_reduce_records_dev(table, capacity, rowbytes, records, record_stride, m, datatype, op,
                                             value_offset, elems, flags, workspace, ws_bytes, status, replies,
                                             reply_stride, None)


@pytest.mark.parametrize("kw,msg", GEOM + [
    (dict(m=1 << 32, ws_bytes=1 << 40), b"table reduce: m must be < 2^32"),
    (dict(record_stride=32), STRIDE),
    (dict(record_stride=44), STRIDE),
    (dict(records=REC + 4), b"table reduce: records must be 8-byte aligned"),
    (dict(datatype=3), DATATYPE),   # CharType
    (dict(datatype=4), DATATYPE),   # BoolType
    (dict(datatype=-1), DATATYPE),
    (dict(datatype=5), DATATYPE),
    (dict(op=-1), OP),
    (dict(op=6), OP),
    (dict(op=1 << 20), OP),
    (dict(datatype=2, op=-1), OP),
    (dict(datatype=2, op=6), OP),
    (dict(datatype=2, op=3), BITWISE),
    (dict(datatype=2, op=4), BITWISE),
    (dict(datatype=2, op=5), BITWISE),
    (dict(datatype=2, op=5, flags=1, replies=REP, reply_stride=24), BITWISE),
    (dict(flags=2), b"table reduce: unknown flags"),
    (dict(flags=3), b"table reduce: unknown flags"),
    (dict(flags=1 << 31), b"table reduce: unknown flags"),
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
    (dict(flags=1, workspace=WS + 2), b"table reduce: workspace must be 4-byte aligned"),
    (dict(replies=REP, reply_stride=24, workspace=WS + 2), b"table reduce: workspace must be 4-byte aligned"),
    # a workspace one byte short, in each of the three sizes (m = 10)
    (dict(replies=REP, reply_stride=24, ws_bytes=39), b"table reduce: workspace too small (40 bytes needed)"),
    (dict(flags=1, ws_bytes=51), b"table reduce: workspace too small (52 bytes needed)"),  # 40 + 12
    (dict(flags=1, replies=REP, reply_stride=24, ws_bytes=51), b"table reduce: workspace too small (52 bytes needed)"),
    (dict(flags=1, ws_bytes=0), b"table reduce: workspace too small (52 bytes needed)"),
    # every reply misalignment
    (dict(replies=REP + 4, reply_stride=24), b"table reduce: replies must be 8-byte aligned"),
    (dict(replies=REP + 1, reply_stride=24), b"table reduce: replies must be 8-byte aligned"),
    (dict(replies=REP, reply_stride=16), RSTRIDE),   # shorter than a reply
    (dict(replies=REP, reply_stride=0), RSTRIDE),
    (dict(replies=REP, reply_stride=28), RSTRIDE),   # no multiple of 8
    (dict(replies=REP, reply_stride=25), RSTRIDE),
    (dict(flags=1, replies=REP + 4, reply_stride=24), b"table reduce: replies must be 8-byte aligned"),
    (dict(op=0, replies=REP, reply_stride=20), RSTRIDE),
    (dict(records=None), b"table reduce: records must not be NULL"),
    (dict(flags=1, workspace=None), b"table reduce: workspace must not be NULL"),
    (dict(replies=REP, reply_stride=24, workspace=None), b"table reduce: workspace must not be NULL"),
])
def test_table_reduce_abi_refuses(kw, msg):
    lib = P.lib()
    assert _red(lib, **kw) != 0
    assert lib.pdht_hip_last_error().startswith(msg), lib.pdht_hip_last_error()


def test_the_accumulate_still_takes_the_sum_only():
    """The old entry point is untouched: any op but PDHT_ACC_ADD is refused there with its message."""
    lib = P.lib()
    for op in (1, 2, 3, 4, 5, -1):
        rc = lib.pdht_table_acc_records_dev(TAB, 64, 16, REC, 40, 10, 1, op, 8, 1, 0, WS, 1 << 20, ST, None)
        assert rc != 0 and lib.pdht_hip_last_error().startswith(b"table acc: op must be PDHT_ACC_ADD")


def test_what_is_not_refused():
    """i32 at offset 4 and 12 (m == 0, so nothing is launched); a workspace that is not needed is not looked
    at; without replies the reply stride means nothing."""
    lib = P.lib()
    for vo, elems in ((4, 1), (4, 3), (12, 1), (0, 4)):
        for op in range(6):
            assert _red(lib, m=0, datatype=0, op=op, value_offset=vo, elems=elems) == 0, lib.pdht_hip_last_error()
    assert _red(lib, m=0, workspace=WS + 1, ws_bytes=0) == 0, lib.pdht_hip_last_error()
    assert _red(lib, m=0, flags=1, workspace=WS + 2, ws_bytes=0) == 0, lib.pdht_hip_last_error()
    assert _red(lib, m=0, replies=None, reply_stride=3) == 0, lib.pdht_hip_last_error()


TAGS = {0: "i32", 1: "i64", 2: "f64"}


@pytest.mark.parametrize("datatype", [0, 1, 2])
@pytest.mark.parametrize("op", range(6))
def test_empty_batches_launch_nothing_and_name_the_kernels(datatype, op):
    """m == 0 returns 0 without a device call (none is possible here), and names what would have run, for
    every type x op x insert x replies.  ADD names the accumulate's kernels: they are the same."""
    if datatype == 2 and op >= 3:
        return  # refused (test_table_reduce_abi_refuses)
    lib = P.lib()
    t = TAGS[datatype] + ("" if op == 0 else "," + OPS[op])
    for flags, base in ((0, f"k_table_acc<{t}>"), (1, f"k_table_acc_claim+k_table_acc<{t},insert>")):
        assert _red(lib, m=0, datatype=datatype, op=op, flags=flags, records=None, workspace=None, ws_bytes=0,
                    status=None) == 0
        assert lib.pdht_hip_last_kernel() == base.encode()
        # rowbytes 16: three reply words, the <8> form at any address; rowbytes 24: four, <16> where
        # address and stride allow
        for rowbytes, rep, stride, w in ((16, REP, 32, 8), (24, REP, 32, 16), (24, REP + 8, 32, 8), (24, REP, 40, 8),
                                         (8, REP, 16, 16), (8, REP, 24, 8)):
            assert _red(lib, m=0, datatype=datatype, op=op, flags=flags, rowbytes=rowbytes, record_stride=48,
                        value_offset=0, records=None, workspace=None, ws_bytes=0, status=None, replies=rep,
                        reply_stride=stride) == 0, lib.pdht_hip_last_error()
            assert lib.pdht_hip_last_kernel() == (base + f"+k_table_add_reply<{w}>").encode()
    if op == 0:  # the accumulate's own tags
        assert lib.pdht_table_acc_records_dev(TAB, 64, 16, None, 40, 0, datatype, 0, 8, 1, 1, None, 0, None, None) == 0
        assert lib.pdht_hip_last_kernel() == f"k_table_acc_claim+k_table_acc<{TAGS[datatype]},insert>".encode()


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
    (dict(op="sum"), "op"),
    (dict(op="MIN"), "op"),
    (dict(op=6), "op"),
    (dict(op=-1), "op"),
    (dict(op=1.0), "op"),
    (dict(op=True), "op"),
    (dict(op=None), "op"),
    (dict(dtype=torch.float64, op="and"), "int32 and torch.int64 only"),
    (dict(dtype=torch.float64, op="or"), "int32 and torch.int64 only"),
    (dict(dtype=torch.float64, op=P.PDHT_RED_XOR), "int32 and torch.int64 only"),
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
def test_reduce_wrapper_refuses_operands(kw, match):
    """dtype, op and region are checked first, in Python: CPU records never get as far as being looked at."""
    args = dict(dtype=torch.int64, op="min", value_offset=8, elems=1)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        _bare_table().reduce_records(torch.zeros((4, 40), dtype=torch.uint8), **args)


def test_reduce_wrapper_checks_records_before_c():
    t = _bare_table()
    for op in OPS + list(range(6)):
        with pytest.raises(ValueError, match="records"):
            t.reduce_records(torch.zeros((4, 40), dtype=torch.uint8), torch.int64, op, 8)  # CPU records
    with pytest.raises(ValueError):
        t.reduce_records(torch.zeros(160, dtype=torch.uint8), torch.float64, "max", 8, insert=True)  # not [m, stride]


# ----------------------------------------------- the model, by hand ---
def _row(*words):
    return np.array([w % (1 << 64) for w in words], np.uint64).view(np.uint8).copy()


def _words(row):
    return [int(x) for x in row.view(np.uint64)]


bits = R.bits


M1 = (1 << 64) - 1


def test_reduce_ref_signedness_by_hand():
    """-1 against 0: a min that compared unsigned would keep 0, a max would take -1."""
    for dt, one in ((np.int64, M1), (np.int32, (1 << 32) - 1)):
        assert R.reduce_word(R.MIN, dt, 0, one) == one and R.reduce_word(R.MIN, dt, one, 0) == one
        assert R.reduce_word(R.MAX, dt, 0, one) == 0 and R.reduce_word(R.MAX, dt, one, 0) == 0
    imin, imax = 1 << 63, (1 << 63) - 1
    assert R.reduce_word(R.MIN, np.int64, imax, imin) == imin and R.reduce_word(R.MAX, np.int64, imin, imax) == imax
    assert R.reduce_word(R.MIN, np.int32, 0x7FFFFFFF, 0x80000000) == 0x80000000
    assert R.reduce_word(R.MAX, np.int32, 0x80000000, 1) == 1
    state = {5: _row(1, 0), 7: _row(3, -1)}
    rows = np.stack([_row(100, -1), _row(200, 20), _row(300, -30), _row(400, 0), _row(500, 50)])
    st, rep = R.reduce_ref(state, [5, 9, 5, 7, 9], rows, np.int64, "min", 8, 1, False)
    assert st.tolist() == [0, 3, 0, 0, 3] and sorted(state) == [5, 7]
    assert _words(state[5]) == [1, (-30) % (1 << 64)] and _words(state[7]) == [3, M1]  # word 0 untouched
    # replies: the state AFTER the call for every record of a present mbits, zeros for the absent one
    assert rep.shape == (5, 24) and rep[0].tobytes() == rep[2].tobytes() == b"\1" + bytes(7) + state[5].tobytes()
    assert rep[3].tobytes() == b"\1" + bytes(7) + state[7].tobytes() and not rep[1].any() and not rep[4].any()
    st, _ = R.reduce_ref(state, [5, 7], rows[:2], np.int64, R.MAX, 8, 1, False)
    assert _words(state[5]) == [1, M1] and _words(state[7]) == [3, 20]  # max(-30, -1) = -1; max(-1, 20)
    assert R.reduce_ref(state, [], rows[:0], np.int64, "max", 8, 1, False)[0].tolist() == []


def test_reduce_ref_bitwise_and_i32_by_hand():
    def r32(*w):
        return np.array(w, np.uint32).view(np.uint8).copy()
    state = {5: r32(7, 0xF0F0F0F0, 0x0000FFFF, 5)}
    rows = np.stack([r32(99, 0xFF00FF00, 0x00FF00FF, 9), r32(98, 0x0F0F0F0F, 0xFFFFFFFF, 9)])
    for op, want in (("and", [7, 0, 0x000000FF, 5]), ("or", [7, 0xFF0FFF0F, 0xFFFFFFFF, 5]),
                     ("xor", [7, 0x0F000F00, 0x00FF00FF, 5])):
        st, _ = R.reduce_ref(state, [5, 5], rows, np.int32, op, 4, 2, False)  # two i32 at offset 4
        assert st.tolist() == [0, 0] and state[5].view(np.uint32).tolist() == want
    with pytest.raises(AssertionError):
        R.reduce_ref({5: _row(1, 2)}, [5], np.stack([_row(1, 2)]), np.float64, "xor", 8, 1, False)


def test_reduce_ref_insert_and_add_by_hand():
    state = {5: _row(1, 2)}
    rows = np.stack([_row(100, 10), _row(200, 20), _row(300, 3), _row(400, 40), _row(500, 50)])
    st, rep = R.reduce_ref(state, [9, 5, 9, 0, 9], rows, np.int64, "min", 8, 1, True, capacity=64)
    assert st.tolist() == [0, 0, 0, 0, 0]
    assert _words(state[9]) == [100, 3]  # the FIRST record's word 0, the min of all three
    assert _words(state[5]) == [1, 2] and _words(state[0]) == [400, 40]
    assert rep[0].tobytes() == rep[2].tobytes() == rep[4].tobytes() == b"\1" + bytes(7) + state[9].tobytes()
    # overflow: the device said 11 and 12 lost
    st, rep = R.reduce_ref(state, [11, 9, 12, 11, 13], rows, np.int64, "max", 8, 1, True, dropped={11, 12})
    assert st.tolist() == [2, 0, 2, 2, 0] and 11 not in state and 12 not in state
    assert _words(state[9]) == [100, 20] and _words(state[13]) == [500, 50]
    assert not rep[[0, 2, 3]].any() and rep[1, 0] == rep[4, 0] == 1
    # ADD is the accumulate's model
    a, b = {5: _row(1, 2)}, {5: _row(1, 2)}
    st, rep = R.reduce_ref(a, [9, 5, 9], rows[:3], np.int64, "add", 8, 1, True)
    import table_acc_ref as A
    assert st.tolist() == A.acc_ref(b, [9, 5, 9], rows[:3], np.int64, 8, 1, True)[0].tolist()
    assert {k: v.tobytes() for k, v in a.items()} == {k: v.tobytes() for k, v in b.items()}
    assert _words(a[9]) == [100, 13] and rep[0].tobytes() == b"\1" + bytes(7) + a[9].tobytes()


QNAN, SNAN, SIGN, LADDER = R.QNAN, R.SNAN, R.SIGN, R.LADDER


def test_the_double_order_by_hand():
    """Every pair of the ladder, both ways round: min takes the earlier, max the later, and the result is that
    operand's bits -- a signalling NaN stays signalling, a subnormal stays, -0.0 is below +0.0."""
    keys = [R.total_order_key(b) for b in LADDER]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    for i, a in enumerate(LADDER):
        for j, b in enumerate(LADDER):
            assert R.reduce_word(R.MIN, np.float64, a, b) == LADDER[min(i, j)]
            assert R.reduce_word(R.MAX, np.float64, a, b) == LADDER[max(i, j)]
    # where both are non-NaN and unequal it is <
    vals = [b for b in LADDER if not np.isnan(np.array([b], np.uint64).view(np.float64)[0])]
    for a in vals:
        for b in vals:
            x, y = (np.array([v], np.uint64).view(np.float64)[0] for v in (a, b))
            if x != y:
                assert (R.total_order_key(a) < R.total_order_key(b)) == bool(x < y)
    assert R.reduce_word(R.MIN, np.float64, bits(0.0), bits(-0.0)) == bits(-0.0)
    assert R.reduce_word(R.MAX, np.float64, bits(-0.0), bits(0.0)) == bits(0.0)
    # through the loop: the row keeps the bits
    state = {5: _row(1, bits(1.5))}
    rows = np.stack([_row(0, SNAN), _row(0, SIGN | 1), _row(0, SIGN | SNAN)])
    R.reduce_ref(state, [5], rows[:1], np.float64, "max", 8, 1, False)
    assert _words(state[5]) == [1, SNAN]
    R.reduce_ref(state, [5, 5], rows[1:], np.float64, "min", 8, 1, False)
    assert _words(state[5]) == [1, SIGN | SNAN]
