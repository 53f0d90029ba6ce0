"""CPU-side checks of put records and the row movers (no GPU needed):
the record-size query, the argument checks of the C ABI -- every one refused
with a message before any device call, so they hold on a machine without a
GPU -- and the exports of the three libraries (include/pdht_hip_put.h)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

import pdht_amd as P


@pytest.mark.parametrize("keysize,elemsize,key_slot,want", [(8, 8, 0, 40), (8, 8, 32, 64), (13, 5, 0, 48),
                                                            (32, 40, 32, 96), (64, 1, 0, 96), (64, 256, 64, 344)])
def test_put_record_bytes(keysize, elemsize, key_slot, want):
    assert P.put_record_bytes(keysize, elemsize, key_slot) == want
    assert P.lib().pdht_bucket_put_record_bytes(keysize, key_slot, elemsize) == want
    if key_slot == 0:  # the compact form is bucket_records' record plus the padded value
        assert want == P.bucket_record_bytes(keysize) + (elemsize + 7) // 8 * 8


@pytest.mark.parametrize("keysize,key_slot", [(32, 24), (8, 12), (13, 8), (8, 4)])
def test_put_record_bytes_refuses_a_bad_key_slot(keysize, key_slot):
    assert P.lib().pdht_bucket_put_record_bytes(keysize, key_slot, 8) == 0
    with pytest.raises(ValueError, match="key_slot"):
        P.put_record_bytes(keysize, 8, key_slot)


# Fake device addresses: every case below must be refused before anything dereferences them
KEYS, VALS, WS, REC, OFFS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000


def _put(lib, *, keysize=8, values=VALS, elemsize=8, value_stride=8, n=100, nranks=7, key_slot=0,
         records=REC, ws_bytes=1 << 30):
    return lib.pdht_bucket_put_records_dev(KEYS, keysize, values, elemsize, value_stride, n, nranks, P.PDHT_PUT,
                                           0, 0, key_slot, WS, ws_bytes, records, OFFS, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(values=None), b"values must not be NULL"),
    (dict(elemsize=0, value_stride=0), b"elemsize must be >= 1"),
    (dict(elemsize=16, value_stride=12), b"value_stride must be >= elemsize"),
    (dict(records=REC + 4), b"records must be 8-byte aligned"),
    (dict(records=None), b"records must not be NULL"),
    (dict(key_slot=12), b"key_slot"),
    (dict(keysize=32, key_slot=24), b"key_slot"),
    (dict(n=1 << 32), b"2^32"),
    (dict(nranks=0), b"nranks must be > 0"),
    (dict(ws_bytes=16), b"workspace too small"),
])
def test_put_records_abi_refuses(kw, msg):
    lib = P.lib()
    assert _put(lib, **kw) != 0
    assert msg in lib.pdht_hip_last_error(), lib.pdht_hip_last_error()


def _rows(f, *, src=VALS, src_stride=16, rowbytes=16, index=KEYS, index_stride=4, m=10, dst=REC, dst_stride=16):
    return f(src, src_stride, rowbytes, index, index_stride, m, dst, dst_stride, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(index_stride=2), b"index_stride"),
    (dict(index_stride=6), b"index_stride"),
    (dict(index_stride=0), b"index_stride"),
    (dict(dst_stride=15), b"dst_stride must be >= rowbytes"),
    (dict(src_stride=8), b"src_stride must be >= rowbytes"),
    (dict(rowbytes=0, src_stride=0, dst_stride=0), b"rowbytes must be >= 1"),
    (dict(m=1 << 32), b"m must be < 2^32"),
    (dict(index=KEYS + 2), b"index must be 4-byte aligned"),
    (dict(src=None), b"null src, dst or index"),
    (dict(dst=None), b"null src, dst or index"),
    (dict(index=None), b"null src, dst or index"),
])
@pytest.mark.parametrize("mover", ["pdht_gather_rows_dev", "pdht_scatter_rows_dev"])
def test_row_movers_abi_refuse(mover, kw, msg):
    lib = P.lib()
    assert _rows(getattr(lib, mover), **kw) != 0
    assert msg in lib.pdht_hip_last_error(), lib.pdht_hip_last_error()


NEW_SYMS = {"pdht_gather_rows_dev", "pdht_scatter_rows_dev", "pdht_bucket_put_record_bytes",
            "pdht_bucket_put_records_dev"}


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


@pytest.mark.parametrize("path", [P.LIB_PATH, P.MPI_LIB_PATH, P.TUNING_LIB_PATH])
def test_every_library_exports_the_put_entry_points(path):
    assert NEW_SYMS <= _exports(path)
    v = C.CDLL(path).pdht_hip_version
    v.restype = C.c_char_p
    assert b"abi 4" in v()


def test_put_header_declares_what_the_libraries_export():
    """include/pdht_hip_put.h declares exactly the four entry points, and pdht_hip.h includes it, so a
    caller of pdht_hip.h sees them."""
    src = open(os.path.join(ROOT, "include", "pdht_hip_put.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{)]*\)\s*;", src))
    assert names == NEW_SYMS
    assert '#include "pdht_hip_put.h"' in open(os.path.join(ROOT, "include", "pdht_hip.h")).read()
    assert "#define PDHT_HIP_ABI_VERSION 4" in open(os.path.join(ROOT, "include", "pdht_hip.h")).read()


def test_put_header_compiles_as_c99_either_way_round(tmp_path):
    for first in ("pdht_hip.h", "pdht_hip_put.h"):
        c = tmp_path / "t.c"
        c.write_text(f'#include "{first}"\n'
                     "int main(void) { pdht_hip_stream_t s = 0; return pdht_bucket_put_record_bytes(8, 0, 8) == 40 "
                     "? pdht_gather_rows_dev(0, 0, 0, 0, 0, 0, 0, 0, s) : 1; }\n")
        p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                            "-I" + os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr


def test_wrappers_check_before_c():
    """dtype, device and shape are checked in Python (no GPU needed)."""
    import torch
    k = torch.zeros((4, 8), dtype=torch.uint8)
    with pytest.raises(ValueError):
        P.bucket_put_records(k, torch.zeros((4, 8), dtype=torch.uint8), 7)  # CPU tensors
    with pytest.raises(ValueError):
        P.gather_rows(k, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        P.scatter_rows(k, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="records must have shape"):
        P.put_record_fields(torch.zeros((4, 32), dtype=torch.uint8), 8, 8)
