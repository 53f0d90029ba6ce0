"""pdht_amd -- MI355X batch key-hashing engine for pdht's CityHash path.

Python view of the C-ABI in include/pdht_hip.h / pdht_city.h / pdht_hash.h,
loaded from the in-tree pdht_amd/lib/libpdht_hip.so (built by `make` or
__graft_entry__.build()).  There is no fallback: if the library is missing
the import fails, and the batch entry points fail when no GPU is usable.

torch is used only as device-memory / stream plumbing: tensors are passed to
the C-ABI as raw pointers on torch's current HIP stream.

Mirrors of the reference interface:
  CityHash64 / CityHash64WithSeed(s) / CityHash128(WithSeed) /
  CityHashCrc128(WithSeed) / CityHashCrc256   -- city.h:68-84, citycrc.h:39-46
  PdhtTable.hash (pdht_hash, hash.c:25-30), PdhtTable.sethash (hash.c:39-41)
Batch API (new): city64_batch, city128_batch, citycrc128_batch, *_var,
place_batch (fused pdht_hash over a batch), *_host variants.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(HERE, "lib", "libpdht_hip.so")

__all__ = [
    "lib", "LIB_PATH", "PdhtError", "CityHash64", "CityHash64WithSeed", "CityHash64WithSeeds",
    "CityHash128", "CityHash128WithSeed", "CityHashCrc128", "CityHashCrc128WithSeed",
    "CityHashCrc256", "city64_batch", "city64_seeds_batch", "city64_var_batch", "city128_batch",
    "city128_seed_batch", "city128_var_batch", "citycrc128_batch", "citycrc128_seed_batch",
    "citycrc128_var_batch", "place_batch", "city64_batch_host", "city64_var_batch_host",
    "citycrc128_batch_host", "place_batch_host", "splitmix64_fill", "mixed_lengths",
    "device_count", "PdhtTable", "K2", "bucket_batch", "bucket_records", "record_fields",
    "bucket_record_bytes", "bucket_workspace_bytes", "WeakHashLen32WithSeeds", "WeakHashLen32WithSeeds6",
    "tuning", "last_kernel", "mpi_lib", "table_bytes", "table_reply_bytes", "DeviceTable", "get_resolve",
    "table_export_workspace_bytes", "table_reduce_workspace_bytes", "table_put_keys_workspace_bytes",
    "table_update_keys_workspace_bytes", "table_add_keys_workspace_bytes", "table_cswap_keys_workspace_bytes",
]

K2 = 0x9AE16A3B2F90404F  # city.c:96 (CityHash64WithSeed's seed0)


class PdhtError(RuntimeError):
    pass


class Uint128(C.Structure):
    """city.h:58-65"""

    _fields_ = [("first", C.c_uint64), ("second", C.c_uint64)]


class PtlProcess(C.Union):
    """ptl_process_t stand-in (portals4.h): 8 bytes, .rank is the low uint32."""

    class _Phys(C.Structure):
        _fields_ = [("nid", C.c_uint32), ("pid", C.c_uint32)]

    _fields_ = [("phys", _Phys), ("rank", C.c_uint32)]


_HASHFUNC = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                        C.POINTER(C.c_uint32), C.POINTER(PtlProcess))


class _PdhtT(C.Structure):
    """Stand-in pdht_t of include/pdht_hash.h (keysize, hashfn, ptl.nptes)."""

    _fields_ = [("keysize", C.c_uint), ("hashfn", C.c_void_p), ("nptes", C.c_uint)]


_lib = None        # the library the wrappers call (product, or tuning inside tuning())
_product = None
_tuning = None
_exp = {}  # libpdht_hip_exp[_<tag>].so by tag (tools/ only)
_V = C.c_void_p
_S = C.c_size_t
_U64 = C.c_uint64
_U32 = C.c_uint32
TUNING_LIB_PATH = os.path.join(HERE, "lib", "libpdht_hip_tuning.so")
# tools/ only: the tuning build with a compile-time experiment switched on
# (`make exp EXP=-DPDHT_...`), for A/B of changes a run-time variant cannot select
EXP_LIB_PATH = os.path.join(HERE, "lib", "libpdht_hip_exp.so")
MPI_LIB_PATH = os.path.join(HERE, "lib", "libpdht_hip_mpi.so")


class Xpose64Plan(C.Structure):
    """pdht_hip_xpose64_plan (pdht_hip.h): the 64-B kernel's launch plan."""
    _fields_ = [("grid", C.c_uint64), ("rounds", C.c_uint64), ("launches", C.c_uint64), ("waves", C.c_uint32),
                ("rounds_per_wg", C.c_uint32), ("round_blocked", C.c_uint32), ("reserved", C.c_uint32)]


def _declare(L, tuning=False):
    sig = {
        "pdht_hip_version": (C.c_char_p, []),
        "pdht_hip_last_error": (C.c_char_p, []),
        "pdht_hip_last_kernel": (C.c_char_p, []),
        "pdht_hip_device_count": (C.c_int, [C.POINTER(C.c_int)]),
        "pdht_hip_set_device": (C.c_int, [C.c_int]),
        "pdht_city64_batch_dev": (C.c_int, [_V, _S, _S, _S, _V, _V]),
        "pdht_city64_seeds_batch_dev": (C.c_int, [_V, _S, _S, _S, _U64, _U64, _V, _V]),
        "pdht_city64_batch_var_dev": (C.c_int, [_V, _S, _V, _S, _V, _V]),
        "pdht_city128_batch_dev": (C.c_int, [_V, _S, _S, _S, _V, _V]),
        "pdht_city128_seed_batch_dev": (C.c_int, [_V, _S, _S, _S, _U64, _U64, _V, _V]),
        "pdht_city128_batch_var_dev": (C.c_int, [_V, _S, _V, _S, _V, _V]),
        "pdht_citycrc128_batch_dev": (C.c_int, [_V, _S, _S, _S, _V, _V]),
        "pdht_citycrc128_seed_batch_dev": (C.c_int, [_V, _S, _S, _S, _U64, _U64, _V, _V]),
        "pdht_citycrc128_batch_var_dev": (C.c_int, [_V, _S, _V, _S, _V, _V]),
        "pdht_place_batch_dev": (C.c_int, [_V, _S, _S, _U32, _U32, _V, _V, _V, _S, _V, _V]),
        "pdht_city64_batch_host": (C.c_int, [_V, _S, _S, _V, C.c_int]),
        "pdht_city64_batch_var_host": (C.c_int, [_V, _V, _S, _V, C.c_int]),
        "pdht_citycrc128_batch_host": (C.c_int, [_V, _S, _S, _V, C.c_int]),
        "pdht_place_batch_host": (C.c_int, [_V, _S, _S, _U32, _U32, _V, _V, _V, _S, C.c_int]),
        "pdht_hip_splitmix64_fill_dev": (C.c_int, [_U64, _U64, _S, _V, _V]),
        "pdht_hip_mixed_lengths_dev": (C.c_int, [_U64, _U64, _S, _U32, _U32, _V, _V]),
        "pdht_hip_read_stream_dev": (C.c_int, [_V, _S, C.c_int, _V, _V]),
        "pdht_hip_key_stream_dev": (C.c_int, [_V, _S, _V, _V]),
        "pdht_hip_key_stream_var_dev": (C.c_int, [_V, _S, _V, _S, _V, _V]),
        "pdht_hip_mod_dev": (C.c_int, [_V, _S, _U32, _V, _V]),
        "pdht_hip_xpose64_plan_for": (C.c_int, [_S, C.c_int, C.c_int, C.c_int, C.POINTER(Xpose64Plan)]),
        "pdht_hip_xpose64_tiles": (C.c_int, [C.POINTER(Xpose64Plan), _U64, _S, _V]),
        "pdht_bucket_workspace_bytes": (C.c_size_t, [_S, _S, _U32]),
        "pdht_bucket_records_workspace_bytes": (C.c_size_t, [_S, _S, _U32]),
        "pdht_bucket_batch_dev": (C.c_int, [_V, _S, _S, _U32, _U32, _V, _S, _V, _V, _V, _V, _V, _V]),
        "pdht_bucket_record_bytes": (C.c_size_t, [_S]),
        "pdht_bucket_records_dev": (C.c_int, [_V, _S, _S, _U32, _U32, _U32, _U32, _V, _S, _V, _V, _V]),
        "pdht_bucket_put_record_bytes": (C.c_size_t, [_S, _S, _S]),
        "pdht_bucket_put_records_dev": (C.c_int, [_V, _S, _V, _S, _S, _S, _U32, _U32, _U32, _U32, _S, _V, _S, _V,
                                                  _V, _V]),
        "pdht_gather_rows_dev": (C.c_int, [_V, _S, _S, _V, _S, _S, _V, _S, _V]),
        "pdht_scatter_rows_dev": (C.c_int, [_V, _S, _S, _V, _S, _S, _V, _S, _V]),
        "pdht_table_bytes": (C.c_size_t, [_U64, _S]),
        "pdht_table_init_dev": (C.c_int, [_V, _S, _U64, _S, _V]),
        "pdht_table_put_workspace_bytes": (C.c_size_t, [_S]),
        "pdht_table_put_records_dev": (C.c_int, [_V, _U64, _S, _V, _S, _S, _V, _S, _V, _V]),
        "pdht_table_reply_bytes": (C.c_size_t, [_S, _S]),
        "pdht_table_get_dev": (C.c_int, [_V, _U64, _S, _V, _S, _S, _V, _S, _S, _V]),
        "pdht_table_counts_dev": (C.c_int, [_V, _V, _V]),
        "pdht_table_export_workspace_bytes": (C.c_size_t, [_U64]),
        "pdht_table_export_dev": (C.c_int, [_V, _U64, _S, _U64, _U64, _V, _S, _V, _S, _V, _S, _U64, _V, _V, _S, _V]),
        "pdht_table_update_workspace_bytes": (C.c_size_t, [_S]),
        "pdht_table_update_records_dev": (C.c_int, [_V, _U64, _S, _V, _S, _S, _V, _S, _V, _V]),
        "pdht_table_cswap_workspace_bytes": (C.c_size_t, [_S]),
        "pdht_table_cswap_dev": (C.c_int, [_V, _U64, _S, _V, _S, _S, _S, _U64, _U64, _V, _S, _V, _S, _V]),
        "pdht_table_acc_workspace_bytes": (C.c_size_t, [_S, C.c_uint]),
        "pdht_table_acc_records_dev": (C.c_int, [_V, _U64, _S, _V, _S, _S, C.c_int, C.c_int, _S, _S, C.c_uint, _V, _S,
                                                 _V, _V]),
        "pdht_table_add_workspace_bytes": (C.c_size_t, [_S]),
        "pdht_table_add_records_dev": (C.c_int, [_V, _U64, _S, _V, _S, _S, _V, _S, _V, _V, _S, _V]),
        "pdht_table_reduce_workspace_bytes": (C.c_size_t, [_S, C.c_uint, C.c_int]),
        "pdht_table_reduce_records_dev": (C.c_int, [_V, _U64, _S, _V, _S, _S, C.c_int, C.c_int, _S, _S, C.c_uint, _V,
                                                    _S, _V, _V, _S, _V]),
        "pdht_get_resolve_dev": (C.c_int, [_V, _S, _S, _S, _V, _S, _V, _S, _S, _V, _S, _S, _V, _V]),
        "pdht_table_put_keys_workspace_bytes": (C.c_size_t, [_S]),
        "pdht_table_put_keys_dev": (C.c_int, [_V, _U64, _S, _V, _S, _S, _V, _S, _S, _S, _V, _S, _V, _V, _V]),
        "pdht_table_get_keys_dev": (C.c_int, [_V, _U64, _S, _V, _S, _S, _S, _V, _S, _S, _V, _V, _V]),
        "pdht_table_update_keys_workspace_bytes": (C.c_size_t, [_S]),
        "pdht_table_update_keys_dev": (C.c_int, [_V, _U64, _S, _V, _S, _S, _V, _S, _S, _S, _V, _S, _V, _V, _V]),
        "pdht_table_add_keys_workspace_bytes": (C.c_size_t, [_S]),
        "pdht_table_add_keys_dev": (C.c_int, [_V, _U64, _S, _V, _S, _S, _V, _S, _S, _S, _V, _S, _V, _V, _V]),
        "pdht_table_cswap_keys_workspace_bytes": (C.c_size_t, [_S]),
        "pdht_table_cswap_keys_dev": (C.c_int, [_V, _U64, _S, _V, _S, _S, _S, _U64, _U64, _V, _S, _V, _S, _V, _V]),
        "CityHash64": (_U64, [_V, _S]),
        "CityHash64WithSeed": (_U64, [_V, _S, _U64]),
        "CityHash64WithSeeds": (_U64, [_V, _S, _U64, _U64]),
        "CityHash128": (Uint128, [_V, _S]),
        "CityHash128WithSeed": (Uint128, [_V, _S, Uint128]),
        "CityHashCrc128": (Uint128, [_V, _S]),
        "CityHashCrc128WithSeed": (Uint128, [_V, _S, Uint128]),
        "CityHashCrc256": (None, [_V, _S, C.POINTER(C.c_uint64)]),
        "WeakHashLen32WithSeeds": (Uint128, [_V, _U64, _U64]),
        "WeakHashLen32WithSeeds6": (Uint128, [_U64, _U64, _U64, _U64, _U64, _U64]),
        "pdht_hash": (None, [_V, _V, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                             C.POINTER(PtlProcess)]),
        "pdht_sethash": (None, [_V, _V]),
        "pdht_hash_batch": (C.c_int, [_V, _V, _S, _V, _V, _V, C.c_int]),
        "pdht_hash_batch_dev": (C.c_int, [_V, _V, _S, _V, _V, _V, _V, _V]),
        "pdht_hip_table_init": (None, [_V, C.c_uint, C.c_uint]),
    }
    if tuning:
        sig["pdht_hip_set_variant"] = (C.c_int, [C.c_int])
        sig["pdht_hip_set_blocks_per_cu"] = (C.c_int, [C.c_int])
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args


def _load(path, tuning=False):
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `make -C {ROOT}` or "
            "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
    L = C.CDLL(path)
    _declare(L, tuning)
    return L


def lib():
    """The library the batch wrappers call: the product libpdht_hip.so (loaded
    once), or the tuning build inside a `tuning()` block.  Raises if it was
    not built."""
    global _lib, _product
    if _lib is None:
        _product = _load(LIB_PATH)
        _lib = _product
    return _lib


_mpi = None


def mpi_lib():
    """libpdht_hip_mpi.so: the same engine with the libmpipdht flavour of
    pdht_hash / pdht_hash_batch(_dev) (libmpipdht/hash.c:6-9: mbits and rank,
    ptindex never written).  Loaded on demand, beside the product library."""
    global _mpi
    if _mpi is None:
        _mpi = _load(MPI_LIB_PATH)
    return _mpi


class tuning:
    """Context manager for tools/ and the A/B tests: route every wrapper
    through libpdht_hip_tuning.so (same sources, built with the A/B hook
    headers of pdht_amd/csrc/tuning/) with
    kernel variant `variant` and, optionally, `per_cu` workgroups per CU.
    The product library has no variants and no tuning entry points."""

    def __init__(self, variant: int = 0, per_cu: int = 0, exp=False):
        # exp: True = libpdht_hip_exp.so, "<tag>" = libpdht_hip_exp_<tag>.so
        # (compile-time experiments: make exp EXP=... EXP_TAG=<tag>)
        self.variant, self.per_cu, self.exp = variant, per_cu, exp

    def __enter__(self):
        global _lib, _tuning, _exp
        lib()
        if self.exp:
            tag = "" if self.exp is True else str(self.exp)
            if tag not in _exp:
                path = EXP_LIB_PATH if not tag else EXP_LIB_PATH.replace(".so", f"_{tag}.so")
                _exp[tag] = _load(path, tuning=True)
            self._t = _exp[tag]
        else:
            if _tuning is None:
                _tuning = _load(TUNING_LIB_PATH, tuning=True)
            self._t = _tuning
        self._prev = _lib
        self._old = (self._t.pdht_hip_set_variant(self.variant),
                     self._t.pdht_hip_set_blocks_per_cu(self.per_cu))
        _lib = self._t
        return self

    def __exit__(self, *exc):
        global _lib
        self._t.pdht_hip_set_variant(self._old[0])
        self._t.pdht_hip_set_blocks_per_cu(self._old[1])
        _lib = self._prev
        return False


def _check(rc: int, what: str):
    if rc != 0:
        raise PdhtError(f"{what}: {lib().pdht_hip_last_error().decode()}")


def last_kernel() -> str:
    return lib().pdht_hip_last_kernel().decode()


def device_count() -> int:
    c = C.c_int(0)
    _check(lib().pdht_hip_device_count(C.byref(c)), "device_count")
    return c.value


# ------------------------------------------------------------ scalar API ---
def _cbuf(data):
    if isinstance(data, np.ndarray):
        return C.c_void_p(data.ctypes.data), data.nbytes
    b = bytes(data)
    return C.c_char_p(b), len(b)


def CityHash64(data) -> int:
    p, n = _cbuf(data)
    return lib().CityHash64(p, n)


def CityHash64WithSeed(data, seed: int) -> int:
    p, n = _cbuf(data)
    return lib().CityHash64WithSeed(p, n, seed)


def CityHash64WithSeeds(data, seed0: int, seed1: int) -> int:
    p, n = _cbuf(data)
    return lib().CityHash64WithSeeds(p, n, seed0, seed1)


def CityHash128(data) -> tuple[int, int]:
    p, n = _cbuf(data)
    r = lib().CityHash128(p, n)
    return r.first, r.second


def CityHash128WithSeed(data, seed: tuple[int, int]) -> tuple[int, int]:
    p, n = _cbuf(data)
    r = lib().CityHash128WithSeed(p, n, Uint128(*seed))
    return r.first, r.second


def CityHashCrc128(data) -> tuple[int, int]:
    p, n = _cbuf(data)
    r = lib().CityHashCrc128(p, n)
    return r.first, r.second


def CityHashCrc128WithSeed(data, seed: tuple[int, int]) -> tuple[int, int]:
    p, n = _cbuf(data)
    r = lib().CityHashCrc128WithSeed(p, n, Uint128(*seed))
    return r.first, r.second


def CityHashCrc256(data) -> tuple[int, int, int, int]:
    p, n = _cbuf(data)
    out = (C.c_uint64 * 4)()
    lib().CityHashCrc256(p, n, out)
    return tuple(out)


def WeakHashLen32WithSeeds(data, a: int, b: int) -> tuple[int, int]:
    """city.c:190-198 (reads 32 bytes of data)."""
    p, n = _cbuf(data)
    if n < 32:
        raise ValueError("WeakHashLen32WithSeeds reads 32 bytes")
    r = lib().WeakHashLen32WithSeeds(p, a, b)
    return r.first, r.second


def WeakHashLen32WithSeeds6(w: int, x: int, y: int, z: int, a: int, b: int) -> tuple[int, int]:
    """city.c:173-187"""
    r = lib().WeakHashLen32WithSeeds6(w, x, y, z, a, b)
    return r.first, r.second


# ----------------------------------------------------- device batch API ---
# Every device wrapper launches on the device its tensors live on: the C-ABI
# sizes grids for, and launches on, the CURRENT device, so each call runs
# under `with torch.cuda.device(<tensor's device>)` on that device's stream
# (the caller's `stream`, which must belong to the same device, or the
# device's current stream).  Every tensor handed to C is checked for device,
# dtype, contiguity and size first: a wrong one raises instead of letting a
# kernel write past its end.
def _torch():
    import torch
    return torch


class _on:
    """Device guard + stream of one device-side call.  The device switch and
    the current-stream lookup go through torch's raw accessors when they
    exist (a batch call's host cost is what a 1M-key batch waits for:
    tools/call_overhead.py)."""

    __slots__ = ("device", "index", "stream_obj", "prev", "stream")

    def __init__(self, device, stream=None):
        if device.type != "cuda":
            raise ValueError("expected CUDA tensors")
        self.device = device
        self.index = device.index if device.index is not None else _torch().cuda.current_device()
        self.stream_obj = stream
        if stream is not None and stream.device != device:
            raise ValueError(f"stream is on {stream.device}, tensors on {device}")

    def __enter__(self):
        tc = _torch()._C
        if hasattr(tc, "_cuda_getDevice") and hasattr(tc, "_cuda_getCurrentRawStream"):
            self.prev = tc._cuda_getDevice()
            if self.prev != self.index:
                tc._cuda_setDevice(self.index)
            s = self.stream_obj.cuda_stream if self.stream_obj is not None else \
                tc._cuda_getCurrentRawStream(self.index)
        else:
            torch = _torch()
            self.prev = torch.cuda.current_device()
            torch.cuda.set_device(self.index)
            s = (self.stream_obj if self.stream_obj is not None else torch.cuda.current_stream(self.device)).cuda_stream
        self.stream = C.c_void_p(s)
        return self

    def __exit__(self, *exc):
        if self.prev != self.index:
            _torch().cuda.set_device(self.prev)
        return False


def _dptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def _opt(t):
    return _dptr(t) if t is not None else None


def _need(t, name, dtype, device, numel=None, shape=None):
    """A CUDA tensor of `dtype` on `device`, contiguous, with >= numel
    elements (or exactly `shape`)."""
    if t is None:
        raise ValueError(f"{name} is required")
    if not getattr(t, "is_cuda", False) or t.device != device:
        raise ValueError(f"{name} must be a CUDA tensor on {device}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if numel is not None and t.numel() < numel:
        raise ValueError(f"{name} must hold >= {numel} elements, got {t.numel()}")
    return t


def _keys_2d(keys):
    """keys: uint8 CUDA tensor [n, L] with unit inner stride (rows may be strided)."""
    torch = _torch()
    if not isinstance(keys, torch.Tensor) or keys.dtype != torch.uint8 or keys.dim() != 2 or not keys.is_cuda:
        raise ValueError("keys must be a CUDA uint8 tensor of shape [n, keylen]")
    n, L = keys.shape
    if keys.stride(1) != 1 and L > 1 and n > 0:
        raise ValueError("keys rows must be contiguous")
    stride = keys.stride(0) if n > 1 else L
    return n, L, stride


def _out(n, words, device, out=None):
    torch = _torch()
    shape = (n,) if words == 1 else (n, words)
    if out is None:
        return torch.empty(shape, dtype=torch.int64, device=device)
    return _need(out, "out", torch.int64, device, shape=shape)


def city64_batch(keys, out=None, stream=None):
    """CityHash64 of each row of keys [n, L] (uint8, CUDA) -> int64 [n] (bit pattern of u64)."""
    n, L, stride = _keys_2d(keys)
    out = _out(n, 1, keys.device, out)
    with _on(keys.device, stream) as g:
        _check(lib().pdht_city64_batch_dev(_dptr(keys), stride, L, n, _dptr(out), g.stream),
               "pdht_city64_batch_dev")
    return out


def city64_seeds_batch(keys, seed0: int, seed1: int, out=None, stream=None):
    n, L, stride = _keys_2d(keys)
    out = _out(n, 1, keys.device, out)
    with _on(keys.device, stream) as g:
        _check(lib().pdht_city64_seeds_batch_dev(_dptr(keys), stride, L, n, seed0, seed1, _dptr(out),
                                                 g.stream), "pdht_city64_seeds_batch_dev")
    return out


def city64_seed_batch(keys, seed: int, out=None, stream=None):
    """CityHash64WithSeed == WithSeeds(k2, seed) (city.c:265-267)."""
    return city64_seeds_batch(keys, K2, seed, out, stream)


def _check_var(data, offsets, check=True, stream=None):
    """(n, nbytes) of a variable-length batch.  nbytes is what the C ABI takes
    as the key bytes the batch spans: it picks the LDS window and how the
    batch is cut into ~512 MiB launches (launch.h launch_var); it never
    addresses memory.

    check=True (default): read offsets[0] and offsets[n] back ON THE LAUNCH
    STREAM (`stream`, else the device's current stream) -- one 16-B D2H copy
    that waits for the work queued before it on that stream, so this call is
    host-synchronous -- require 0 <= offsets[0] <= offsets[n] <= data.numel()
    (a bad offsets tensor raises instead of sending the window kernel past the
    data buffer) and pass the exact span offsets[n] - offsets[0].
    check=False, or while the launch stream is being captured into a graph:
    no read, fully asynchronous; the caller vouches for the offsets and the
    span passed is data.numel() (an upper bound; a much larger buffer than
    the keys only skews the window/launch-size heuristic, never correctness).
    The kernels trust that offsets never decrease, as the reference trusts
    its key pointers."""
    torch = _torch()
    if data.dtype != torch.uint8 or not data.is_cuda or not data.is_contiguous():
        raise ValueError("data must be a contiguous CUDA uint8 tensor")
    _need(offsets, "offsets", torch.int64, data.device)
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("offsets must be a 1-D int64 tensor of n+1 entries")
    n = offsets.numel() - 1
    if check and n:
        s = stream if stream is not None else torch.cuda.current_stream(data.device)
        if s.device != data.device:
            raise ValueError(f"stream is on {s.device}, tensors on {data.device}")
        with torch.cuda.stream(s):
            if not torch.cuda.is_current_stream_capturing():
                lo, hi = (int(x) for x in offsets[[0, n]].tolist())
                if not 0 <= lo <= hi <= data.numel():
                    raise ValueError(f"offsets span bytes [{lo}, {hi}) but data holds {data.numel()}")
                return n, hi - lo
    return n, data.numel()


def city64_var_batch(data, offsets, out=None, stream=None, check=True):
    n, nb = _check_var(data, offsets, check, stream)
    out = _out(n, 1, data.device, out)
    with _on(data.device, stream) as g:
        _check(lib().pdht_city64_batch_var_dev(_dptr(data), nb, _dptr(offsets), n, _dptr(out), g.stream),
               "pdht_city64_batch_var_dev")
    return out


def city128_batch(keys, out=None, stream=None):
    n, L, stride = _keys_2d(keys)
    out = _out(n, 2, keys.device, out)
    with _on(keys.device, stream) as g:
        _check(lib().pdht_city128_batch_dev(_dptr(keys), stride, L, n, _dptr(out), g.stream),
               "pdht_city128_batch_dev")
    return out


def city128_seed_batch(keys, seed: tuple[int, int], out=None, stream=None):
    n, L, stride = _keys_2d(keys)
    out = _out(n, 2, keys.device, out)
    with _on(keys.device, stream) as g:
        _check(lib().pdht_city128_seed_batch_dev(_dptr(keys), stride, L, n, seed[0], seed[1], _dptr(out),
                                                 g.stream), "pdht_city128_seed_batch_dev")
    return out


def city128_var_batch(data, offsets, out=None, stream=None, check=True):
    n, nb = _check_var(data, offsets, check, stream)
    out = _out(n, 2, data.device, out)
    with _on(data.device, stream) as g:
        _check(lib().pdht_city128_batch_var_dev(_dptr(data), nb, _dptr(offsets), n, _dptr(out), g.stream),
               "pdht_city128_batch_var_dev")
    return out


def citycrc128_batch(keys, out=None, stream=None):
    n, L, stride = _keys_2d(keys)
    out = _out(n, 2, keys.device, out)
    with _on(keys.device, stream) as g:
        _check(lib().pdht_citycrc128_batch_dev(_dptr(keys), stride, L, n, _dptr(out), g.stream),
               "pdht_citycrc128_batch_dev")
    return out


def citycrc128_seed_batch(keys, seed: tuple[int, int], out=None, stream=None):
    n, L, stride = _keys_2d(keys)
    out = _out(n, 2, keys.device, out)
    with _on(keys.device, stream) as g:
        _check(lib().pdht_citycrc128_seed_batch_dev(_dptr(keys), stride, L, n, seed[0], seed[1],
                                                    _dptr(out), g.stream), "pdht_citycrc128_seed_batch_dev")
    return out


def citycrc128_var_batch(data, offsets, out=None, stream=None, check=True):
    n, nb = _check_var(data, offsets, check, stream)
    out = _out(n, 2, data.device, out)
    with _on(data.device, stream) as g:
        _check(lib().pdht_citycrc128_batch_var_dev(_dptr(data), nb, _dptr(offsets), n, _dptr(out),
                                                   g.stream), "pdht_citycrc128_batch_var_dev")
    return out


def place_batch(keys, nptes: int, nranks: int, *, ptindex=True, rank=True, hist=None,
                stream=None, out=None):
    """Fused pdht_hash (hash.c:25-30) over keys [n, keysize] (packed, CUDA).

    Returns (mbits int64[n], ptindex int32[n] | None, rank int32[n] | None);
    if `hist` (int64[>= nranks], CUDA) is given, per-rank counts are added to it.
    `out` = a previous return value (same n) to reuse its tensors.
    """
    torch = _torch()
    n, L, stride = _keys_2d(keys)
    if stride != L:
        raise ValueError("place_batch needs packed keys")
    dev = keys.device
    if hist is not None:
        _need(hist, "hist", torch.int64, dev, numel=nranks)
    if out is not None:
        mb, pt, rk = out
        _need(mb, "out[0] (mbits)", torch.int64, dev, shape=(n,))
        if pt is not None:
            _need(pt, "out[1] (ptindex)", torch.int32, dev, shape=(n,))
        if rk is not None:
            _need(rk, "out[2] (rank)", torch.int32, dev, shape=(n,))
    else:
        mb = torch.empty(n, dtype=torch.int64, device=dev)
        pt = torch.empty(n, dtype=torch.int32, device=dev) if ptindex else None
        rk = torch.empty(n, dtype=torch.int32, device=dev) if rank else None
    with _on(dev, stream) as g:
        _check(lib().pdht_place_batch_dev(_dptr(keys), L, n, nptes, nranks, _dptr(mb), _opt(pt), _opt(rk), 4,
                                          _opt(hist), g.stream), "pdht_place_batch_dev")
    return mb, pt, rk


def bind_place_batch(keys, nptes: int, nranks: int, *, hist=None, stream=None, out=None):
    """place_batch prepared once for repeated calls on the same tensors.

    The checks, pointer and stream lookups run here; the returned callable
    makes only the C call (pdht_place_batch_dev on the stream current now),
    i.e. a C caller's per-batch cost.  Returns (call, (mbits, ptindex, rank)).
    The caller keeps keys.device current and the tensors alive.
    """
    torch = _torch()
    n, L, stride = _keys_2d(keys)
    if stride != L:
        raise ValueError("bind_place_batch needs packed keys")
    dev = keys.device
    if hist is not None:
        _need(hist, "hist", torch.int64, dev, numel=nranks)
    if out is None:
        out = (torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev))
    mb, pt, rk = out
    _need(mb, "out[0] (mbits)", torch.int64, dev, shape=(n,))
    _need(pt, "out[1] (ptindex)", torch.int32, dev, shape=(n,))
    _need(rk, "out[2] (rank)", torch.int32, dev, shape=(n,))
    f = lib().pdht_place_batch_dev
    with _on(dev, stream) as g:
        st = g.stream
    vals = (_dptr(keys), L, n, nptes, nranks, _dptr(mb), _dptr(pt), _dptr(rk), 4, _opt(hist), st)
    args = tuple(a if isinstance(a, C._SimpleCData) or a is None else t(a) for t, a in zip(f.argtypes, vals))

    def call():
        rc = f(*args)
        if rc:
            _check(rc, "pdht_place_batch_dev")

    return call, out


def bucket_workspace_bytes(n: int, keysize: int, nranks: int, records: bool = False) -> int:
    """Workspace bytes of bucket_batch (records=False) or bucket_records
    (records=True) on n keysize-byte keys over nranks ranks."""
    if records:
        return lib().pdht_bucket_records_workspace_bytes(n, keysize, nranks)
    return lib().pdht_bucket_workspace_bytes(n, keysize, nranks)


def _workspace(workspace, n, L, nranks, dev, records=False):
    torch = _torch()
    need = bucket_workspace_bytes(n, L, nranks, records)
    if workspace is None:
        return torch.empty(max(need, 1), dtype=torch.uint8, device=dev), need
    _need(workspace, "workspace", torch.uint8, dev, numel=need)
    if workspace.data_ptr() % 16:
        raise ValueError("workspace must be 16-byte aligned")
    return workspace, workspace.numel()


def bucket_batch(keys, nptes: int, nranks: int, *, with_keys=True, with_ptindex=True,
                 with_index=True, stream=None, out=None, workspace=None):
    """Destination bucketing (include/pdht_hip.h pdht_bucket_batch_dev): a stable
    counting sort of packed keys [n, L] by rank = CityHash64 % nranks.

    Returns (keys_out [n, L] | None, mbits int64[n], ptindex int32[n] | None,
    index int32[n] (unsigned original positions) | None, offsets
    int64[nranks+1]); bucket r is rows offsets[r]:offsets[r+1], keys in
    original order.  `out` = a previous return value (same n, L, nranks) to
    reuse its tensors; `workspace` = a uint8 CUDA tensor of at least
    bucket_workspace_bytes(n, L, nranks) bytes (allocated per call if None).
    """
    torch = _torch()
    n, L, stride = _keys_2d(keys)
    if stride != L:
        raise ValueError("bucket_batch needs packed keys")
    dev = keys.device
    ws, ws_bytes = _workspace(workspace, n, L, nranks, dev)
    if out is not None:
        ko, mb, pt, ix, offs = out
        if ko is not None:
            _need(ko, "out[0] (keys)", torch.uint8, dev, shape=(n, L))
        _need(mb, "out[1] (mbits)", torch.int64, dev, shape=(n,))
        if pt is not None:
            _need(pt, "out[2] (ptindex)", torch.int32, dev, shape=(n,))
        if ix is not None:
            _need(ix, "out[3] (index)", torch.int32, dev, shape=(n,))
        _need(offs, "out[4] (offsets)", torch.int64, dev, shape=(nranks + 1,))
    else:
        ko = torch.empty_like(keys, memory_format=torch.contiguous_format) if with_keys else None
        mb = torch.empty(n, dtype=torch.int64, device=dev)
        pt = torch.empty(n, dtype=torch.int32, device=dev) if with_ptindex else None
        ix = torch.empty(n, dtype=torch.int32, device=dev) if with_index else None
        offs = torch.empty(nranks + 1, dtype=torch.int64, device=dev)
    with _on(dev, stream) as g:
        _check(lib().pdht_bucket_batch_dev(_dptr(keys), L, n, nptes, nranks, _dptr(ws), ws_bytes, _opt(ko),
                                           _dptr(mb), _opt(pt), _opt(ix), _dptr(offs), g.stream),
               "pdht_bucket_batch_dev")
    return ko, mb, pt, ix, offs


PDHT_PUT = 1  # msg_type pdhtPut (libmpipdht/pdht.h:72)


def bucket_record_bytes(keysize: int) -> int:
    return lib().pdht_bucket_record_bytes(keysize)


def bucket_records(keys, nranks: int, *, msg_type: int = PDHT_PUT, src_rank: int = 0, ht_index: int = 0,
                   stream=None, out=None, workspace=None):
    """Destination bucketing into wire records (include/pdht_hip.h
    pdht_bucket_records_dev): the MPI variant's message_t header + key for
    every key, bucket r = records[offsets[r]:offsets[r+1]].

    Returns (records uint8 [n, pdht_bucket_record_bytes(L)], offsets int64
    [nranks+1]); record_fields() splits them into tensors.  `out` = a previous
    return value to reuse; `workspace` as for bucket_batch, of at least
    bucket_workspace_bytes(n, L, nranks, records=True) bytes.
    """
    torch = _torch()
    n, L, stride = _keys_2d(keys)
    if stride != L:
        raise ValueError("bucket_records needs packed keys")
    dev = keys.device
    rb = bucket_record_bytes(L)
    ws, ws_bytes = _workspace(workspace, n, L, nranks, dev, records=True)
    if out is not None:
        rec, offs = out
        _need(rec, "out[0] (records)", torch.uint8, dev, shape=(n, rb))
        if rec.data_ptr() % 8:
            raise ValueError("records must be 8-byte aligned")
        _need(offs, "out[1] (offsets)", torch.int64, dev, shape=(nranks + 1,))
    else:
        # int64 storage keeps the records 8-byte aligned
        rec = torch.empty(max(n * rb // 8, 1), dtype=torch.int64, device=dev).view(torch.uint8)[: n * rb]
        rec = rec.view(n, rb)
        offs = torch.empty(nranks + 1, dtype=torch.int64, device=dev)
    with _on(dev, stream) as g:
        _check(lib().pdht_bucket_records_dev(_dptr(keys), L, n, nranks, msg_type, src_rank, ht_index,
                                             _dptr(ws), ws_bytes, _dptr(rec), _dptr(offs), g.stream),
               "pdht_bucket_records_dev")
    return rec, offs


def record_fields(records, keysize: int):
    """Views of a record batch [m, stride] (uint8): (type int32[m], rank
    int32[m], ht_index int32[m], index int32[m] (unsigned), mbits int64[m],
    keys uint8[m, keysize])."""
    torch = _torch()
    m, rb = records.shape
    flat = records.contiguous().view(-1)
    w32 = flat.view(torch.int32).view(m, rb // 4)
    w64 = flat.view(torch.int64).view(m, rb // 8)
    return w32[:, 0], w32[:, 1], w32[:, 2], w32[:, 3], w64[:, 2], records[:, 24:24 + keysize]


# ------------------------------------------- put records and row movers ---
# The payload half of bucketing (include/pdht_hip_put.h).
#   put: bucket_put_records(keys, values, nranks) -> dist.exchange_records
#        (the stride is records.shape[1]) -> DeviceTable.put_records on the
#        receiver (or put_record_fields to split them);
#   get: bucket_records -> dist.exchange_records -> DeviceTable.get ->
#        dist.exchange_replies: the replies come back in bucket order (reply p
#        answers record p) -> get_resolve(replies, keys, E, index=...).
#        scatter_rows(rows, index) puts any row p at row index[p], the
#        caller's order, index being record_fields(records, L)[3] or
#        bucket_batch's index output.  gather_rows(rows, index) is the
#        inverse: rows into bucket order.
def put_record_bytes(keysize: int, elemsize: int, key_slot: int = 0) -> int:
    """Stride of a put record: 24 + slot + elemsize rounded up to 8, slot =
    key_slot or keysize rounded up to 8.  key_slot must be 0 or a multiple of
    8 that is >= keysize (32 = PDHT_MAXKEYSIZE gives putget.c's sbuf)."""
    rb = lib().pdht_bucket_put_record_bytes(keysize, key_slot, elemsize)
    if rb == 0:
        raise ValueError(f"key_slot {key_slot} must be 0 or a multiple of 8 that is >= keysize {keysize}")
    return rb


def _rows_2d(t, name, device=None):
    """t: uint8 CUDA tensor [m, rowbytes] with unit inner stride; rows may be
    strided (a column slice of a wider tensor) and start at any address."""
    torch = _torch()
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2 or not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA uint8 tensor of shape [rows, rowbytes]")
    if device is not None and t.device != device:
        raise ValueError(f"{name} must be on {device}")
    m, B = t.shape
    if B == 0:
        raise ValueError(f"{name} must have at least one byte per row")
    if m and B > 1 and t.stride(1) != 1:
        raise ValueError(f"{name} rows must be contiguous")
    stride = t.stride(0) if m > 1 else B
    if stride < B:
        raise ValueError(f"{name} rows overlap (row stride {stride} < {B} bytes)")
    return m, B, stride


def bucket_put_records(keys, values, nranks: int, *, key_slot: int = 0, msg_type: int = PDHT_PUT,
                       src_rank: int = 0, ht_index: int = 0, stream=None, out=None, workspace=None):
    """Destination bucketing into put records (include/pdht_hip_put.h
    pdht_bucket_put_records_dev): bucket_records' header + key, padded to the
    key slot, + the key's value -- bucket r = records[offsets[r]:offsets[r+1]]
    is the send buffer of a put batch for rank r.

    keys [n, L] packed uint8; values [n, E] uint8, row i the value of key i (a
    column slice of a wider tensor is accepted: its row stride is passed on).
    Returns (records uint8 [n, put_record_bytes(L, E, key_slot)], offsets int64
    [nranks+1]); put_record_fields() splits them.  `out` = a previous return
    value to reuse; `workspace` as for bucket_records
    (bucket_workspace_bytes(n, L, nranks, records=True) bytes).

    Put flow: bucket_put_records -> dist.exchange_records -> DeviceTable.put_records.
    Get flow: bucket_records -> dist.exchange_records -> DeviceTable.get ->
    dist.exchange_replies (bucket order) -> get_resolve(replies, keys, E, index=...).
    """
    torch = _torch()
    n, L, stride = _keys_2d(keys)
    if stride != L:
        raise ValueError("bucket_put_records needs packed keys")
    dev = keys.device
    nv, E, vstride = _rows_2d(values, "values", dev)
    if nv != n:
        raise ValueError(f"values must have one row per key: {nv} rows for {n} keys")
    rb = put_record_bytes(L, E, key_slot)
    ws, ws_bytes = _workspace(workspace, n, L, nranks, dev, records=True)
    if out is not None:
        rec, offs = out
        _need(rec, "out[0] (records)", torch.uint8, dev, shape=(n, rb))
        if rec.data_ptr() % 8:
            raise ValueError("records must be 8-byte aligned")
        _need(offs, "out[1] (offsets)", torch.int64, dev, shape=(nranks + 1,))
    else:
        # int64 storage keeps the records 8-byte aligned
        rec = torch.empty(max(n * rb // 8, 1), dtype=torch.int64, device=dev).view(torch.uint8)[: n * rb]
        rec = rec.view(n, rb)
        offs = torch.empty(nranks + 1, dtype=torch.int64, device=dev)
    with _on(dev, stream) as g:
        _check(lib().pdht_bucket_put_records_dev(_dptr(keys), L, _dptr(values), E, vstride, n, nranks, msg_type,
                                                 src_rank, ht_index, key_slot, _dptr(ws), ws_bytes, _dptr(rec),
                                                 _dptr(offs), g.stream),
               "pdht_bucket_put_records_dev")
    return rec, offs


def put_record_fields(records, keysize: int, elemsize: int, key_slot: int = 0):
    """Views of a put-record batch [m, stride] (uint8): record_fields' tuple
    plus values uint8 [m, elemsize]."""
    rb = put_record_bytes(keysize, elemsize, key_slot)
    if records.dim() != 2 or records.shape[1] != rb:
        raise ValueError(f"records must have shape [m, {rb}], got {tuple(records.shape)}")
    slot = key_slot if key_slot else (keysize + 7) // 8 * 8
    return record_fields(records, keysize) + (records[:, 24 + slot:24 + slot + elemsize],)


def _move_rows(src, index, out, stream, check, scatter):
    torch = _torch()
    name = "scatter_rows" if scatter else "gather_rows"
    rows, B, sstride = _rows_2d(src, "src")
    dev = src.device
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or index.dim() != 1 or \
            not index.is_cuda or index.device != dev:
        raise ValueError(f"index must be a 1-D int32 tensor on {dev}")
    m = index.numel()
    istride = 4 * index.stride(0) if m > 1 else 4
    if istride < 4:
        raise ValueError("index must have a positive stride")
    if scatter and rows != m:
        raise ValueError(f"scatter_rows: src has {rows} rows, index {m} entries")
    if out is None:
        out = torch.empty((m, B), dtype=torch.uint8, device=dev)
    orows, oB, ostride = _rows_2d(out, "out", dev)
    if oB != B or (not scatter and orows != m):
        raise ValueError(f"out must have shape [{'rows' if scatter else m}, {B}], got {tuple(out.shape)}")
    limit = orows if scatter else rows
    if check and m:
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            if not torch.cuda.is_current_stream_capturing():
                top = int((index.to(torch.int64) & 0xFFFFFFFF).max().item())
                if top >= limit:
                    raise ValueError(f"{name}: index {top} is past the {limit} rows it indexes")
    with _on(dev, stream) as g:
        f = lib().pdht_scatter_rows_dev if scatter else lib().pdht_gather_rows_dev
        _check(f(_dptr(src), sstride, B, _dptr(index), istride, m, _dptr(out), ostride, g.stream),
               f"pdht_{name}_dev")
    return out


def gather_rows(src, index, out=None, stream=None, check=True):
    """out[p] = src[index[p]] (include/pdht_hip_put.h pdht_gather_rows_dev): rows
    into bucket order.  src uint8 [rows, B]; index int32 [m] (unsigned row
    numbers, as bucket_batch returns them; a strided view such as
    record_fields(...)[3] is read in place; repeats allowed); out uint8 [m, B]
    (allocated if None).  src and out may be row-strided views at any
    address; bytes of out outside its rows are not written.  check=True reads
    the largest index back on the launch stream (host-synchronous) and
    raises if it is past src's rows; check=False, or during graph capture:
    asynchronous, the caller vouches for the indices."""
    return _move_rows(src, index, out, stream, check, False)


def scatter_rows(src, index, out=None, stream=None, check=True):
    """out[index[p]] = src[p] (pdht_scatter_rows_dev): rows that arrived in
    bucket order -- get replies -- back into the caller's order.  The indices
    must be distinct.  src uint8 [m, B]; index int32 [m]; out uint8 [rows, B]
    (None: [m, B], index a permutation).  Rows of out that no index names keep
    their bytes.  check as for gather_rows, against out's rows."""
    return _move_rows(src, index, out, stream, check, True)


# ------------------------------------------------- device-resident table ---
# The owner's side of a put and a get (include/pdht_hip_table.h; the server
# loop of libmpipdht/init.c:173-290) and the client's resolve (putget.c:50-59).
#   put: bucket_put_records -> dist.exchange_records -> DeviceTable.put_records
#   get: bucket_records(msg_type=get) -> dist.exchange_records -> DeviceTable.get
#        -> dist.exchange_replies -> get_resolve(replies, keys, E, index=...)
#   update: bucket_put_records -> dist.exchange_records -> DeviceTable.update_records
#   claim: bucket_records -> dist.exchange_records -> DeviceTable.cswap
#        -> dist.exchange_replies -> scatter_rows(replies, index)
#   (include/pdht_hip_table_rmw.h: pdht_update, pdht_atomic_cswap)
#   accumulate: bucket_put_records -> dist.exchange_records -> DeviceTable.acc_records
#   (include/pdht_hip_table_acc.h: pdht_acc)
#   create: bucket_put_records -> dist.exchange_records -> DeviceTable.add_records(replies=True)
#        -> dist.exchange_replies -> get_resolve(replies, keys, E, index=...)
#   (include/pdht_hip_table_add.h: the Portals put, the first record of an mbits wins)
#   reduce: bucket_put_records -> dist.exchange_records -> DeviceTable.reduce_records(op, replies=True)
#        -> dist.exchange_replies -> get_resolve(replies, keys, E, index=...)
#   (include/pdht_hip_table_reduce.h: min, max, and, or, xor beside the sum)
#   local: DeviceTable.put_keys(keys, values) / DeviceTable.get_keys(keys, E) -- keys and values already on
#        the table's device: no records, no replies, no sort
#        DeviceTable.update_keys(keys, values) / add_keys(keys, values) / cswap_keys(keys, word_offset, compare,
#        desired) -- the update, create and claim flows the same way
#   (include/pdht_hip_table_keys.h, pdht_hip_table_keys_rmw.h: byte for byte the record flows at nranks = 1)
def table_bytes(capacity: int, rowbytes: int) -> int:
    """Bytes of a DeviceTable's storage: 64 + (capacity + 1) * (16 + rowbytes).
    capacity: a power of two in 64 .. 2^31; rowbytes: a multiple of 8, >= 8."""
    b = lib().pdht_table_bytes(capacity, rowbytes)
    if b == 0:
        raise ValueError(f"capacity {capacity} must be a power of two in 64 .. 2^31 and rowbytes {rowbytes} "
                         "a multiple of 8 that is >= 8 and < 2^31")
    return b


def table_reply_bytes(head: int, rowbytes: int) -> int:
    """Bytes of a get reply: head + rowbytes (head 1 = the packed reply_t of
    libmpipdht/pdht.h:131-135, head 8 = the aligned form)."""
    b = lib().pdht_table_reply_bytes(head, rowbytes)
    if b == 0:
        raise ValueError(f"head {head} must be 1 or 8 and rowbytes {rowbytes} a multiple of 8 that is >= 8")
    return b


def table_export_workspace_bytes(nslots: int) -> int:
    """Bytes of workspace DeviceTable.export needs for a range of `nslots` slots
    (1 .. capacity + 1); a function of nslots only."""
    b = lib().pdht_table_export_workspace_bytes(nslots) if 0 < nslots <= (1 << 31) + 1 else 0
    if b == 0:
        raise ValueError(f"nslots {nslots} must be in 1 .. 2^31 + 1")
    return b


# pdht_acc's datatypes, operation and flag (include/pdht_hip_table_acc.h; the reference's enums)
PDHT_ACC_INT32, PDHT_ACC_INT64, PDHT_ACC_DOUBLE = 0, 1, 2
PDHT_ACC_ADD = 0
PDHT_ACC_INSERT = 1


def table_acc_workspace_bytes(m: int, insert: bool = False) -> int:
    """Bytes of workspace DeviceTable.acc_records needs for m records: 0
    without insert, 4*m + m rounded up to 4 with it."""
    if not 0 <= m < (1 << 32):
        raise ValueError(f"m {m} must be in 0 .. 2^32 - 1")
    return lib().pdht_table_acc_workspace_bytes(m, PDHT_ACC_INSERT if insert else 0)


def table_add_workspace_bytes(m: int) -> int:
    """Bytes of workspace DeviceTable.add_records needs for m records: 4*m +
    m rounded up to 4."""
    if not 0 <= m < (1 << 32):
        raise ValueError(f"m {m} must be in 0 .. 2^32 - 1")
    return lib().pdht_table_add_workspace_bytes(m)


def table_put_keys_workspace_bytes(m: int) -> int:
    """Bytes of workspace DeviceTable.put_keys needs for m keys: 4*m."""
    if not 0 <= m < (1 << 32):
        raise ValueError(f"m {m} must be in 0 .. 2^32 - 1")
    return lib().pdht_table_put_keys_workspace_bytes(m)


def table_update_keys_workspace_bytes(m: int) -> int:
    """Bytes of workspace DeviceTable.update_keys needs for m keys: 4*m."""
    if not 0 <= m < (1 << 32):
        raise ValueError(f"m {m} must be in 0 .. 2^32 - 1")
    return lib().pdht_table_update_keys_workspace_bytes(m)


def table_add_keys_workspace_bytes(m: int) -> int:
    """Bytes of workspace DeviceTable.add_keys needs for m keys: 4*m + m
    rounded up to 4."""
    if not 0 <= m < (1 << 32):
        raise ValueError(f"m {m} must be in 0 .. 2^32 - 1")
    return lib().pdht_table_add_keys_workspace_bytes(m)


def table_cswap_keys_workspace_bytes(m: int) -> int:
    """Bytes of workspace DeviceTable.cswap_keys needs for m keys: 4*m."""
    if not 0 <= m < (1 << 32):
        raise ValueError(f"m {m} must be in 0 .. 2^32 - 1")
    return lib().pdht_table_cswap_keys_workspace_bytes(m)


# the reduce's operations (include/pdht_hip_table_reduce.h)
PDHT_RED_ADD, PDHT_RED_MIN, PDHT_RED_MAX, PDHT_RED_AND, PDHT_RED_OR, PDHT_RED_XOR = 0, 1, 2, 3, 4, 5
_RED_OPS = {"add": PDHT_RED_ADD, "min": PDHT_RED_MIN, "max": PDHT_RED_MAX, "and": PDHT_RED_AND, "or": PDHT_RED_OR,
            "xor": PDHT_RED_XOR}


def table_reduce_workspace_bytes(m: int, insert: bool = False, replies: bool = False) -> int:
    """Bytes of workspace DeviceTable.reduce_records needs for m records: 0
    without insert and replies, 4*m with replies only, 4*m + m rounded up to
    4 with insert."""
    if not 0 <= m < (1 << 32):
        raise ValueError(f"m {m} must be in 0 .. 2^32 - 1")
    return lib().pdht_table_reduce_workspace_bytes(m, PDHT_ACC_INSERT if insert else 0, 1 if replies else 0)


def _red_op(op, dtype):
    """op: a PDHT_RED_* int or its name -> the int; the bitwise ones are not
    defined for float64."""
    if isinstance(op, str):
        if op not in _RED_OPS:
            raise ValueError(f"op must be one of {sorted(_RED_OPS)} or a PDHT_RED_* constant, got {op!r}")
        op = _RED_OPS[op]
    if not isinstance(op, int) or isinstance(op, bool) or not PDHT_RED_ADD <= op <= PDHT_RED_XOR:
        raise ValueError(f"op must be one of {sorted(_RED_OPS)} or a PDHT_RED_* constant, got {op!r}")
    if op >= PDHT_RED_AND and dtype == _torch().float64:
        raise ValueError("op and / or / xor is defined for torch.int32 and torch.int64 only")
    return op


def _acc_datatype(dtype):
    torch = _torch()
    kinds = {torch.int32: (PDHT_ACC_INT32, 4), torch.int64: (PDHT_ACC_INT64, 8),
             torch.float64: (PDHT_ACC_DOUBLE, 8)}
    if dtype not in kinds:
        raise ValueError(f"dtype must be torch.int32, torch.int64 or torch.float64, got {dtype!r}")
    return kinds[dtype]


def _strided_1d(t, name, dtype, device):
    """t: a 1-D CUDA tensor of `dtype` on `device`, dense or strided (a column
    of a wider tensor) -> (entries, stride in bytes)."""
    torch = _torch()
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 1 or not t.is_cuda or t.device != device:
        raise ValueError(f"{name} must be a 1-D {dtype} CUDA tensor on {device}")
    m = t.shape[0]
    stride = t.stride(0) * t.element_size() if m > 1 else t.element_size()
    if stride < t.element_size():
        raise ValueError(f"{name} must have a positive stride")
    return m, stride


class DeviceTable:
    """A target table in device memory: opaque rows of `rowbytes` bytes under
    64-bit mbits (include/pdht_hip_table.h).  For put records rowbytes is the
    record stride - 24 (key slot + padded value).  `storage`: a uint8 CUDA
    tensor of at least table_bytes(capacity, rowbytes) bytes, 16-byte aligned
    (allocated if None); it is emptied here.  Calls on one stream are ordered
    by the stream; concurrent calls on one table from different streams are
    undefined."""

    def __init__(self, capacity: int, rowbytes: int, device="cuda", storage=None):
        torch = _torch()
        self.capacity, self.rowbytes = int(capacity), int(rowbytes)
        self.nbytes = table_bytes(self.capacity, self.rowbytes)
        if storage is None:
            device = torch.device(device)
            if device.type != "cuda":
                raise ValueError("a DeviceTable lives on a CUDA device")
            if device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            storage = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        else:
            if not isinstance(storage, torch.Tensor) or not storage.is_cuda:
                raise ValueError("storage must be a CUDA uint8 tensor")
            _need(storage, "storage", torch.uint8, storage.device, numel=self.nbytes)
            if storage.data_ptr() % 16:
                raise ValueError("storage must be 16-byte aligned")
        self.storage = storage
        self.device = storage.device
        self.clear()

    def clear(self, stream=None):
        """Empties the table and its counters (pdht_table_init_dev)."""
        with _on(self.device, stream) as g:
            _check(lib().pdht_table_init_dev(_dptr(self.storage), self.storage.numel(), self.capacity,
                                             self.rowbytes, g.stream), "pdht_table_init_dev")

    def put_records(self, records, status=True, workspace=None, stream=None):
        """Applies a batch of put records [m, stride] (uint8, 8-byte aligned,
        stride >= 24 + rowbytes; bucket_put_records' or forged ones: only the
        mbits at +16 and the row at +24 are read) as init.c:223-241 would one
        after the other: the last record of an mbits leaves its row.
        status: True = return a new uint8 [m] (0 stored / 1 superseded by a
        later record of the batch / 2 dropped, table full), a uint8 [m] tensor
        = fill and return it, False / None = none.  workspace: uint8, >= 4*m
        bytes (allocated if None)."""
        return self._apply_records("put", records, status, workspace, stream)

    def update_records(self, records, status=True, workspace=None, stream=None):
        """Applies a batch of put records as pdht_update would one after the
        other (libpdht/putget.c:278; pdht_table_update_records_dev): find by
        mbits, overwrite the row if the entry is there, do nothing otherwise.
        Arguments as put_records.  status: 0 stored / 1 superseded by a later
        record of the batch / 3 not found.  Nothing is ever inserted or
        dropped; counts()[2] advances by one."""
        return self._apply_records("update", records, status, workspace, stream)

    # The arguments that the records operations share, each checked in one place

    def _records_arg(self, records):
        """-> (m, row stride in bytes) of a batch of put records."""
        m, B, stride = _rows_2d(records, "records", self.device)
        if B < 24 + self.rowbytes:
            raise ValueError(f"records must have >= {24 + self.rowbytes} bytes per row, got {B}")
        if stride % 8 or records.data_ptr() % 8:
            raise ValueError("records must be 8-byte aligned with a row stride that is a multiple of 8")
        return m, stride

    def _status_arg(self, status, m):
        """True -> a new uint8 [m]; False / None -> None; a tensor is checked."""
        torch = _torch()
        if status is True:
            return torch.empty(m, dtype=torch.uint8, device=self.device)
        if status is False or status is None:
            return None
        _need(status, "status", torch.uint8, self.device, shape=(m,))
        return status

    def _replies_arg(self, replies, m):
        """True -> new head-8 replies; False / None -> None; a tensor is
        checked.  -> (replies, their row stride in bytes)."""
        torch = _torch()
        rb = 8 + self.rowbytes
        if replies is True:
            replies = torch.empty((m, rb // 8), dtype=torch.int64, device=self.device).view(torch.uint8).view(m, rb)
        elif replies is False or replies is None:
            return None, 0
        om, oB, rstride = _rows_2d(replies, "replies", self.device)
        if (om, oB) != (m, rb):
            raise ValueError(f"replies must have shape [{m}, {rb}], got {tuple(replies.shape)}")
        if rstride % 8 or replies.data_ptr() % 8:
            raise ValueError("replies must be 8-byte aligned with a row stride that is a multiple of 8")
        return replies, rstride

    def _workspace_arg(self, workspace, need):
        """None -> a new workspace of `need` bytes; a tensor is checked."""
        torch = _torch()
        if workspace is None:
            return torch.empty(max(need // 4, 1), dtype=torch.int32, device=self.device).view(torch.uint8)
        _need(workspace, "workspace", torch.uint8, self.device, numel=need)
        if workspace.data_ptr() % 4:
            raise ValueError("workspace must be 4-byte aligned")
        return workspace

    def _region_arg(self, size, value_offset, elems):
        """The region of an accumulate or a reduce inside the row."""
        for name, v in (("value_offset", value_offset), ("elems", elems)):
            if not isinstance(v, int) or isinstance(v, bool) or v < 0:
                raise ValueError(f"{name} must be a non-negative int, got {v!r}")
        if value_offset % size or elems < 1 or value_offset + elems * size > self.rowbytes:
            raise ValueError(f"the region must be elems >= 1 elements of {size} bytes at a value_offset that is a "
                             f"multiple of {size}, inside the {self.rowbytes}-byte row; got value_offset "
                             f"{value_offset}, elems {elems}")

    def _apply_records(self, kind, records, status, workspace, stream):
        m, stride = self._records_arg(records)
        status = self._status_arg(status, m)
        need = getattr(lib(), f"pdht_table_{kind}_workspace_bytes")(m)
        workspace = self._workspace_arg(workspace, need)
        with _on(self.device, stream) as g:
            name = f"pdht_table_{kind}_records_dev"
            _check(getattr(lib(), name)(_dptr(self.storage), self.capacity, self.rowbytes, _dptr(records), stride, m,
                                        _dptr(workspace), workspace.numel(), _opt(status), g.stream), name)
        return status

    def acc_records(self, records, dtype, value_offset: int, elems: int = 1, insert: bool = False, status=True,
                    workspace=None, stream=None):
        """Applies a batch of put records as pdht_acc would one after the
        other (libpdht/pdht.h:349, AssocOpAdd; pdht_table_acc_records_dev):
        find by mbits and add the `elems` elements of `dtype` (torch.int32,
        torch.int64 or torch.float64) at `value_offset` of the record's row
        into the same place of the entry's row; no other byte of a present
        entry changes.  value_offset: a multiple of the element size, the
        region inside the row.  insert=False: an absent mbits stays absent
        (status 3) and no counter moves.  insert=True: an absent mbits is
        created with the whole row of its first record in the batch, later
        records of it add; a new mbits without a free slot is dropped
        (status 2) as by put_records, and counts() advance as for a put.
        status: 0 added / 2 dropped / 3 not found (True, a uint8 [m] tensor,
        or False / None as in put_records).  Integers wrap and the result is
        byte-exact; float64 sums are added in an order the schedule picks
        (within n*u/(1 - n*u) * sum|x_i| of the exact sum, u = 2^-53, while
        no partial sum overflows).  NaN and infinities propagate as IEEE
        addition has it in any order: a NaN among old value and addends gives
        NaN, +inf alone +inf, -inf alone -inf, both NaN, and addends of one
        sign whose exact sum passes DBL_MAX give that infinity.  Subnormals
        are not flushed: multiples of 2^-1074 whose magnitudes sum to less
        than 2^53 of them add exactly.  The table must be in ordinary device
        memory.  workspace: uint8, >=
        table_acc_workspace_bytes(m, insert) bytes (allocated if None)."""
        datatype, size = _acc_datatype(dtype)
        self._region_arg(size, value_offset, elems)
        m, stride = self._records_arg(records)
        status = self._status_arg(status, m)
        flags = PDHT_ACC_INSERT if insert else 0
        need = lib().pdht_table_acc_workspace_bytes(m, flags)
        workspace = self._workspace_arg(workspace, need)
        with _on(self.device, stream) as g:
            _check(lib().pdht_table_acc_records_dev(_dptr(self.storage), self.capacity, self.rowbytes, _dptr(records),
                                                    stride, m, datatype, PDHT_ACC_ADD, value_offset, elems, flags,
                                                    _dptr(workspace), workspace.numel(), _opt(status), g.stream),
                   "pdht_table_acc_records_dev")
        return status

    def reduce_records(self, records, dtype, op, value_offset: int, elems: int = 1, insert: bool = False,
                       status=True, replies=None, workspace=None, stream=None):
        """acc_records with an operation of the caller's choice, and with
        replies (pdht_table_reduce_records_dev): find by mbits and set the
        `elems` elements of `dtype` at `value_offset` of the entry's row to
        op(entry's, record's); no other byte of a present entry changes.
        op: a PDHT_RED_* constant or "add", "min", "max", "and", "or", "xor".
        add is acc_records' sum.  min and max compare torch.int32 /
        torch.int64 as signed integers and torch.float64 by IEEE 754
        totalOrder on the 64 bits (-NaN < -inf < .. < -0.0 < +0.0 < .. < +inf
        < +NaN): the result is one operand's bits, NaNs and subnormals
        included.  and, or, xor are bitwise, for the integer types only.
        Every op but add on float64 is byte-exact against the records applied
        one after the other, and the same on every run.  dtype, value_offset,
        elems, insert, status (0 applied / 2 dropped / 3 not found) and
        counts() as in acc_records.  replies as in add_records: None / False
        = none; True = a new uint8 [m, 8 + rowbytes]; a uint8 [m, 8 +
        rowbytes] tensor or row-strided view (8-byte aligned, row stride a
        multiple of 8) = filled.  Reply p is the head-8 reply a get after the
        call would give for record p's mbits -- the reduced entry, or byte 0
        = 0 and zeros for a record with status 2 or 3.  Returns status
        without replies, (status, replies) with them.  workspace: uint8, >=
        table_reduce_workspace_bytes(m, insert, replies) bytes (allocated if
        None)."""
        datatype, size = _acc_datatype(dtype)
        op = _red_op(op, dtype)
        self._region_arg(size, value_offset, elems)
        m, stride = self._records_arg(records)
        status = self._status_arg(status, m)
        replies, rstride = self._replies_arg(replies, m)
        flags = PDHT_ACC_INSERT if insert else 0
        need = lib().pdht_table_reduce_workspace_bytes(m, flags, 1 if replies is not None else 0)
        workspace = self._workspace_arg(workspace, need)
        with _on(self.device, stream) as g:
            _check(lib().pdht_table_reduce_records_dev(_dptr(self.storage), self.capacity, self.rowbytes,
                                                       _dptr(records), stride, m, datatype, op, value_offset, elems,
                                                       flags, _dptr(workspace), workspace.numel(), _opt(status),
                                                       _opt(replies), rstride, g.stream),
                   "pdht_table_reduce_records_dev")
        return status if replies is None else (status, replies)

    def add_records(self, records, status=True, replies=None, workspace=None, stream=None):
        """Applies a batch of put records as the Portals put would one after
        the other (libpdht/poll.c:205-263; pdht_table_add_records_dev): find
        by mbits, insert the record's row if the entry is absent, do nothing
        if it is there.  The first record of a new mbits wins, an entry that
        is present keeps every byte.  records, status (True, a uint8 [m]
        tensor, or False / None) and counts() as in put_records; status: 0
        created by this record / 4 exists, from before or from an earlier
        record of the batch / 2 dropped, table full.  replies: None / False =
        none; True = a new uint8 [m, 8 + rowbytes]; a uint8 [m, 8 + rowbytes]
        tensor or row-strided view (8-byte aligned, row stride a multiple of
        8) = filled.  Reply p is the head-8 reply a get after the call would
        give for record p's mbits (byte 0 = 0 and zeros for a dropped one),
        for dist.exchange_replies and get_resolve.  Returns status without
        replies, (status, replies) with them.  workspace: uint8, >=
        table_add_workspace_bytes(m) bytes (allocated if None)."""
        m, stride = self._records_arg(records)
        status = self._status_arg(status, m)
        replies, rstride = self._replies_arg(replies, m)
        need = lib().pdht_table_add_workspace_bytes(m)
        workspace = self._workspace_arg(workspace, need)
        with _on(self.device, stream) as g:
            _check(lib().pdht_table_add_records_dev(_dptr(self.storage), self.capacity, self.rowbytes, _dptr(records),
                                                    stride, m, _dptr(workspace), workspace.numel(), _opt(status),
                                                    _opt(replies), rstride, g.stream), "pdht_table_add_records_dev")
        return status if replies is None else (status, replies)

    def get(self, mbits_or_records, head: int = 8, out=None, stream=None):
        """Answers a batch of requests as init.c:192-220 does: replies uint8
        [m, head + rowbytes], byte 0 = 1 found / 0 not found, bytes 1..head-1
        zero, then the row (zeros when not found).  A 1-D int64 tensor is read
        as dense mbits; a 2-D uint8 record batch (bucket_records' or put
        records) is read in place at +16 with its row stride.  out: a uint8
        [m, head + rowbytes] tensor or row-strided view at any address; bytes
        outside its rows are not written."""
        torch = _torch()
        rb = table_reply_bytes(head, self.rowbytes)
        m, ptr, stride = self._requests(mbits_or_records)
        if out is None:
            out = torch.empty((m, rb // 8 if head == 8 else rb), dtype=torch.int64 if head == 8 else torch.uint8,
                              device=self.device).view(torch.uint8).view(m, rb)
        om, oB, ostride = _rows_2d(out, "out", self.device)
        if (om, oB) != (m, rb):
            raise ValueError(f"out must have shape [{m}, {rb}], got {tuple(out.shape)}")
        with _on(self.device, stream) as g:
            _check(lib().pdht_table_get_dev(_dptr(self.storage), self.capacity, self.rowbytes, C.c_void_p(ptr),
                                            stride, m, _dptr(out), ostride, head, g.stream), "pdht_table_get_dev")
        return out

    def _requests(self, t):
        """(m, address of the first mbits, stride) of a batch of requests: a
        1-D int64 tensor of dense mbits, or a 2-D uint8 record batch read in
        place at +16."""
        torch = _torch()
        if isinstance(t, torch.Tensor) and t.dim() == 1 and t.dtype == torch.int64:
            _need(t, "mbits", torch.int64, self.device)
            return t.numel(), t.data_ptr(), 8
        if isinstance(t, torch.Tensor) and t.dim() == 2 and t.dtype == torch.uint8:
            m, B, stride = _rows_2d(t, "records", self.device)
            if B < 24:
                raise ValueError(f"records must have >= 24 bytes per row, got {B}")
            if stride % 8 or t.data_ptr() % 8:
                raise ValueError("records must be 8-byte aligned with a row stride that is a multiple of 8")
            return m, t.data_ptr() + 16, stride
        raise ValueError("expected a 1-D int64 tensor of mbits or a 2-D uint8 record batch")

    def cswap(self, mbits_or_records, word_offset: int, compare: int, desired: int, out=None, workspace=None,
              stream=None):
        """Compare-and-swap of the uint64 at `word_offset` of the row of every
        request, as pdht_atomic_cswap would one request after the other
        (libpdht/atomics.c:81-154; pdht_table_cswap_dev): old = word; if word
        == compare: word = desired.  Requests as in get (dense int64 mbits, or
        records read in place at +16).  compare / desired: one pair per call,
        any int in [-2^63, 2^64), passed as its 64-bit pattern.  Returns the
        replies, uint8 [m, 16]: byte 0 = 1 found / 0 not found, bytes 1..7
        zero, bytes 8..15 the old word (0 when not found) -- a head-8 get
        reply of an 8-byte row, for dist.exchange_replies and scatter_rows.
        Among the requests of one mbits only the first can see `compare`.
        Nothing is inserted.  out: a uint8 [m, 16] tensor or row-strided view,
        8-byte aligned with a stride that is a multiple of 8; workspace:
        uint8, >= 4*m bytes (allocated if None)."""
        m, ptr, stride = self._requests(mbits_or_records)
        pair, out, ostride = self._cswap_args(m, word_offset, compare, desired, out)
        workspace = self._workspace_arg(workspace, lib().pdht_table_cswap_workspace_bytes(m))
        with _on(self.device, stream) as g:
            _check(lib().pdht_table_cswap_dev(_dptr(self.storage), self.capacity, self.rowbytes, C.c_void_p(ptr),
                                              stride, m, word_offset, pair[0], pair[1], _dptr(out), ostride,
                                              _dptr(workspace), workspace.numel(), g.stream), "pdht_table_cswap_dev")
        return out

    def _cswap_args(self, m, word_offset, compare, desired, out):
        """The arguments that cswap and cswap_keys share -> ((compare,
        desired) as 64-bit patterns, out, its row stride in bytes)."""
        torch = _torch()
        if not isinstance(word_offset, int) or word_offset < 0 or word_offset % 8 or \
                word_offset + 8 > self.rowbytes:
            raise ValueError(f"word_offset must be a multiple of 8 in 0 .. {self.rowbytes - 8}, got {word_offset}")
        pair = []
        for name, v in (("compare", compare), ("desired", desired)):
            if not isinstance(v, int) or isinstance(v, bool) or not -(1 << 63) <= v < (1 << 64):
                raise ValueError(f"{name} must be an int in [-2^63, 2^64), got {v!r}")
            pair.append(v & ((1 << 64) - 1))
        if out is None:
            out = torch.empty((m, 2), dtype=torch.int64, device=self.device).view(torch.uint8).view(m, 16)
        om, oB, ostride = _rows_2d(out, "out", self.device)
        if (om, oB) != (m, 16):
            raise ValueError(f"out must have shape [{m}, 16], got {tuple(out.shape)}")
        if ostride % 8 or out.data_ptr() % 8:
            raise ValueError("out must be 8-byte aligned with a row stride that is a multiple of 8")
        return pair, out, ostride

    # ---- by key (include/pdht_hip_table_keys.h, pdht_hip_table_keys_rmw.h) ----

    def _packed_keys_arg(self, keys, route):
        """-> (m, keysize) of a batch of packed keys of 1 .. 64 bytes; route:
        where longer keys go, for the message."""
        m, L, kstride = _keys_2d(keys)
        if keys.device != self.device or kstride != L:
            raise ValueError(f"keys must be packed and on {self.device}")
        if not 1 <= L <= 64:
            raise ValueError(f"keys must have 1 .. 64 bytes, got {L}: longer keys go through {route}")
        return m, L

    def _keys_arg(self, keys, elemsize, key_slot):
        """-> (m, keysize) of a batch of packed keys whose rows of `elemsize`
        value bytes behind a key slot are this table's rows."""
        m, L = self._packed_keys_arg(keys, "bucket_put_records and put_records (get: bucket_records, get, "
                                           "get_resolve)")
        if not isinstance(elemsize, int) or isinstance(elemsize, bool) or elemsize < 1:
            raise ValueError("elemsize must be >= 1")
        if not isinstance(key_slot, int) or isinstance(key_slot, bool) or key_slot < 0 or \
                (key_slot and (key_slot % 8 or key_slot < L)):
            raise ValueError(f"key_slot {key_slot} must be 0 or a multiple of 8 that is >= keysize {L}")
        slot = key_slot if key_slot else (L + 7) // 8 * 8
        if self.rowbytes != (slot + elemsize + 7) // 8 * 8:
            raise ValueError(f"rowbytes {self.rowbytes} must be the key slot {slot} + elemsize {elemsize} rounded up "
                             f"to 8 (put_record_bytes(keysize, elemsize, key_slot) - 24)")
        return m, L

    def _mbits_arg(self, mbits, m):
        """True -> a new int64 [m]; False / None -> None; a tensor is checked."""
        torch = _torch()
        if mbits is True:
            return torch.empty(m, dtype=torch.int64, device=self.device)
        if mbits is False or mbits is None:
            return None
        return _need(mbits, "mbits", torch.int64, self.device, shape=(m,))

    def put_keys(self, keys, values, *, key_slot: int = 0, status=True, mbits=None, workspace=None, stream=None):
        """Stores values[i] under keys[i] (pdht_table_put_keys_dev): what
        bucket_put_records(keys, values, nranks=1, key_slot=key_slot) ->
        put_records leaves, table, status and counts()[:3] byte for byte,
        without records: mbits = CityHash64(key), the row is the key, zeros up
        to the key slot, the value, zeros up to 8, and the last key of an
        mbits leaves its row.  keys [m, L] packed uint8, L in 1 .. 64; values
        [m, E] uint8, a row-strided view at any address is accepted; rowbytes
        must be slot + E rounded up to 8.  status as put_records (0 stored / 1
        superseded / 2 dropped).  mbits: None / False = none; True = a new
        int64 [m], a tensor = filled: the digests, for a later get or cswap by
        mbits.  Returns status, or (status, mbits) with mbits.  workspace:
        uint8, >= table_put_keys_workspace_bytes(m) bytes (allocated if None).
        counts()[2] advances by one."""
        return self._apply_keys("put", keys, values, key_slot, status, mbits, workspace, stream)

    def _apply_keys(self, kind, keys, values, key_slot, status, mbits, workspace, stream):
        nv, E, vstride = _rows_2d(values, "values", self.device)
        m, L = self._keys_arg(keys, E, key_slot)
        if nv != m:
            raise ValueError(f"values must have one row per key: {nv} rows for {m} keys")
        status = self._status_arg(status, m)
        mbits = self._mbits_arg(mbits, m)
        workspace = self._workspace_arg(workspace, getattr(lib(), f"pdht_table_{kind}_keys_workspace_bytes")(m))
        with _on(self.device, stream) as g:
            name = f"pdht_table_{kind}_keys_dev"
            _check(getattr(lib(), name)(_dptr(self.storage), self.capacity, self.rowbytes, _dptr(keys), L, key_slot,
                                        _dptr(values), E, vstride, m, _dptr(workspace), workspace.numel(),
                                        _opt(mbits), _opt(status), g.stream), name)
        return status if mbits is None else (status, mbits)

    def update_keys(self, keys, values, *, key_slot: int = 0, status=True, mbits=None, workspace=None, stream=None):
        """Overwrites the rows under keys that have an entry
        (pdht_table_update_keys_dev): what bucket_put_records(keys, values,
        nranks=1, key_slot=key_slot) -> update_records leaves, table, status
        and counts() byte for byte, without records.  Matching is by mbits =
        CityHash64(key) alone; the whole row -- key, zeros up to the key slot,
        value, zeros up to 8 -- replaces the entry's, and the last key of an
        mbits leaves its row.  Nothing is inserted.  Arguments and return as
        put_keys; status: 0 stored / 1 superseded / 3 not found.  workspace:
        uint8, >= table_update_keys_workspace_bytes(m) bytes (allocated if
        None).  counts()[2] advances by one."""
        return self._apply_keys("update", keys, values, key_slot, status, mbits, workspace, stream)

    def add_keys(self, keys, values, *, key_slot: int = 0, status=True, mbits=None, workspace=None, stream=None):
        """Inserts values[i] under keys[i] where no entry is
        (pdht_table_add_keys_dev): what bucket_put_records(keys, values,
        nranks=1, key_slot=key_slot) -> add_records leaves, table, status and
        counts()[:3] byte for byte, without records.  The first key of a new
        mbits wins, an entry that is present keeps every byte.  Arguments and
        return as put_keys; status: 0 created by this key / 4 exists / 2
        dropped, table full.  There are no replies: get_keys reads the
        entries.  workspace: uint8, >= table_add_keys_workspace_bytes(m) bytes
        (allocated if None).  counts() advance as for add_records."""
        return self._apply_keys("add", keys, values, key_slot, status, mbits, workspace, stream)

    def cswap_keys(self, keys, word_offset: int, compare: int, desired: int, *, out=None, mbits=None, workspace=None,
                   stream=None):
        """cswap by key (pdht_table_cswap_keys_dev): what bucket_records(keys,
        1) -> cswap(records, word_offset, compare, desired) leaves, table,
        replies and counts() byte for byte, without records.  keys [m, L]
        packed uint8, L in 1 .. 64, matched by mbits = CityHash64(key) alone.
        word_offset, compare, desired and out as in cswap; reply i is key i's.
        mbits as in put_keys.  Returns the replies uint8 [m, 16], or (replies,
        mbits) with mbits.  workspace: uint8, >=
        table_cswap_keys_workspace_bytes(m) bytes (allocated if None)."""
        m, L = self._packed_keys_arg(keys, "bucket_records and cswap")
        pair, out, ostride = self._cswap_args(m, word_offset, compare, desired, out)
        mbits = self._mbits_arg(mbits, m)
        workspace = self._workspace_arg(workspace, lib().pdht_table_cswap_keys_workspace_bytes(m))
        with _on(self.device, stream) as g:
            _check(lib().pdht_table_cswap_keys_dev(_dptr(self.storage), self.capacity, self.rowbytes, _dptr(keys), L,
                                                   m, word_offset, pair[0], pair[1], _dptr(out), ostride,
                                                   _dptr(workspace), workspace.numel(), _opt(mbits), g.stream),
                   "pdht_table_cswap_keys_dev")
        return out if mbits is None else (out, mbits)

    def get_keys(self, keys, elemsize: int, *, key_slot: int = 0, values=None, status=None, mbits=None, stream=None):
        """Reads the values under keys (pdht_table_get_keys_dev): what
        bucket_records(keys, 1) -> get -> get_resolve(replies, keys, elemsize,
        key_slot=key_slot) leaves, without records or replies.  status[i] = 2
        no entry / 3 collision (the row's key differs from keys[i]) / 0 found,
        and values[i] receives the row's value when 0.  Returns (values uint8
        [m, elemsize], status uint8 [m]); rows whose status is not 0 keep their
        bytes (new values start as zeros, new status as 2).  values may be a
        row-strided view at any address.  mbits: an int64 [m] tensor receives
        the digests.  Repeated keys are allowed; the table is not written."""
        torch = _torch()
        m, L = self._keys_arg(keys, elemsize, key_slot)
        if values is None:
            values = torch.zeros((m, elemsize), dtype=torch.uint8, device=self.device)
        vn, vE, vstride = _rows_2d(values, "values", self.device)
        if (vn, vE) != (m, elemsize):
            raise ValueError(f"values must have shape [{m}, {elemsize}], got {tuple(values.shape)}")
        if status is None:
            status = torch.full((m,), 2, dtype=torch.uint8, device=self.device)
        _need(status, "status", torch.uint8, self.device, shape=(m,))
        if mbits is not None:
            _need(mbits, "mbits", torch.int64, self.device, shape=(m,))
        with _on(self.device, stream) as g:
            _check(lib().pdht_table_get_keys_dev(_dptr(self.storage), self.capacity, self.rowbytes, _dptr(keys), L,
                                                 key_slot, m, _dptr(values), elemsize, vstride, _opt(mbits),
                                                 _dptr(status), g.stream), "pdht_table_get_keys_dev")
        return values, status

    def counts_dev(self, out=None, stream=None):
        """The four counters as an int64 [4] CUDA tensor, asynchronously."""
        torch = _torch()
        if out is None:
            out = torch.empty(4, dtype=torch.int64, device=self.device)
        _need(out, "out", torch.int64, self.device, shape=(4,))
        with _on(self.device, stream) as g:
            _check(lib().pdht_table_counts_dev(_dptr(self.storage), _dptr(out), g.stream), "pdht_table_counts_dev")
        return out

    def counts(self):
        """(entries stored, records dropped, batches applied -- put, update,
        cswap, inserting accumulate, add and the keyed put, update, add and
        cswap --, slots inspected by puts, inserting accumulates, adds, keyed
        puts and keyed adds); the last three cumulative.
        Host-synchronous."""
        return tuple(int(x) for x in self.counts_dev().cpu().tolist())

    # ---- enumerate and grow (include/pdht_hip_table_iter.h) ----
    def _slot_range(self, first_slot, nslots):
        first_slot = int(first_slot)
        nslots = self.capacity + 1 - first_slot if nslots is None else int(nslots)
        if first_slot < 0 or nslots < 1 or first_slot + nslots > self.capacity + 1:
            raise ValueError(f"slots [{first_slot}, {first_slot + nslots}) are not a non-empty range inside "
                             f"0 .. {self.capacity + 1}")
        return first_slot, nslots

    def export(self, mbits, rows=None, slots=None, *, first_slot=0, nslots=None, count=None, workspace=None,
               stream=None):
        """The live slots of [first_slot, first_slot + nslots) (slots 0 ..
        capacity, the last one mbits 0's private slot; nslots None = to the
        end) in ascending slot order, asynchronously: entry e < len(mbits)
        goes to mbits[e] (int64, 1-D), rows[e] (uint8 [m, rowbytes]) and
        slots[e] (int32, 1-D); rows and slots may be None.  All three may be
        row-strided views -- of one [m, stride] uint8 record buffer for the
        record form (export_records).  Nothing else is written.  A tensor of 0
        entries (or None) for mbits is the count-only form.  Returns the int64
        [2] count tensor (`count`, allocated if None): live slots of the
        range, entries written.  Page by resuming at slots[last] + 1.
        workspace: uint8, >= table_export_workspace_bytes(nslots) bytes,
        16-byte aligned (allocated if None); its contents are never read."""
        torch = _torch()
        first_slot, nslots = self._slot_range(first_slot, nslots)
        m, mp, ms, rp, rs, sp, ss = 0, None, 8, None, 8, None, 4
        if mbits is not None:
            m, ms = _strided_1d(mbits, "mbits", torch.int64, self.device)
        if m:
            mp = mbits.data_ptr()
            if ms % 8:
                raise ValueError("mbits must have a byte stride that is a multiple of 8")
            if rows is not None:
                rm, rB, rs = _rows_2d(rows, "rows", self.device)
                if (rm, rB) != (m, self.rowbytes):
                    raise ValueError(f"rows must have shape [{m}, {self.rowbytes}], got {tuple(rows.shape)}")
                if rs % 8 or rows.data_ptr() % 8:
                    raise ValueError("rows must be 8-byte aligned with a row stride that is a multiple of 8")
                rp = rows.data_ptr()
            if slots is not None:
                sm, ss = _strided_1d(slots, "slots", torch.int32, self.device)
                if sm != m:
                    raise ValueError(f"slots must have {m} entries, got {sm}")
                sp = slots.data_ptr()
        if count is None:
            count = torch.empty(2, dtype=torch.int64, device=self.device)
        _need(count, "count", torch.int64, self.device, shape=(2,))
        need = table_export_workspace_bytes(nslots)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        else:
            _need(workspace, "workspace", torch.uint8, self.device, numel=need)
            if workspace.data_ptr() % 16:
                raise ValueError("workspace must be 16-byte aligned")
        with _on(self.device, stream) as g:
            _check(lib().pdht_table_export_dev(_dptr(self.storage), self.capacity, self.rowbytes, first_slot, nslots,
                                               mp, ms, rp, rs, sp, ss, m, _dptr(count), _dptr(workspace),
                                               workspace.numel(), g.stream), "pdht_table_export_dev")
        return count

    def export_records(self, records, *, first_slot=0, nslots=None, count=None, workspace=None, stream=None):
        """export() in the record form: entry e becomes put record e of
        `records` (uint8 [m, stride], 8-byte aligned, stride a multiple of 8
        and >= 24 + rowbytes): slot index at +12, mbits at +16, row at +24;
        bytes +0 .. +11 and the pad behind the row keep what they held.  The
        first count[1] records feed put_records of another table as they
        stand."""
        torch = _torch()
        m, S, stride = _rows_2d(records, "records", self.device)
        if S < 24 + self.rowbytes:
            raise ValueError(f"records must have >= {24 + self.rowbytes} bytes per row, got {S}")
        if stride % 8 or records.data_ptr() % 8:
            raise ValueError("records must be 8-byte aligned with a row stride that is a multiple of 8")
        if m == 0:
            return self.export(None, first_slot=first_slot, nslots=nslots, count=count, workspace=workspace,
                               stream=stream)
        mb = records[:, 16:24].view(torch.int64)[:, 0]  # three views of the one buffer
        sl = records[:, 12:16].view(torch.int32)[:, 0]
        return self.export(mb, records[:, 24:24 + self.rowbytes], sl, first_slot=first_slot, nslots=nslots,
                           count=count, workspace=workspace, stream=stream)

    def entries(self, first_slot=0, nslots=None):
        """The entries of a slot range in slot order, trimmed: (mbits int64
        [e], rows uint8 [e, rowbytes], slots int32 [e]).  Host-synchronous
        (it reads the count before it allocates), like counts()."""
        torch = _torch()
        first_slot, nslots = self._slot_range(first_slot, nslots)
        ws = torch.empty(table_export_workspace_bytes(nslots), dtype=torch.uint8, device=self.device)
        e = int(self.export(None, first_slot=first_slot, nslots=nslots, workspace=ws).cpu()[0])
        mbits = torch.empty(e, dtype=torch.int64, device=self.device)
        rows = torch.empty((e, self.rowbytes // 8), dtype=torch.int64, device=self.device).view(torch.uint8)
        rows = rows.view(e, self.rowbytes)
        slots = torch.empty(e, dtype=torch.int32, device=self.device)
        if e:
            self.export(mbits, rows, slots, first_slot=first_slot, nslots=nslots, workspace=ws)
        return mbits, rows, slots

    def rehash(self, capacity: int, storage=None, chunk_bytes: int = 256 << 20, stream=None):
        """A new DeviceTable of `capacity` and the same rowbytes holding this
        table's entries; this table is left untouched.  rehash = export as
        records -> put_records: the slots are walked in ranges whose record
        buffer stays within chunk_bytes, each exported with room for every
        slot of the range (a chunk is never cut), and put with exactly the
        count it returned.  put_records takes its m from the host, so this is
        host-synchronous -- one count read per chunk -- and cannot be captured
        into a graph.  Raises ValueError before anything is allocated when the
        ordinary entries (all but mbits 0, which has its private slot on both
        sides) exceed `capacity`.  The new table's counters: entries as here,
        dropped 0, batches = the chunks that held an entry."""
        torch = _torch()
        capacity = int(capacity)
        table_bytes(capacity, self.rowbytes)  # the geometry, before anything else
        if chunk_bytes < 1:
            raise ValueError("chunk_bytes must be >= 1")
        entries = self.counts()[0]
        if entries > capacity + 1:
            raise ValueError(f"{entries} entries do not fit a capacity of {capacity}")
        if entries == capacity + 1:  # fits only with mbits 0 among them
            if int(self.export(None, first_slot=self.capacity, nslots=1).cpu()[0]) == 0:
                raise ValueError(f"{entries} ordinary entries do not fit a capacity of {capacity}")
        new = DeviceTable(capacity, self.rowbytes, self.device, storage=storage)
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream(self.device))
        S = 24 + self.rowbytes
        per = max(1, min(self.capacity + 1, chunk_bytes // S))
        records = torch.empty((per, S // 8), dtype=torch.int64, device=self.device).view(torch.uint8).view(per, S)
        ws = torch.empty(table_export_workspace_bytes(per), dtype=torch.uint8, device=self.device)
        pws = torch.empty(max(per, 1), dtype=torch.int32, device=self.device).view(torch.uint8)
        count = torch.empty(2, dtype=torch.int64, device=self.device)
        for s0 in range(0, self.capacity + 1, per):
            n = min(per, self.capacity + 1 - s0)
            self.export_records(records[:n], first_slot=s0, nslots=n, count=count, workspace=ws, stream=stream)
            if stream is not None:
                stream.synchronize()
            c = int(count.cpu()[1])
            if c:
                new.put_records(records[:c], status=False, workspace=pws, stream=stream)
        return new


def get_resolve(replies, keys, elemsize: int, *, head: int = 8, key_slot: int = 0, index=None, values=None,
                status=None, stream=None):
    """The client's side of a get batch (pdht_get_resolve_dev; putget.c:50-59):
    replies uint8 [m, >= head + slot + elemsize] in bucket order, as
    DeviceTable.get wrote them and dist.exchange_replies brought them back;
    keys uint8 [n, L] packed, the caller's keys; slot = key_slot or L rounded
    up to 8.  With i = index[p] (int32 [m], e.g. record_fields(records, L)[3]
    read in place; None: i = p), status[i] = 2 NotFound / 3 Collision (the
    reply's key differs from keys[i]) / 0 OK, and values[i] receives the
    reply's value when 0.  Returns (values uint8 [n, elemsize], status uint8
    [n]); rows that no OK reply names keep their bytes (new tensors start as
    zeros, and status as 2).  values may be a row-strided view."""
    torch = _torch()
    m, RB, rstride = _rows_2d(replies, "replies")
    dev = replies.device
    n, L, kstride = _keys_2d(keys)
    if keys.device != dev or kstride != L:
        raise ValueError(f"keys must be packed and on {dev}")
    if head not in (1, 8):
        raise ValueError("head must be 1 or 8")
    if elemsize < 1:
        raise ValueError("elemsize must be >= 1")
    if key_slot and (key_slot % 8 or key_slot < L):
        raise ValueError(f"key_slot {key_slot} must be 0 or a multiple of 8 that is >= keysize {L}")
    slot = key_slot if key_slot else (L + 7) // 8 * 8
    if RB < head + slot + elemsize:
        raise ValueError(f"replies must have >= {head + slot + elemsize} bytes per row, got {RB}")
    if index is not None:
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or index.dim() != 1 or \
                not index.is_cuda or index.device != dev or index.numel() != m:
            raise ValueError(f"index must be a 1-D int32 tensor of {m} entries on {dev}")
        istride = 4 * index.stride(0) if m > 1 else 4
        if istride < 4:
            raise ValueError("index must have a positive stride")
    else:
        istride = 4
        if m > n:
            raise ValueError(f"{m} replies for {n} keys")
    if values is None:
        values = torch.zeros((n, elemsize), dtype=torch.uint8, device=dev)
    vn, vE, vstride = _rows_2d(values, "values", dev)
    if (vn, vE) != (n, elemsize):
        raise ValueError(f"values must have shape [{n}, {elemsize}], got {tuple(values.shape)}")
    if status is None:
        status = torch.full((n,), 2, dtype=torch.uint8, device=dev)
    _need(status, "status", torch.uint8, dev, shape=(n,))
    with _on(dev, stream) as g:
        _check(lib().pdht_get_resolve_dev(_dptr(replies), rstride, head, slot, _dptr(keys), L, _opt(index), istride,
                                          m, _dptr(values), elemsize, vstride, _dptr(status), g.stream),
               "pdht_get_resolve_dev")
    return values, status


def splitmix64_fill(seed: int, first: int, nwords: int, out=None, device="cuda", stream=None):
    torch = _torch()
    if out is None:
        out = torch.empty(nwords, dtype=torch.int64, device=device)
    else:
        _need(out, "out", torch.int64, out.device, numel=nwords)
    with _on(out.device, stream) as g:
        _check(lib().pdht_hip_splitmix64_fill_dev(seed, first, nwords, _dptr(out), g.stream),
               "pdht_hip_splitmix64_fill_dev")
    return out


def read_stream(buf, nt: bool = False, out=None, stream=None):
    """HBM read-bandwidth calibration: XOR-fold of a CUDA buffer (16-B multiple)."""
    torch = _torch()
    if not buf.is_contiguous():
        raise ValueError("buf must be contiguous")
    if out is None:
        out = torch.zeros(1, dtype=torch.int64, device=buf.device)
    _need(out, "out", torch.int64, buf.device, numel=1)
    with _on(buf.device, stream) as g:
        _check(lib().pdht_hip_read_stream_dev(_dptr(buf), buf.numel() * buf.element_size(), int(nt),
                                              _dptr(out), g.stream), "pdht_hip_read_stream_dev")
    return out


def key_stream(keys, out=None, stream=None):
    """Calibration: the 64-B kernel's data movement with an XOR fold for a hash."""
    torch = _torch()
    n = keys.shape[0]
    if keys.dim() != 2 or keys.shape[1] != 64 or keys.dtype != torch.uint8 or not keys.is_contiguous():
        raise PdhtError("key_stream takes a contiguous (n, 64) uint8 tensor")
    out = _out(n, 1, keys.device, out)
    with _on(keys.device, stream) as g:
        _check(lib().pdht_hip_key_stream_dev(_dptr(keys), n, _dptr(out), g.stream), "pdht_hip_key_stream_dev")
    return out


def mod_batch(values, divisor: int, out=None, stream=None):
    """Calibration: values int64 [n] (bit patterns of u64, CUDA) -> int32 [n]
    (bit patterns of u32), values[i] % divisor through the FastMod object of
    the placement and bucketing kernels (pdht_hip_mod_dev).  divisor: 1 ..
    2^32 - 1."""
    torch = _torch()
    if not isinstance(values, torch.Tensor) or values.dim() != 1 or not values.is_cuda:
        raise ValueError("values must be a 1-D CUDA int64 tensor")
    dev = values.device
    _need(values, "values", torch.int64, dev)
    if not 1 <= divisor <= 0xFFFFFFFF:
        raise ValueError(f"divisor {divisor} must be in 1 .. 2^32 - 1")
    n = values.numel()
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=dev)
    else:
        _need(out, "out", torch.int32, dev, shape=(n,))
    with _on(dev, stream) as g:
        _check(lib().pdht_hip_mod_dev(_dptr(values), n, divisor, _dptr(out), g.stream), "pdht_hip_mod_dev")
    return out


def xpose64_plan(n: int, cus: int = None, rounds_per_wg: int = -1, hist: bool = False) -> Xpose64Plan:
    """Launch plan of the default 64-B kernel over n packed keys (pdht_hip.h,
    pdht_hip_xpose64_plan_for; host arithmetic only).  cus = None: the CUs of
    the current GPU; rounds_per_wg = -1: the library's own choice, 0: the
    persistent shape; hist: a call that accumulates a histogram."""
    if cus is None:
        torch = _torch()
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    p = Xpose64Plan()
    _check(lib().pdht_hip_xpose64_plan_for(n, cus, rounds_per_wg, int(hist), C.byref(p)), "pdht_hip_xpose64_plan_for")
    return p


def xpose64_tiles(plan: Xpose64Plan, block0: int = 0, nblocks: int = None) -> np.ndarray:
    """Tile numbers of workgroups [block0, block0 + nblocks) of the plan's
    (first) launch as a (nblocks, rounds, 2, 4) uint64 array indexed [workgroup,
    its r-th round, d, wave], from the function the kernel indexes with."""
    nblocks = plan.grid - block0 if nblocks is None else nblocks
    rw = plan.rounds_per_wg if plan.round_blocked else plan.rounds
    t = np.empty((nblocks, rw, 2, 4), dtype=np.uint64)
    _check(lib().pdht_hip_xpose64_tiles(C.byref(plan), block0, nblocks, t.ctypes.data_as(C.c_void_p)),
           "pdht_hip_xpose64_tiles")
    return t


def key_stream_var(data, offsets, out=None, stream=None, check=True):
    """Calibration: the variable-length kernel's data movement with an XOR fold."""
    n, nb = _check_var(data, offsets, check, stream)
    out = _out(n, 1, data.device, out)
    with _on(data.device, stream) as g:
        _check(lib().pdht_hip_key_stream_var_dev(_dptr(data), nb, _dptr(offsets), n, _dptr(out), g.stream),
               "pdht_hip_key_stream_var_dev")
    return out


def mixed_lengths(seed: int, first: int, n: int, lo: int, hi: int, device="cuda", stream=None):
    torch = _torch()
    out = torch.empty(n, dtype=torch.int64, device=device)
    with _on(out.device, stream) as g:
        _check(lib().pdht_hip_mixed_lengths_dev(seed, first, n, lo, hi, _dptr(out), g.stream),
               "pdht_hip_mixed_lengths_dev")
    return out


# ------------------------------------------------------- host batch API ---
# Host buffers: numpy arrays or CPU torch tensors (pinned ones take the
# zero-copy path).  Everything is checked before C sees it: dtype,
# C-contiguity and size, so a strided view or a short `out` raises instead
# of producing wrong digests or writing past a host buffer.
def _host_arr(a, name, dtype, shape=None, numel=None):
    """numpy array or CPU torch tensor of `dtype` (numpy dtype), C-contiguous."""
    if isinstance(a, np.ndarray):
        if a.dtype != dtype:
            raise ValueError(f"{name} must be {np.dtype(dtype)}, got {a.dtype}")
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError(f"{name} must be C-contiguous")
        shp, size = a.shape, a.size
    else:
        torch = _torch()
        if not isinstance(a, torch.Tensor) or a.is_cuda:
            raise ValueError(f"{name} must be a numpy array or a CPU torch tensor")
        tdt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint64): torch.int64,
               np.dtype(np.uint32): torch.int32}[np.dtype(dtype)]
        if a.dtype not in (tdt, {torch.int64: torch.uint64, torch.int32: torch.uint32}.get(tdt, tdt)):
            raise ValueError(f"{name} must be {tdt}, got {a.dtype}")
        if not a.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        shp, size = tuple(a.shape), a.numel()
    if shape is not None and tuple(shp) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(shp)}")
    if numel is not None and size < numel:
        raise ValueError(f"{name} must hold >= {numel} elements, got {size}")
    return a


def _host_keys(keys):
    """Host keys [n, L] uint8, C-contiguous (packed rows)."""
    _host_arr(keys, "keys", np.uint8)
    if len(keys.shape) != 2:
        raise ValueError("keys must be 2-D [n, keylen]")
    return tuple(keys.shape)


def _np_keys(keys: np.ndarray):
    if keys.dtype != np.uint8 or keys.ndim != 2 or not keys.flags["C_CONTIGUOUS"]:
        raise ValueError("keys must be a C-contiguous uint8 array [n, keylen]")
    return keys.shape


def _host_ptr(a):
    """numpy array or (pinned) CPU torch tensor -> address."""
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    return C.c_void_p(a.data_ptr())


def city64_batch_host(keys, out=None, device: int = 0):
    """Host-resident keys (numpy uint8 [n, L] or pinned CPU tensor) -> uint64 [n]."""
    n, L = _host_keys(keys)
    if out is None:
        out = np.empty(n, dtype=np.uint64)
    _host_arr(out, "out", np.uint64, numel=n)
    _check(lib().pdht_city64_batch_host(_host_ptr(keys), L, n, _host_ptr(out), device),
           "pdht_city64_batch_host")
    return out


def city64_var_batch_host(data, offsets, out=None, device: int = 0):
    """Host-resident variable-length keys: data uint8 [nbytes], offsets [n+1]
    (uint64, or int64 with no negative entry -- numpy arrays and CPU tensors
    alike, viewed as uint64 without a copy so pinned buffers stay pinned)."""
    _host_arr(data, "data", np.uint8)
    if isinstance(offsets, np.ndarray) and offsets.dtype == np.int64:
        if offsets.size and int(offsets.min()) < 0:
            raise ValueError("offsets must not be negative")
        offsets = offsets.view(np.uint64)
    elif not isinstance(offsets, np.ndarray) and str(getattr(offsets, "dtype", "")) == "torch.int64":
        if offsets.numel() and int(offsets.min()) < 0:
            raise ValueError("offsets must not be negative")
    offsets = _host_arr(offsets, "offsets", np.uint64)
    n = offsets.size - 1 if isinstance(offsets, np.ndarray) else offsets.numel() - 1
    if n < 0:
        raise ValueError("offsets must hold n+1 entries")
    if n:
        last = int(offsets[-1])
        nbytes = data.nbytes if isinstance(data, np.ndarray) else data.numel()
        if last > nbytes or int(offsets[0]) > last:
            raise ValueError(f"offsets reach byte {last}, data holds {nbytes}")
    if out is None:
        out = np.empty(n, dtype=np.uint64)
    _host_arr(out, "out", np.uint64, numel=n)
    _check(lib().pdht_city64_batch_var_host(_host_ptr(data), _host_ptr(offsets), n, _host_ptr(out), device),
           "pdht_city64_batch_var_host")
    return out


def citycrc128_batch_host(keys, out=None, device: int = 0):
    n, L = _host_keys(keys)
    if out is None:
        out = np.empty((n, 2), dtype=np.uint64)
    _host_arr(out, "out", np.uint64, numel=2 * n)
    _check(lib().pdht_citycrc128_batch_host(_host_ptr(keys), L, n, _host_ptr(out), device),
           "pdht_citycrc128_batch_host")
    return out


def place_batch_host(keys, nptes: int, nranks: int, device: int = 0, out=None):
    """Host-resident fused placement; `out` = (mbits uint64[n], ptindex
    uint32[n], rank uint32[n]) host arrays to fill (pinned ones, with pinned
    keys, take the zero-copy path)."""
    n, L = _host_keys(keys)
    if out is not None:
        mb, pt, rk = out
    else:
        mb = np.empty(n, dtype=np.uint64)
        pt = np.empty(n, dtype=np.uint32)
        rk = np.empty(n, dtype=np.uint32)
    _host_arr(mb, "mbits", np.uint64, numel=n)
    _host_arr(pt, "ptindex", np.uint32, numel=n)
    _host_arr(rk, "rank", np.uint32, numel=n)
    _check(lib().pdht_place_batch_host(_host_ptr(keys), L, n, nptes, nranks, _host_ptr(mb),
                                       _host_ptr(pt), _host_ptr(rk), 4, device),
           "pdht_place_batch_host")
    return mb, pt, rk


# ------------------------------------------------------- pdht_t mirror ---
class PdhtTable:
    """The hash-path view of a pdht table (pdht_create's keysize/nptes,
    init.c:80-94) over the stand-in pdht_t of include/pdht_hash.h.

    hash(key)            -> (mbits, ptindex, rank)       pdht_hash, hash.c:25-30
    sethash(fn)          -> install a plugin              pdht_sethash, hash.c:39-41
    hash_batch(keys)     -> arrays                        pdht_hash_batch (GPU or plugin)
    """

    def __init__(self, keysize: int, nptes: int = 1, nranks: int = 1):
        self._t = _PdhtT()
        lib().pdht_hip_table_init(C.byref(self._t), keysize, nptes)
        self.nranks = nranks
        self._plugin = None

    @property
    def keysize(self) -> int:
        return self._t.keysize

    @property
    def nptes(self) -> int:
        return self._t.nptes

    def _set_ranks(self):
        C.c_int.in_dll(lib(), "pdht_hip_shim_nranks").value = self.nranks

    def sethash(self, fn):
        """fn(table, key_bytes) -> (mbits, ptindex, rank) or a raw C function pointer."""
        if fn is None:
            lib().pdht_sethash(C.byref(self._t), C.cast(lib().pdht_hash, C.c_void_p))
            self._plugin = None
            return
        L = self.keysize

        def tramp(dht, key, mb, pt, rk):
            m, p, r = fn(self, C.string_at(key, L))
            mb[0] = m & 0xFFFFFFFFFFFFFFFF
            pt[0] = p & 0xFFFFFFFF
            rk[0].rank = r & 0xFFFFFFFF

        self._plugin = _HASHFUNC(tramp)
        lib().pdht_sethash(C.byref(self._t), C.cast(self._plugin, C.c_void_p))

    def hash(self, key: bytes):
        if len(key) < self.keysize:
            raise ValueError("key shorter than keysize")
        self._set_ranks()
        mb, pt, rk = C.c_uint64(), C.c_uint32(), PtlProcess()
        # dht->hashfn(dht, key, &mbits, &ptindex, &rank), as putget.c:53 calls it
        fn = _HASHFUNC(self._t.hashfn)
        fn(C.cast(C.byref(self._t), C.c_void_p), C.c_char_p(bytes(key)), C.byref(mb), C.byref(pt),
           C.byref(rk))
        return mb.value, pt.value, rk.rank

    def hash_batch(self, keys: np.ndarray, device: int = 0):
        """keys uint8 [n, keysize] (host) -> (mbits u64[n], ptindex u32[n], rank u32[n])."""
        n, L = _np_keys(keys)
        if L != self.keysize:
            raise ValueError("key width != keysize")
        self._set_ranks()
        mb = np.empty(n, dtype=np.uint64)
        pt = np.empty(n, dtype=np.uint32)
        rk = (PtlProcess * max(n, 1))()
        _check(lib().pdht_hash_batch(C.byref(self._t), _host_ptr(keys), n, _host_ptr(mb),
                                     _host_ptr(pt), C.cast(rk, C.c_void_p), device),
               "pdht_hash_batch")
        ranks = np.frombuffer(rk, dtype=np.uint32).reshape(-1, 2)[:n, 0].copy()
        return mb, pt, ranks
