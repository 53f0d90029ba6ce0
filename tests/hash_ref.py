"""What the hash launch paths choose, restated for the tests that assert
pdht_hip_last_kernel (pdht_amd/csrc/launch.h), and the window kernel's
LDS / global split."""
import numpy as np


def fixed_kernel(L, stride=None, aligned=True, crc=False):
    """launch_fixed's choice for a generic length: the LDS window that holds a
    64-key tile (12 KiB or 16 KiB), else per-lane global reads (16-B loads
    when every key starts 16-B aligned; 2 WG/CU, 8 with the LDS CRC tables)."""
    tile = 63 * (stride or L) + L + 16
    if tile > 16384:
        a16 = aligned and (stride or L) % 16 == 0
        return ("k_global<fixed,a16,lines>" if a16 else "k_global<fixed>") + ("@8" if crc and L > 900 else "@2")
    return "k_window<fixed,nt,16K>@2" if tile > 12288 else "k_window<fixed,nt,12K>@3"


VAR_WINDOW_KERNELS = {10224: "k_window<var,nt,10224>@4", 16384: "k_window<var,nt,16K>@2"}


def var_kernel(total_bytes, n):
    """launch_var's window choice: mean key length > 160 B -> 16 KiB."""
    return VAR_WINDOW_KERNELS[16384 if total_bytes // n > 160 else 10224]


def var_from_lds(offs, base, win):
    """k_window<var>'s rule, per key: True where the key is hashed out of the
    wave's LDS window, False where it is read from global memory.  `offs` are
    the n + 1 byte offsets, `base` the address of byte 0 (only base mod 16
    matters), `win` the window's bytes.  A tile is 64 consecutive keys; its
    window starts at the 16-B block of the tile's first byte and holds
    min(span, win) bytes; a key is in it when it ends inside."""
    offs = np.asarray(offs, dtype=np.int64)
    n = offs.size - 1
    k0 = np.arange(n) // 64 * 64
    first = offs[k0]
    whi = offs[np.minimum(k0 + 64, n)]
    wlo = (base + first) & ~np.int64(15)
    span = np.where(whi > first, base + whi - wlo, 0)
    return base + offs[1:] - wlo <= np.minimum(span, win)
