"""The line forms of city_core.h against its plain form, without a GPU.

The long-key kernels read through GlobalReaderT with kPairs / kLines (or
kStream) set: 128-B spans in the CityHash64 and CityHash128WithSeed loops,
CityHashCrc256Long's blocks as whole 128-B lines with a carried remainder or
as a line stream.  tests/city_lines_check.cpp (its own main, city_core.h the
only project header) runs those forms on the host over a bounds-checking
reader and compares them with HostReader, which test_scalar_vs_oracle_random
and the golden vectors pin to the oracle, at every length 0..6000; four fixed
lengths are also compared with oracle digests passed on the command line.

Built for the host by hipcc as a child process, under AddressSanitizer and
UBSan where they link (the test's output says which); nothing here touches
the GPU or code loaded into Python.  Removing crc256_long's
`line_end(k) <= len` guard makes the program fail (a read past the key).
"""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pdht_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "city_lines_check.cpp")
# -O0: the sanitized build of these always-inlined templates takes 12 s, 60 s at -O1 (the run 3 s against 0.7 s)
HIPCC = ["--offload-arch=gfx950", "-std=c++17", "-O0", "-g", "-x", "hip"]
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]

ORACLE_LENGTHS = (901, 1920, 2688, 3200)
# per length 0..6000: six digests on the kLines + kPairs reader, the two CRC ones on the kStream reader;
# per oracle length: plain, lines and stream
N_CHECKS = 6001 * 8 + len(ORACLE_LENGTHS) * 3


def key_bytes(n):
    """city_lines_check.cpp's key of length n."""
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (i + np.uint64(1 + n * 1000003)) * np.uint64(0x9E3779B97F4A7C15)
    return (x >> np.uint64(56)).astype(np.uint8)


def _hipcc():
    for c in (os.environ.get("HIPCC"), "hipcc", "/opt/rocm/bin/hipcc"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_line_forms_match_plain_form_at_every_length(tmp_path, oracle):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = SAN
    p = subprocess.run([hipcc] + HIPCC + san + ["-o", str(tmp_path / "probe"), str(probe)],
                       capture_output=True, text=True)
    if p.returncode != 0:
        san = []  # the reader's own bounds checks still end the program at a read past the key
        p = subprocess.run([hipcc] + HIPCC + ["-o", str(tmp_path / "probe"), str(probe)],
                           capture_output=True, text=True)
        if p.returncode != 0:
            pytest.skip(f"hipcc cannot build a host program: {p.stderr.strip().splitlines()[-1:]}")
    exe = tmp_path / "city_lines_check"
    t0 = time.perf_counter()
    p = subprocess.run([hipcc] + HIPCC + san + ["-Wall", "-I", CSRC, "-o", str(exe), SRC],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    t1 = time.perf_counter()
    args = []
    for n in ORACLE_LENGTHS:
        lo, hi = (int(x) for x in oracle.city128_fixed(key_bytes(n).reshape(1, n), crc=True)[0])
        args.append(f"{n}:{lo:x}:{hi:x}")
    # leak checking needs ptrace rights a test runner may lack
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, env=env, timeout=300)
    t2 = time.perf_counter()
    print(f"sanitizers {'on (address, undefined)' if san else 'OFF (they do not link here)'}; "
          f"build {t1 - t0:.1f} s, run {t2 - t1:.2f} s; {r.stdout.strip().splitlines()[-1:]}")
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines()[-1] == f"OK {N_CHECKS}", r.stdout[-500:]
