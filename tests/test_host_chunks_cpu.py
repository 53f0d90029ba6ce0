"""The host path's variable-length chunk planner, without a GPU.

pdht_amd/csrc/host_chunks.h holds the greedy planner of
pdht_city64_batch_var_host as a pure function.  A stand-alone C++ program
(its own main, only that header included) compares it with a brute-force
linear restatement on every small length vector and on seeded random ones,
asserts the planner's invariants directly, and runs under AddressSanitizer
and UBSan as a child process: an offsets[] read past n, which the binary
search's bounds could make, ends it.

Also here: the host entry points refuse a device index outside the table of
per-device pipelines before any device call.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pdht_amd as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pdht_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

PROGRAM = r"""
#include "host_chunks.h"

#include <cstdio>
#include <cstdlib>
#include <random>

typedef std::vector<std::pair<size_t, size_t>> Chunks;

// from a, keys while count < max_keys and offsets[b+1] - offsets[a] <= chunk_bytes, always at least one
static void brute(const uint64_t *off, size_t n, uint64_t cb, size_t mk, Chunks &out) {
  size_t a = 0;
  while (a < n) {
    size_t b = a + 1;
    while (b < n && b - a < mk && off[b + 1] - off[a] <= cb) ++b;
    out.push_back({a, b});
    a = b;
  }
}

static void dump(const char *why, const uint64_t *off, size_t n, uint64_t cb, size_t mk, const Chunks &got,
                 const Chunks &want) {
  printf("FAIL %s: chunk_bytes=%llu max_keys=%zu n=%zu offsets=[", why, (unsigned long long)cb, mk, n);
  for (size_t i = 0; i <= n; ++i) printf("%s%llu", i ? "," : "", (unsigned long long)off[i]);
  printf("] got=");
  for (auto &c : got) printf("[%zu,%zu)", c.first, c.second);
  printf(" want=");
  for (auto &c : want) printf("[%zu,%zu)", c.first, c.second);
  printf("\n");
  exit(1);
}

static Chunks g_got, g_want;
static size_t g_count = 0;

// off: a heap array of exactly n + 1 entries (a read of off[n + 1] is ASan's to report)
static void check(const uint64_t *off, size_t n, uint64_t cb, size_t mk) {
  Chunks &got = g_got, &want = g_want;
  got.clear();
  want.clear();
  pdht::host_var_chunks(off, n, cb, mk, got);
  brute(off, n, cb, mk, want);
  if (got != want) dump("differs from the linear restatement", off, n, cb, mk, got, want);
  // the invariants, directly
  size_t next = 0;
  for (auto &c : got) {
    const size_t a = c.first, b = c.second;
    if (a != next) dump("not a partition in order", off, n, cb, mk, got, want);
    if (b <= a || b > n) dump("empty chunk or past n", off, n, cb, mk, got, want);
    if (b - a > 1 && off[b] - off[a] > cb) dump("more than chunk_bytes in a chunk of several keys", off, n, cb, mk, got, want);
    if (b - a > mk) dump("more than max_keys keys", off, n, cb, mk, got, want);
    if (b < n && b - a < mk && off[b + 1] - off[a] <= cb) dump("not maximal", off, n, cb, mk, got, want);
    next = b;
  }
  if (next != n) dump("does not end at n", off, n, cb, mk, got, want);
  ++g_count;
}

int main() {
  // every length vector of up to 7 keys over these lengths
  static const uint64_t kLen[8] = {0, 1, 7, 8, 9, 16, 17, 40};
  static const size_t kMaxKeys[4] = {1, 2, 3, 100};
  static const uint64_t kFirst[2] = {0, 5};
  for (size_t n = 0; n <= 7; ++n) {
    uint64_t *off = new uint64_t[n + 1];
    size_t total = 1;
    for (size_t i = 0; i < n; ++i) total *= 8;
    for (size_t v = 0; v < total; ++v)
      for (uint64_t first : kFirst) {
        off[0] = first;
        size_t d = v;
        for (size_t i = 0; i < n; ++i, d /= 8) off[i + 1] = off[i] + kLen[d % 8];
        for (size_t mk : kMaxKeys) check(off, n, 16, mk);
      }
    delete[] off;
  }
  // seeded random vectors: lengths 0-50, now and then a 500-byte key
  std::mt19937_64 rng(0x5EED5EED5EED5EEDull);
  for (int it = 0; it < 20000; ++it) {
    const size_t n = rng() % 301;
    uint64_t *off = new uint64_t[n + 1];
    off[0] = rng() % 3 ? 0 : rng() % 1000;
    for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + (rng() % 37 == 0 ? 500 : rng() % 51);
    check(off, n, 64, 8);
    delete[] off;
  }
  printf("OK %zu\n", g_count);
  return 0;
}
"""

# inputs of the program above: sum_{n<=7} 8^n vectors x 2 first offsets x 4 max_keys, + 20 000 random
N_INPUTS = sum(8 ** n for n in range(8)) * 2 * 4 + 20000


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return c
    return None


def test_planner_matches_linear_restatement_under_sanitizers(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program itself where the compiler has them
    # as archives (gcc), so that it depends on nothing in the process's
    # library list; else the compiler's default
    for static in (["-static-libasan", "-static-libubsan"], []):
        p = subprocess.run([cxx] + SAN + static + ["-o", str(tmp_path / "probe"), str(probe)],
                           capture_output=True, text=True)
        if p.returncode == 0:
            break
    else:
        pytest.skip(f"{cxx} cannot link the sanitizer runtime: {p.stderr.strip().splitlines()[-1:]}")
    src = tmp_path / "host_chunks_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "host_chunks_check"
    p = subprocess.run([cxx] + SAN + static + ["-Wall", "-Wextra", "-I", CSRC, "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    # leak checking needs ptrace rights a test runner may lack; the planner allocates only in the caller's vector
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines()[-1] == f"OK {N_INPUTS}", r.stdout[-500:]


def test_pdht_host_uses_the_header():
    """The pipeline plans with the function the program above checks, at the
    limits the GPU tests restate (32 MiB, 2 Mi keys)."""
    src = open(os.path.join(CSRC, "pdht_host.hip")).read()
    assert '#include "host_chunks.h"' in src
    assert "host_var_chunks(offsets, n, kChunkBytes, max_keys, chunks)" in src
    assert "const size_t max_keys = kChunkBytes / 16;" in src and "kChunkBytes = 32u << 20" in src
    assert "while (lo_b < hi_b)" not in src  # one copy of the search


# ------------------------------------------------ device index, no GPU ---
def _no_gpu():
    if P.device_count() != 0:
        pytest.skip("a GPU is present (tests/test_gpu_host.py checks this there)")


@pytest.mark.parametrize("device", [64, -1])
def test_host_entry_points_refuse_device_out_of_range(device):
    """The device index is checked before any device call, whatever the
    pinning query answers on a machine without a GPU."""
    _no_gpu()
    keys = np.zeros((10, 64), dtype=np.uint8)
    with pytest.raises(P.PdhtError, match="out of range"):
        P.city64_batch_host(keys, device=device)
    with pytest.raises(P.PdhtError, match="out of range"):
        P.citycrc128_batch_host(keys, device=device)
    with pytest.raises(P.PdhtError, match="out of range"):
        P.place_batch_host(keys, 3, 10, device=device)
    data = np.zeros(100, dtype=np.uint8)
    offs = np.arange(0, 101, 10, dtype=np.uint64)
    with pytest.raises(P.PdhtError, match="out of range"):
        P.city64_var_batch_host(data, offs, device=device)
