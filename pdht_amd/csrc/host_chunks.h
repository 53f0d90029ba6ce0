// host_chunks.h -- chunk planning of the host-resident variable-length batch
// (pdht_host.hip), as a pure function: no HIP in here, so that a plain C++
// program can include it (tests/test_host_chunks_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace pdht {

// Cuts keys [0, n) of an offset-indexed batch (key i = bytes [offsets[i],
// offsets[i+1]), offsets non-decreasing, n+1 entries) greedily into chunks
// [a, b): from a, the most keys with b - a <= max_keys and offsets[b] -
// offsets[a] <= chunk_bytes, and never fewer than one (a key longer than
// chunk_bytes gets a chunk of its own).  Appends the chunks to `out`.
static inline void host_var_chunks(const uint64_t *offsets, size_t n, uint64_t chunk_bytes, size_t max_keys,
                                   std::vector<std::pair<size_t, size_t>> &out) {
  size_t next = 0;
  while (next < n) {
    const size_t a = next;
    const uint64_t lim = offsets[a] + chunk_bytes;
    const size_t hi = std::min(n, a + max_keys);
    // largest b <= hi with offsets[b] <= lim (binary search; offsets sorted)
    size_t lo_b = a + 1, hi_b = hi;
    while (lo_b < hi_b) {
      size_t mid = (lo_b + hi_b + 1) / 2;
      if (offsets[mid] <= lim) lo_b = mid; else hi_b = mid - 1;
    }
    const size_t b = std::max(a + 1, lo_b);
    out.push_back({a, b});
    next = b;
  }
}

}  // namespace pdht
