// table_keys_host.h -- the host side that the keyed operations of the device-resident target table share
// (pdht_table_keys.hip: put and get by key; pdht_table_keys_rmw.hip: update, insert-if-absent and
// compare-and-swap by key): the geometry of keys and values against a row, the class of a keys batch for
// key_digest, the checks of the buffers, and the launcher of k_table_write_keys.
#pragma once
#include "table_keys.h"
#include "table_host.h"

namespace pdht {

// The geometry that the calls with values share: -> slot, or a refusal.  op = the call's name, "put_keys" ...
static int keys_check(const char *op, size_t rowbytes, size_t keysize, size_t key_slot, size_t elemsize,
                      size_t value_stride, size_t m, size_t *slot) {
  if (m >= (1ull << 32)) return fail("table %s: m must be < 2^32 per call", op);
  if (keysize == 0) return fail("table %s: keysize must be >= 1", op);
  if (keysize > 64)
    return fail("table %s: keysize must be <= 64; longer keys go through pdht_bucket_put_records_dev and "
                "pdht_table_put_records_dev (get: pdht_bucket_records_dev, pdht_table_get_dev, pdht_get_resolve_dev)",
                op);
  if (key_slot && ((key_slot & 7) || key_slot < keysize))
    return fail("table %s: key_slot must be 0 or a multiple of 8 that is >= keysize", op);
  if (elemsize == 0) return fail("table %s: elemsize must be >= 1", op);
  *slot = key_slot ? key_slot : (keysize + 7) & ~(size_t)7;
  if (elemsize >= (1ull << 31) || rowbytes != ((*slot + elemsize + 7) & ~(size_t)7))
    return fail("table %s: rowbytes must be slot + elemsize rounded up to 8 (pdht_bucket_put_record_bytes - 24)", op);
  if (value_stride < elemsize) return fail("table %s: value_stride must be >= elemsize", op);
  return 0;
}

// The buffers of a keyed call that writes the table, behind its geometry.  need: the workspace bytes of this
// call.  has_values: the call reads values (a compare-and-swap does not, and checks its replies itself).
static int keys_buffers_check(const char *op, const void *keys, const void *values, bool has_values, size_t m,
                              const void *workspace, size_t workspace_bytes, size_t need, const void *mbits_out) {
  if ((uintptr_t)workspace & 3) return fail("table %s: workspace must be 4-byte aligned", op);
  if (workspace_bytes < need) return fail("table %s: workspace too small (%lld bytes needed)", op, (long long)need);
  if ((uintptr_t)mbits_out & 7) return fail("table %s: mbits_out must be 8-byte aligned", op);
  if (m && !keys) return fail("table %s: keys must not be NULL", op);
  if (has_values && m && !values) return fail("table %s: values must not be NULL", op);
  if (m && !workspace) return fail("table %s: workspace must not be NULL", op);
  return 0;
}

// key_digest's class: keys of 8 bytes on an 8-byte boundary, of 16 / 32 / 64 bytes on a 16-byte one
static u32 keys_class(const void *keys, size_t keysize) {
  if (keysize == 8) return ((uintptr_t)keys & 7) == 0 ? 8 : 0;
  if (keysize == 16 || keysize == 32 || keysize == 64) return ((uintptr_t)keys & 15) == 0 ? (u32)keysize : 0;
  return 0;
}

// f(std::integral_constant<int, L>) for the class L of a keys batch: the launches of the kernels built per L
template <typename F>
static void by_keys_class(const void *keys, size_t keysize, F f) {
  switch (keys_class(keys, keysize)) {
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    case 64: f(std::integral_constant<int, 64>{}); break;
    default: f(std::integral_constant<int, 0>{}); break;
  }
}

static RowSource row_source(const void *keys, size_t keysize, size_t slot, const void *values, size_t elemsize,
                            size_t value_stride) {
  RowSource s{};
  s.keys = static_cast<const uint8_t *>(keys);
  s.values = static_cast<const uint8_t *>(values);
  s.value_stride = value_stride;
  s.keysize = (u32)keysize;
  s.slot = (u32)slot;
  s.elemsize = (u32)elemsize;
  return s;
}

// whole-word loads: keys, keysize, values, value_stride and elemsize are all multiples of 8
static bool row_source_aligned(const RowSource &s) {
  return (((uintptr_t)s.keys | s.keysize | (uintptr_t)s.values | s.value_stride | s.elemsize) & 7) == 0;
}

template <int P>
static void launch_write_keys_p(const KeysWriteArgs &w, unsigned grid, hipStream_t st) {
  const bool nt = hook_table_put_nt(kTablePutNt);
  if (row_source_aligned(w.s))
    nt ? k_table_write_keys<P, true, true><<<grid, kBlock, 0, st>>>(w)
       : k_table_write_keys<P, false, true><<<grid, kBlock, 0, st>>>(w);
  else
    nt ? k_table_write_keys<P, true, false><<<grid, kBlock, 0, st>>>(w)
       : k_table_write_keys<P, false, false><<<grid, kBlock, 0, st>>>(w);
}

// k_table_write_keys of a put_keys (absent 2) or an update_keys (absent 3) behind the kernel that left slots
// and winner words: w.t, w.s, w.m, w.slots and w.status are the caller's.  Row pieces of 16 bytes when
// rowbytes allows them (the table's rows are the only vector accesses with an alignment of their own).
static void launch_write_keys(KeysWriteArgs w, u32 absent, int dev, hipStream_t st) {
  const bool p16 = (w.t.rowbytes & 15) == 0;
  w.np = (u32)(w.t.rowbytes / (p16 ? 16 : 8));
  w.gshift = group_shift(w.np);
  w.absent = absent;
  const unsigned grid = table_grid(w.m, (u64)(64u >> w.gshift) * kRowsInFlight, dev);
  p16 ? launch_write_keys_p<16>(w, grid, st) : launch_write_keys_p<8>(w, grid, st);
}

}  // namespace pdht
