// pdht_table_keys.hip -- put and get by key on the device-resident target table
// (include/pdht_hip_table_keys.h; kernels in table_keys.h): argument checks, launchers and the C ABI.
// Every check runs before any device call.
#include "table_keys.h"
#include "table_host.h"

namespace pdht {

static thread_local char g_keys_name[96];

// The geometry that both calls share: -> slot, or a refusal.  op = "put_keys" or "get_keys".
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

// key_digest's class: keys of 8 bytes on an 8-byte boundary, of 16 / 32 / 64 bytes on a 16-byte one
static u32 keys_class(const void *keys, size_t keysize) {
  if (keysize == 8) return ((uintptr_t)keys & 7) == 0 ? 8 : 0;
  if (keysize == 16 || keysize == 32 || keysize == 64) return ((uintptr_t)keys & 15) == 0 ? (u32)keysize : 0;
  return 0;
}

template <int L>
static void launch_claim_keys(const KeysClaimArgs &c, int dev, hipStream_t st) {
  k_table_claim_keys<L><<<table_grid(c.m, 64, dev), kBlock, 0, st>>>(c);
}

// aligned: keys, keysize, values, value_stride and elemsize are all multiples of 8
template <int P>
static void launch_write_keys(const KeysWriteArgs &w, bool aligned, int dev, hipStream_t st) {
  const unsigned grid = table_grid(w.m, (u64)(64u >> w.gshift) * kRowsInFlight, dev);
  const bool nt = hook_table_put_nt(kTablePutNt);
  if (aligned)
    nt ? k_table_write_keys<P, true, true><<<grid, kBlock, 0, st>>>(w)
       : k_table_write_keys<P, false, true><<<grid, kBlock, 0, st>>>(w);
  else
    nt ? k_table_write_keys<P, true, false><<<grid, kBlock, 0, st>>>(w)
       : k_table_write_keys<P, false, false><<<grid, kBlock, 0, st>>>(w);
}

static int table_put_keys(void *table, u64 capacity, size_t rowbytes, const void *keys, size_t keysize,
                          size_t key_slot, const void *values, size_t elemsize, size_t value_stride, size_t m,
                          void *workspace, size_t workspace_bytes, u64 *mbits_out, uint8_t *status, hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  size_t slot;
  if (int rc = keys_check("put_keys", rowbytes, keysize, key_slot, elemsize, value_stride, m, &slot)) return rc;
  if ((uintptr_t)workspace & 3) return fail("table put_keys: workspace must be 4-byte aligned%s", "");
  if (workspace_bytes < 4 * m)
    return fail("table put_keys: workspace too small (%s%lld bytes needed)", "", (long long)(4 * m));
  if ((uintptr_t)mbits_out & 7) return fail("table put_keys: mbits_out must be 8-byte aligned%s", "");
  if (m && !keys) return fail("table put_keys: keys must not be NULL%s", "");
  if (m && !values) return fail("table put_keys: values must not be NULL%s", "");
  if (m && !workspace) return fail("table put_keys: workspace must not be NULL%s", "");
  const bool p16 = (rowbytes & 15) == 0;
  snprintf(g_keys_name, sizeof g_keys_name, "k_table_claim_keys+k_table_write_keys<%d>", p16 ? 16 : 8);
  g_kernel = g_keys_name;
  if (m == 0) return 0;
  int dev;
  if (int rc = current_device(&dev)) return rc;
  KeysClaimArgs c{};
  c.t = make_geom(table, capacity, rowbytes);
  c.keys = static_cast<const uint8_t *>(keys);
  c.keysize = (u32)keysize;
  c.m = m;
  c.slots = static_cast<u32 *>(workspace);
  c.mbits_out = mbits_out;
  switch (keys_class(keys, keysize)) {
    case 8: launch_claim_keys<8>(c, dev, st); break;
    case 16: launch_claim_keys<16>(c, dev, st); break;
    case 32: launch_claim_keys<32>(c, dev, st); break;
    case 64: launch_claim_keys<64>(c, dev, st); break;
    default: launch_claim_keys<0>(c, dev, st); break;
  }
  HIP_TRY(hipGetLastError());
  KeysWriteArgs w{};
  w.t = c.t;
  w.s.keys = c.keys;
  w.s.values = static_cast<const uint8_t *>(values);
  w.s.value_stride = value_stride;
  w.s.keysize = (u32)keysize;
  w.s.slot = (u32)slot;
  w.s.elemsize = (u32)elemsize;
  const bool aligned = (((uintptr_t)keys | keysize | (uintptr_t)values | value_stride | elemsize) & 7) == 0;
  w.m = m;
  w.slots = c.slots;
  w.status = status;
  w.np = (u32)(rowbytes / (p16 ? 16 : 8));
  w.gshift = group_shift(w.np);
  p16 ? launch_write_keys<16>(w, aligned, dev, st) : launch_write_keys<8>(w, aligned, dev, st);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int table_get_keys(const void *table, u64 capacity, size_t rowbytes, const void *keys, size_t keysize,
                          size_t key_slot, size_t m, void *values, size_t elemsize, size_t value_stride,
                          u64 *mbits_out, uint8_t *status, hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  size_t slot;
  if (int rc = keys_check("get_keys", rowbytes, keysize, key_slot, elemsize, value_stride, m, &slot)) return rc;
  if ((uintptr_t)mbits_out & 7) return fail("table get_keys: mbits_out must be 8-byte aligned%s", "");
  if (m && !keys) return fail("table get_keys: keys must not be NULL%s", "");
  if (m && !values) return fail("table get_keys: values must not be NULL%s", "");
  if (m && !status) return fail("table get_keys: status must not be NULL%s", "");
  const uintptr_t bits = rowbytes | slot | (uintptr_t)values | value_stride | elemsize;
  const int piece = (bits & 15) == 0 ? 16 : (bits & 7) == 0 ? 8 : (bits & 3) == 0 ? 4 : 1;
  g_kernel = piece == 16 ? "k_table_get_keys<16>" : piece == 8 ? "k_table_get_keys<8>" : piece == 4 ? "k_table_get_keys<4>"
                                                                                                    : "k_table_get_keys<1>";
  if (m == 0) return 0;
  int dev;
  if (int rc = current_device(&dev)) return rc;
  KeysGetArgs a{};
  a.t = make_geom(table, capacity, rowbytes);
  a.keys = static_cast<const uint8_t *>(keys);
  a.keysize = (u32)keysize;
  a.lclass = keys_class(keys, keysize);
  a.slot = (u32)slot;
  a.m = m;
  a.values = static_cast<uint8_t *>(values);
  a.value_stride = value_stride;
  a.mbits_out = mbits_out;
  a.status = status;
  a.np = (u32)(elemsize / piece);
  // lanes for the value pieces, and for the key at 4 bytes a lane (the resolve's rule)
  a.gshift = group_shift(std::max<u32>(a.np, (u32)((keysize + 3) / 4)));
  const unsigned grid = table_grid(m, 64u >> a.gshift, dev);
  if (piece == 16)
    k_table_get_keys<16><<<grid, kBlock, 0, st>>>(a);
  else if (piece == 8)
    k_table_get_keys<8><<<grid, kBlock, 0, st>>>(a);
  else if (piece == 4)
    k_table_get_keys<4><<<grid, kBlock, 0, st>>>(a);
  else
    k_table_get_keys<1><<<grid, kBlock, 0, st>>>(a);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace pdht

using namespace pdht;

PDHT_API size_t pdht_table_put_keys_workspace_bytes(size_t m) { return 4 * m; }

PDHT_API int pdht_table_put_keys_dev(void *table, uint64_t capacity, size_t rowbytes, const void *keys, size_t keysize,
                                     size_t key_slot, const void *values, size_t elemsize, size_t value_stride, size_t m,
                                     void *workspace, size_t workspace_bytes, uint64_t *mbits_out, uint8_t *status,
                                     pdht_hip_stream_t s) {
  return table_put_keys(table, capacity, rowbytes, keys, keysize, key_slot, values, elemsize, value_stride, m, workspace,
                        workspace_bytes, mbits_out, status, ST(s));
}

PDHT_API int pdht_table_get_keys_dev(const void *table, uint64_t capacity, size_t rowbytes, const void *keys,
                                     size_t keysize, size_t key_slot, size_t m, void *values, size_t elemsize,
                                     size_t value_stride, uint64_t *mbits_out, uint8_t *status, pdht_hip_stream_t s) {
  return table_get_keys(table, capacity, rowbytes, keys, keysize, key_slot, m, values, elemsize, value_stride, mbits_out,
                        status, ST(s));
}
