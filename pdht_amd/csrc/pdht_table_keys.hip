// pdht_table_keys.hip -- put and get by key on the device-resident target table
// (include/pdht_hip_table_keys.h; kernels in table_keys.h): argument checks, launchers and the C ABI.
// Every check runs before any device call.
#include "table_keys_host.h"

namespace pdht {

static thread_local char g_keys_name[96];

static int table_put_keys(void *table, u64 capacity, size_t rowbytes, const void *keys, size_t keysize,
                          size_t key_slot, const void *values, size_t elemsize, size_t value_stride, size_t m,
                          void *workspace, size_t workspace_bytes, u64 *mbits_out, uint8_t *status, hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  size_t slot;
  if (int rc = keys_check("put_keys", rowbytes, keysize, key_slot, elemsize, value_stride, m, &slot)) return rc;
  if (int rc = keys_buffers_check("put_keys", keys, values, true, m, workspace, workspace_bytes, 4 * m, mbits_out))
    return rc;
  snprintf(g_keys_name, sizeof g_keys_name, "k_table_claim_keys+k_table_write_keys<%d>", (rowbytes & 15) == 0 ? 16 : 8);
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
  const unsigned grid = table_grid(m, 64, dev);
  by_keys_class(keys, keysize, [&](auto L) { k_table_claim_keys<decltype(L)::value><<<grid, kBlock, 0, st>>>(c); });
  HIP_TRY(hipGetLastError());
  KeysWriteArgs w{};
  w.t = c.t;
  w.s = row_source(keys, keysize, slot, values, elemsize, value_stride);
  w.m = m;
  w.slots = c.slots;
  w.status = status;
  launch_write_keys(w, 2, dev, st);
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
