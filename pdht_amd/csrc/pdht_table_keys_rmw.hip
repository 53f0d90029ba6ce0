// pdht_table_keys_rmw.hip -- update, insert-if-absent and compare-and-swap by key on the device-resident
// target table (include/pdht_hip_table_keys_rmw.h; kernels in table_keys_rmw.h): argument checks,
// launchers and the C ABI.  Every check runs before any device call.
#include "table_keys_rmw.h"
#include "table_keys_host.h"

namespace pdht {

static thread_local char g_keys_rmw_name[96];

static int table_update_keys(void *table, u64 capacity, size_t rowbytes, const void *keys, size_t keysize,
                             size_t key_slot, const void *values, size_t elemsize, size_t value_stride, size_t m,
                             void *workspace, size_t workspace_bytes, u64 *mbits_out, uint8_t *status,
                             hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  size_t slot;
  if (int rc = keys_check("update_keys", rowbytes, keysize, key_slot, elemsize, value_stride, m, &slot)) return rc;
  if (int rc = keys_buffers_check("update_keys", keys, values, true, m, workspace, workspace_bytes, 4 * m, mbits_out))
    return rc;
  snprintf(g_keys_rmw_name, sizeof g_keys_rmw_name, "k_table_locate_keys<last>+k_table_write_keys<%d>",
           (rowbytes & 15) == 0 ? 16 : 8);
  g_kernel = g_keys_rmw_name;
  if (m == 0) return 0;
  int dev;
  if (int rc = current_device(&dev)) return rc;
  KeysLocateArgs l{};
  l.t = make_geom(table, capacity, rowbytes);
  l.keys = static_cast<const uint8_t *>(keys);
  l.keysize = (u32)keysize;
  l.m = m;
  l.slots = static_cast<u32 *>(workspace);
  l.mbits_out = mbits_out;
  const unsigned grid = table_grid(m, 64, dev);
  by_keys_class(keys, keysize, [&](auto L) { k_table_locate_keys<decltype(L)::value, false><<<grid, kBlock, 0, st>>>(l); });
  HIP_TRY(hipGetLastError());
  KeysWriteArgs w{};
  w.t = l.t;
  w.s = row_source(keys, keysize, slot, values, elemsize, value_stride);
  w.m = m;
  w.slots = l.slots;
  w.status = status;
  launch_write_keys(w, 3, dev, st);
  HIP_TRY(hipGetLastError());
  return 0;
}

template <int P>
static void launch_add_write_keys(const KeysAddWriteArgs &w, unsigned grid, hipStream_t st) {
  const bool nt = hook_table_put_nt(kTablePutNt);
  if (row_source_aligned(w.s))
    nt ? k_table_add_write_keys<P, true, true><<<grid, kBlock, 0, st>>>(w)
       : k_table_add_write_keys<P, false, true><<<grid, kBlock, 0, st>>>(w);
  else
    nt ? k_table_add_write_keys<P, true, false><<<grid, kBlock, 0, st>>>(w)
       : k_table_add_write_keys<P, false, false><<<grid, kBlock, 0, st>>>(w);
}

static int table_add_keys(void *table, u64 capacity, size_t rowbytes, const void *keys, size_t keysize,
                          size_t key_slot, const void *values, size_t elemsize, size_t value_stride, size_t m,
                          void *workspace, size_t workspace_bytes, u64 *mbits_out, uint8_t *status, hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  size_t slot;
  if (int rc = keys_check("add_keys", rowbytes, keysize, key_slot, elemsize, value_stride, m, &slot)) return rc;
  if (int rc = keys_buffers_check("add_keys", keys, values, true, m, workspace, workspace_bytes, claim_workspace(m),
                                  mbits_out))
    return rc;
  const bool p16 = (rowbytes & 15) == 0;
  snprintf(g_keys_rmw_name, sizeof g_keys_rmw_name, "k_table_add_claim_keys+k_table_add_write_keys<%d>", p16 ? 16 : 8);
  g_kernel = g_keys_rmw_name;
  if (m == 0) return 0;
  int dev;
  if (int rc = current_device(&dev)) return rc;
  KeysAddClaimArgs c{};
  c.t = make_geom(table, capacity, rowbytes);
  c.keys = static_cast<const uint8_t *>(keys);
  c.keysize = (u32)keysize;
  c.m = m;
  c.slots = static_cast<u32 *>(workspace);
  c.creator = static_cast<uint8_t *>(workspace) + 4 * m;
  c.mbits_out = mbits_out;
  c.status = status;
  const unsigned grid = table_grid(m, 64, dev);
  by_keys_class(keys, keysize, [&](auto L) { k_table_add_claim_keys<decltype(L)::value><<<grid, kBlock, 0, st>>>(c); });
  HIP_TRY(hipGetLastError());
  KeysAddWriteArgs w{};
  w.t = c.t;
  w.s = row_source(keys, keysize, slot, values, elemsize, value_stride);
  w.m = m;
  w.slots = c.slots;
  w.creator = c.creator;
  w.status = status;
  w.np = (u32)(rowbytes / (p16 ? 16 : 8));
  w.gshift = group_shift(w.np);
  const unsigned wgrid = table_grid(m, (u64)(64u >> w.gshift) * kRowsInFlight, dev);
  p16 ? launch_add_write_keys<16>(w, wgrid, st) : launch_add_write_keys<8>(w, wgrid, st);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int table_cswap_keys(void *table, u64 capacity, size_t rowbytes, const void *keys, size_t keysize, size_t m,
                            size_t word_offset, u64 compare, u64 desired, void *replies, size_t reply_stride,
                            void *workspace, size_t workspace_bytes, u64 *mbits_out, hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  if (m >= (1ull << 32)) return fail("table cswap_keys: m must be < 2^32 per call");
  if (keysize == 0) return fail("table cswap_keys: keysize must be >= 1");
  if (keysize > 64)
    return fail("table cswap_keys: keysize must be <= 64; longer keys go through pdht_bucket_records_dev and "
                "pdht_table_cswap_dev");
  if ((word_offset & 7) || word_offset > rowbytes - 8)
    return fail("table cswap_keys: word_offset must be a multiple of 8 and <= rowbytes - 8");
  if ((uintptr_t)replies & 7) return fail("table cswap_keys: replies must be 8-byte aligned");
  if (reply_stride < 16 || (reply_stride & 7))
    return fail("table cswap_keys: reply_stride must be a multiple of 8 and >= 16");
  if (int rc = keys_buffers_check("cswap_keys", keys, nullptr, false, m, workspace, workspace_bytes, 4 * m, mbits_out))
    return rc;
  if (m && !replies) return fail("table cswap_keys: replies must not be NULL");
  g_kernel = "k_table_locate_keys<first>+k_table_cswap";
  if (m == 0) return 0;
  int dev;
  if (int rc = current_device(&dev)) return rc;
  KeysLocateArgs l{};
  l.t = make_geom(table, capacity, rowbytes);
  l.keys = static_cast<const uint8_t *>(keys);
  l.keysize = (u32)keysize;
  l.m = m;
  l.slots = static_cast<u32 *>(workspace);
  l.mbits_out = mbits_out;
  const unsigned grid = table_grid(m, 64, dev);
  by_keys_class(keys, keysize, [&](auto L) { k_table_locate_keys<decltype(L)::value, true><<<grid, kBlock, 0, st>>>(l); });
  HIP_TRY(hipGetLastError());
  CswapArgs c{};
  c.t = l.t;
  c.slots = l.slots;
  c.m = m;
  c.word_offset = word_offset;
  c.compare = compare;
  c.desired = desired;
  c.replies = static_cast<uint8_t *>(replies);
  c.reply_stride = reply_stride;
  launch_table_cswap(c, hook_table_reply_nt(kTableReplyNt), grid, st);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace pdht

using namespace pdht;

PDHT_API size_t pdht_table_update_keys_workspace_bytes(size_t m) { return 4 * m; }

PDHT_API int pdht_table_update_keys_dev(void *table, uint64_t capacity, size_t rowbytes, const void *keys,
                                        size_t keysize, size_t key_slot, const void *values, size_t elemsize,
                                        size_t value_stride, size_t m, void *workspace, size_t workspace_bytes,
                                        uint64_t *mbits_out, uint8_t *status, pdht_hip_stream_t s) {
  return table_update_keys(table, capacity, rowbytes, keys, keysize, key_slot, values, elemsize, value_stride, m,
                           workspace, workspace_bytes, mbits_out, status, ST(s));
}

PDHT_API size_t pdht_table_add_keys_workspace_bytes(size_t m) { return claim_workspace(m); }

PDHT_API int pdht_table_add_keys_dev(void *table, uint64_t capacity, size_t rowbytes, const void *keys, size_t keysize,
                                     size_t key_slot, const void *values, size_t elemsize, size_t value_stride, size_t m,
                                     void *workspace, size_t workspace_bytes, uint64_t *mbits_out, uint8_t *status,
                                     pdht_hip_stream_t s) {
  return table_add_keys(table, capacity, rowbytes, keys, keysize, key_slot, values, elemsize, value_stride, m, workspace,
                        workspace_bytes, mbits_out, status, ST(s));
}

PDHT_API size_t pdht_table_cswap_keys_workspace_bytes(size_t m) { return 4 * m; }

PDHT_API int pdht_table_cswap_keys_dev(void *table, uint64_t capacity, size_t rowbytes, const void *keys,
                                       size_t keysize, size_t m, size_t word_offset, uint64_t compare,
                                       uint64_t desired, void *replies, size_t reply_stride, void *workspace,
                                       size_t workspace_bytes, uint64_t *mbits_out, pdht_hip_stream_t s) {
  return table_cswap_keys(table, capacity, rowbytes, keys, keysize, m, word_offset, compare, desired, replies,
                          reply_stride, workspace, workspace_bytes, mbits_out, ST(s));
}
