// pdht_table_rmw.hip -- update and compare-and-swap on the device-resident target table
// (include/pdht_hip_table_rmw.h; kernels in table_rmw.h): argument checks, launchers and the C ABI.
// Every check runs before any device call.
#include "table_rmw.h"
#include "table_host.h"

namespace pdht {

static thread_local char g_rmw_pair[96];

static int table_update(void *table, u64 capacity, size_t rowbytes, const void *records, size_t record_stride,
                        size_t m, void *workspace, size_t workspace_bytes, uint8_t *status, hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  if (int rc = records_check("update", rowbytes, records, record_stride, m)) return rc;
  if (int rc = buffers_check("update", rowbytes, records, m, workspace, workspace_bytes, 4 * m)) return rc;
  const bool p16 = rows_p16(rowbytes, records, record_stride);
  snprintf(g_rmw_pair, sizeof g_rmw_pair, "k_table_locate<last>+k_table_write<%d>", p16 ? 16 : 8);
  g_kernel = g_rmw_pair;
  if (m == 0) return 0;
  int dev;
  if (int rc = current_device(&dev)) return rc;
  LocateArgs l{};
  l.t = make_geom(table, capacity, rowbytes);
  l.mbits = static_cast<const uint8_t *>(records) + 16;
  l.mbits_stride = record_stride;
  l.m = m;
  l.slots = static_cast<u32 *>(workspace);
  k_table_locate<false><<<table_grid(m, 64, dev), kBlock, 0, st>>>(l);
  HIP_TRY(hipGetLastError());
  WriteArgs w{};
  w.t = l.t;
  w.records = static_cast<const uint8_t *>(records);
  w.record_stride = record_stride;
  w.m = m;
  w.slots = l.slots;
  w.status = status;
  launch_table_write(w, p16, 3, dev, st);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int table_cswap(void *table, u64 capacity, size_t rowbytes, const void *mbits, size_t mbits_stride, size_t m,
                       size_t word_offset, u64 compare, u64 desired, void *replies, size_t reply_stride,
                       void *workspace, size_t workspace_bytes, hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  if (m >= (1ull << 32)) return fail("table cswap: m must be < 2^32 per call%s", "");
  if ((uintptr_t)mbits & 7) return fail("table cswap: mbits must be 8-byte aligned%s", "");
  if (mbits_stride < 8 || (mbits_stride & 7))
    return fail("table cswap: mbits_stride must be a multiple of 8 and >= 8%s", "");
  if ((word_offset & 7) || word_offset > rowbytes - 8)
    return fail("table cswap: word_offset must be a multiple of 8 and <= rowbytes - 8%s", "");
  if ((uintptr_t)replies & 7) return fail("table cswap: replies must be 8-byte aligned%s", "");
  if (reply_stride < 16 || (reply_stride & 7))
    return fail("table cswap: reply_stride must be a multiple of 8 and >= 16%s", "");
  if ((uintptr_t)workspace & 3) return fail("table cswap: workspace must be 4-byte aligned%s", "");
  if (workspace_bytes < 4 * m)
    return fail("table cswap: workspace too small (%s%lld bytes needed)", "", (long long)(4 * m));
  if (m && !mbits) return fail("table cswap: mbits must not be NULL%s", "");
  if (m && !replies) return fail("table cswap: replies must not be NULL%s", "");
  if (m && !workspace) return fail("table cswap: workspace must not be NULL%s", "");
  g_kernel = "k_table_locate<first>+k_table_cswap";
  if (m == 0) return 0;
  int dev;
  if (int rc = current_device(&dev)) return rc;
  LocateArgs l{};
  l.t = make_geom(table, capacity, rowbytes);
  l.mbits = static_cast<const uint8_t *>(mbits);
  l.mbits_stride = mbits_stride;
  l.m = m;
  l.slots = static_cast<u32 *>(workspace);
  const unsigned grid = table_grid(m, 64, dev);
  k_table_locate<true><<<grid, kBlock, 0, st>>>(l);
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

PDHT_API size_t pdht_table_update_workspace_bytes(size_t m) { return 4 * m; }

PDHT_API int pdht_table_update_records_dev(void *table, uint64_t capacity, size_t rowbytes, const void *records,
                                           size_t record_stride, size_t m, void *workspace, size_t workspace_bytes,
                                           uint8_t *status, pdht_hip_stream_t s) {
  return table_update(table, capacity, rowbytes, records, record_stride, m, workspace, workspace_bytes, status, ST(s));
}

PDHT_API size_t pdht_table_cswap_workspace_bytes(size_t m) { return 4 * m; }

PDHT_API int pdht_table_cswap_dev(void *table, uint64_t capacity, size_t rowbytes, const void *mbits,
                                  size_t mbits_stride, size_t m, size_t word_offset, uint64_t compare,
                                  uint64_t desired, void *replies, size_t reply_stride, void *workspace,
                                  size_t workspace_bytes, pdht_hip_stream_t s) {
  return table_cswap(table, capacity, rowbytes, mbits, mbits_stride, m, word_offset, compare, desired, replies,
                     reply_stride, workspace, workspace_bytes, ST(s));
}
