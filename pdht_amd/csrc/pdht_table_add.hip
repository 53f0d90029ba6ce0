// pdht_table_add.hip -- insert-if-absent on the device-resident target table
// (include/pdht_hip_table_add.h; kernels in table_add.h): argument checks, launcher and the C ABI.
// Every check runs before any device call.
#include "table_add.h"
#include "table_host.h"

namespace pdht {

static thread_local char g_add_name[96];

static int table_add(void *table, u64 capacity, size_t rowbytes, const void *records, size_t record_stride, size_t m,
                     void *workspace, size_t workspace_bytes, uint8_t *status, void *replies, size_t reply_stride,
                     hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  if (int rc = records_check("add", rowbytes, records, record_stride, m)) return rc;
  if (int rc = buffers_check("add", rowbytes, records, m, workspace, workspace_bytes, claim_workspace(m), replies,
                             reply_stride))
    return rc;
  const bool p16 = rows_p16(rowbytes, records, record_stride), w2 = replies_w2(rowbytes, replies, reply_stride);
  int n = snprintf(g_add_name, sizeof g_add_name, "k_table_add_claim+k_table_add_write<%d>", p16 ? 16 : 8);
  if (replies) snprintf(g_add_name + n, sizeof g_add_name - n, "+k_table_add_reply<%d>", w2 ? 16 : 8);
  g_kernel = g_add_name;
  if (m == 0) return 0;
  int dev;
  if (int rc = current_device(&dev)) return rc;
  AddClaimArgs c{};
  c.t = make_geom(table, capacity, rowbytes);
  c.records = static_cast<const uint8_t *>(records);
  c.record_stride = record_stride;
  c.m = m;
  c.slots = static_cast<u32 *>(workspace);
  c.creator = static_cast<uint8_t *>(workspace) + 4 * m;
  c.status = status;
  k_table_add_claim<<<table_grid(m, 64, dev), kBlock, 0, st>>>(c);
  HIP_TRY(hipGetLastError());
  AddWriteArgs w{};
  w.t = c.t;
  w.records = c.records;
  w.record_stride = record_stride;
  w.m = m;
  w.slots = c.slots;
  w.creator = c.creator;
  w.status = status;
  w.np = (u32)(rowbytes / (p16 ? 16 : 8));
  w.gshift = group_shift(w.np);
  const unsigned wgrid = table_grid(m, (u64)(64u >> w.gshift) * kRowsInFlight, dev);
  const bool put_nt = hook_table_put_nt(kTablePutNt);
  if (p16)
    put_nt ? k_table_add_write<16, true><<<wgrid, kBlock, 0, st>>>(w)
           : k_table_add_write<16, false><<<wgrid, kBlock, 0, st>>>(w);
  else
    put_nt ? k_table_add_write<8, true><<<wgrid, kBlock, 0, st>>>(w)
           : k_table_add_write<8, false><<<wgrid, kBlock, 0, st>>>(w);
  HIP_TRY(hipGetLastError());
  if (!replies) return 0;
  launch_table_reply(c.t, c.slots, m, replies, reply_stride, w2, dev, st);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace pdht

using namespace pdht;

PDHT_API size_t pdht_table_add_workspace_bytes(size_t m) { return claim_workspace(m); }

PDHT_API int pdht_table_add_records_dev(void *table, uint64_t capacity, size_t rowbytes, const void *records,
                                        size_t record_stride, size_t m, void *workspace, size_t workspace_bytes,
                                        uint8_t *status, void *replies, size_t reply_stride, pdht_hip_stream_t s) {
  return table_add(table, capacity, rowbytes, records, record_stride, m, workspace, workspace_bytes, status, replies,
                   reply_stride, ST(s));
}
