// pdht_table_add.hip -- insert-if-absent on the device-resident target table
// (include/pdht_hip_table_add.h; kernels in table_add.h): argument checks, launcher and the C ABI.
// Every check runs before any device call.
#include "table_add.h"
#include "table_host.h"

namespace pdht {

static thread_local char g_add_name[96];

// the slots and the creator marks: the inserting accumulate's formula
static size_t add_workspace(size_t m) { return 4 * m + ((m + 3) & ~(size_t)3); }

static int table_add(void *table, u64 capacity, size_t rowbytes, const void *records, size_t record_stride, size_t m,
                     void *workspace, size_t workspace_bytes, uint8_t *status, void *replies, size_t reply_stride,
                     hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  if (m >= (1ull << 32)) return fail("table add: m must be < 2^32 per call%s", "");
  if (record_stride < 24 + rowbytes || (record_stride & 7))
    return fail("table add: record_stride must be a multiple of 8 and >= 24 + rowbytes%s", "");
  if ((uintptr_t)records & 7) return fail("table add: records must be 8-byte aligned%s", "");
  if ((uintptr_t)workspace & 3) return fail("table add: workspace must be 4-byte aligned%s", "");
  const size_t need = add_workspace(m);
  if (workspace_bytes < need)
    return fail("table add: workspace too small (%s%lld bytes needed)", "", (long long)need);
  if (replies) {  // (without replies the stride means nothing)
    if ((uintptr_t)replies & 7) return fail("table add: replies must be 8-byte aligned%s", "");
    if (reply_stride < 8 + rowbytes || (reply_stride & 7))
      return fail("table add: reply_stride must be a multiple of 8 and >= 8 + rowbytes%s", "");
  }
  if (m && !records) return fail("table add: records must not be NULL%s", "");
  if (m && !workspace) return fail("table add: workspace must not be NULL%s", "");
  // the put's piece rule for the rows, the get's for the replies
  const bool p16 = (rowbytes & 15) == 0 && (record_stride & 15) == 0 && (((uintptr_t)records + 24) & 15) == 0;
  const u32 nw = (u32)(rowbytes / 8) + 1;
  const bool w2 = replies && (((uintptr_t)replies | reply_stride) & 15) == 0 && (nw & 1) == 0;
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
  AddReplyArgs r{};
  r.t = c.t;
  r.slots = c.slots;
  r.m = m;
  r.replies = static_cast<uint8_t *>(replies);
  r.reply_stride = reply_stride;
  r.np = w2 ? nw / 2 : nw;
  r.gshift = group_shift(r.np);
  const unsigned rgrid = table_grid(m, 64u >> r.gshift, dev);
  const bool reply_nt = hook_table_reply_nt(kTableReplyNt);
  if (w2)
    reply_nt ? k_table_add_reply<2, true><<<rgrid, kBlock, 0, st>>>(r)
             : k_table_add_reply<2, false><<<rgrid, kBlock, 0, st>>>(r);
  else
    reply_nt ? k_table_add_reply<1, true><<<rgrid, kBlock, 0, st>>>(r)
             : k_table_add_reply<1, false><<<rgrid, kBlock, 0, st>>>(r);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace pdht

using namespace pdht;

PDHT_API size_t pdht_table_add_workspace_bytes(size_t m) { return add_workspace(m); }

PDHT_API int pdht_table_add_records_dev(void *table, uint64_t capacity, size_t rowbytes, const void *records,
                                        size_t record_stride, size_t m, void *workspace, size_t workspace_bytes,
                                        uint8_t *status, void *replies, size_t reply_stride, pdht_hip_stream_t s) {
  return table_add(table, capacity, rowbytes, records, record_stride, m, workspace, workspace_bytes, status, replies,
                   reply_stride, ST(s));
}
