// pdht_table.hip -- the device-resident target table and the client's resolve
// (include/pdht_hip_table.h; kernels in table.h): argument checks, launchers
// and the C ABI.  Every check runs before any device call.
#include "table_host.h"

namespace pdht {

static thread_local char g_table_pair[96];

static int table_put(void *table, u64 capacity, size_t rowbytes, const void *records, size_t record_stride,
                     size_t m, void *workspace, size_t workspace_bytes, uint8_t *status, hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  if (int rc = records_check("put", rowbytes, records, record_stride, m)) return rc;
  if (int rc = buffers_check("put", rowbytes, records, m, workspace, workspace_bytes, 4 * m)) return rc;
  const bool p16 = rows_p16(rowbytes, records, record_stride);
  snprintf(g_table_pair, sizeof g_table_pair, "k_table_claim+k_table_write<%d>", p16 ? 16 : 8);
  g_kernel = g_table_pair;
  if (m == 0) return 0;
  int dev;
  if (int rc = current_device(&dev)) return rc;
  ClaimArgs c{};
  c.t = make_geom(table, capacity, rowbytes);
  c.records = static_cast<const uint8_t *>(records);
  c.record_stride = record_stride;
  c.m = m;
  c.slots = static_cast<u32 *>(workspace);
  k_table_claim<<<table_grid(m, 64, dev), kBlock, 0, st>>>(c);
  HIP_TRY(hipGetLastError());
  WriteArgs w{};
  w.t = c.t;
  w.records = c.records;
  w.record_stride = record_stride;
  w.m = m;
  w.slots = c.slots;
  w.status = status;
  launch_table_write(w, p16, 2, dev, st);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int table_get(const void *table, u64 capacity, size_t rowbytes, const void *mbits, size_t mbits_stride,
                     size_t m, void *replies, size_t reply_stride, size_t head, hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  if (m >= (1ull << 32)) return fail("table get: m must be < 2^32 per call%s", "");
  if ((uintptr_t)mbits & 7) return fail("table get: mbits must be 8-byte aligned%s", "");
  if (mbits_stride < 8 || (mbits_stride & 7)) return fail("table get: mbits_stride must be a multiple of 8 and >= 8%s", "");
  if (head != 1 && head != 8) return fail("table get: head must be 1 or 8%s", "");
  if (reply_stride < head + rowbytes) return fail("table get: reply_stride must be >= head + rowbytes%s", "");
  if (m && !mbits) return fail("table get: mbits must not be NULL%s", "");
  if (m && !replies) return fail("table get: replies must not be NULL%s", "");
  // word pieces need the aligned form; anything else moves bytes
  const uintptr_t bits = (uintptr_t)replies | reply_stride;
  const bool words = head == 8 && (bits & 7) == 0;
  const u32 nw = (u32)(rowbytes / 8) + 1;
  const bool w2 = words && (bits & 15) == 0 && (nw & 1) == 0;
  g_kernel = !words ? "k_table_get_bytes" : w2 ? "k_table_get<16>" : "k_table_get<8>";
  if (m == 0) return 0;
  int dev;
  if (int rc = current_device(&dev)) return rc;
  GetArgs a{};
  a.t = make_geom(table, capacity, rowbytes);
  a.mbits = static_cast<const uint8_t *>(mbits);
  a.mbits_stride = mbits_stride;
  a.m = m;
  a.replies = static_cast<uint8_t *>(replies);
  a.reply_stride = reply_stride;
  a.head = (u32)head;
  a.np = !words ? (u32)(head + rowbytes) : w2 ? nw / 2 : nw;
  a.gshift = group_shift(a.np);
  const unsigned grid = table_grid(m, 64u >> a.gshift, dev);
  const bool nt = hook_table_reply_nt(kTableReplyNt);
  if (!words)
    nt ? k_table_get_bytes<true><<<grid, kBlock, 0, st>>>(a) : k_table_get_bytes<false><<<grid, kBlock, 0, st>>>(a);
  else if (w2)
    nt ? k_table_get<2, true><<<grid, kBlock, 0, st>>>(a) : k_table_get<2, false><<<grid, kBlock, 0, st>>>(a);
  else
    nt ? k_table_get<1, true><<<grid, kBlock, 0, st>>>(a) : k_table_get<1, false><<<grid, kBlock, 0, st>>>(a);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int get_resolve(const void *replies, size_t reply_stride, size_t head, size_t value_offset, const void *keys,
                       size_t keysize, const void *index, size_t index_stride, size_t m, void *values,
                       size_t elemsize, size_t value_stride, uint8_t *status, hipStream_t st) {
  if (m >= (1ull << 32)) return fail("get resolve: m must be < 2^32 per call%s", "");
  if (head != 1 && head != 8) return fail("get resolve: head must be 1 or 8%s", "");
  if (keysize == 0) return fail("get resolve: keysize must be >= 1%s", "");
  if (elemsize == 0) return fail("get resolve: elemsize must be >= 1%s", "");
  if (keysize >> 31 || elemsize >> 31 || value_offset >> 31) return fail("get resolve: sizes must be < 2^31%s", "");
  if (value_stride < elemsize) return fail("get resolve: value_stride must be >= elemsize%s", "");
  if (reply_stride < head + keysize || reply_stride < head + value_offset + elemsize)
    return fail("get resolve: reply_stride must hold head + key and head + value_offset + elemsize%s", "");
  if (index) {
    if (index_stride < 4 || (index_stride & 3))
      return fail("get resolve: index_stride must be a multiple of 4 and >= 4%s", "");
    if ((uintptr_t)index & 3) return fail("get resolve: index must be 4-byte aligned%s", "");
  }
  if (m && (!replies || !keys || !values || !status)) return fail("get resolve: null replies, keys, values or status%s", "");
  const uintptr_t bits = ((uintptr_t)replies + head + value_offset) | reply_stride | (uintptr_t)values | value_stride |
                         elemsize;
  const int piece = (bits & 15) == 0 ? 16 : (bits & 7) == 0 ? 8 : (bits & 3) == 0 ? 4 : 1;
  g_kernel = piece == 16 ? "k_get_resolve<16>" : piece == 8 ? "k_get_resolve<8>" : piece == 4 ? "k_get_resolve<4>"
                                                                                              : "k_get_resolve<1>";
  if (m == 0) return 0;
  int dev;
  if (int rc = current_device(&dev)) return rc;
  ResolveArgs a{};
  a.replies = static_cast<const uint8_t *>(replies);
  a.reply_stride = reply_stride;
  a.head = (u32)head;
  a.keysize = (u32)keysize;
  a.value_offset = value_offset;
  a.keys = static_cast<const uint8_t *>(keys);
  a.index = static_cast<const uint8_t *>(index);
  a.index_stride = index_stride;
  a.m = m;
  a.values = static_cast<uint8_t *>(values);
  a.value_stride = value_stride;
  a.status = status;
  a.np = (u32)(elemsize / piece);
  // lanes for the value pieces, and for the key at 4 bytes a lane
  a.gshift = group_shift(std::max<u32>(a.np, (u32)((keysize + 3) / 4)));
  const unsigned grid = table_grid(m, 64u >> a.gshift, dev);
  if (piece == 16)
    k_get_resolve<16><<<grid, kBlock, 0, st>>>(a);
  else if (piece == 8)
    k_get_resolve<8><<<grid, kBlock, 0, st>>>(a);
  else if (piece == 4)
    k_get_resolve<4><<<grid, kBlock, 0, st>>>(a);
  else
    k_get_resolve<1><<<grid, kBlock, 0, st>>>(a);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace pdht

using namespace pdht;

PDHT_API size_t pdht_table_bytes(uint64_t capacity, size_t rowbytes) {
  return geom_ok(capacity, rowbytes) ? table_bytes(capacity, rowbytes) : 0;
}

PDHT_API int pdht_table_init_dev(void *table, size_t bytes, uint64_t capacity, size_t rowbytes,
                                 pdht_hip_stream_t s) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  if (bytes < table_bytes(capacity, rowbytes))
    return fail("table: table_bytes too small (%s%lld bytes needed)", "", (long long)table_bytes(capacity, rowbytes));
  // counters, tags and winner words; rows are only ever read behind a tag
  HIP_TRY(hipMemsetAsync(table, 0, kTableTagsAt + (size_t)(capacity + 1) * 16, ST(s)));
  return 0;
}

PDHT_API size_t pdht_table_put_workspace_bytes(size_t m) { return 4 * m; }

PDHT_API int pdht_table_put_records_dev(void *table, uint64_t capacity, size_t rowbytes, const void *records,
                                        size_t record_stride, size_t m, void *workspace, size_t workspace_bytes,
                                        uint8_t *status, pdht_hip_stream_t s) {
  return table_put(table, capacity, rowbytes, records, record_stride, m, workspace, workspace_bytes, status, ST(s));
}

PDHT_API size_t pdht_table_reply_bytes(size_t head, size_t rowbytes) {
  return (head == 1 || head == 8) && geom_ok(64, rowbytes) ? head + rowbytes : 0;
}

PDHT_API int pdht_table_get_dev(const void *table, uint64_t capacity, size_t rowbytes, const void *mbits,
                                size_t mbits_stride, size_t m, void *replies, size_t reply_stride, size_t head,
                                pdht_hip_stream_t s) {
  return table_get(table, capacity, rowbytes, mbits, mbits_stride, m, replies, reply_stride, head, ST(s));
}

PDHT_API int pdht_table_counts_dev(const void *table, uint64_t *counts4, pdht_hip_stream_t s) {
  if (!table || !counts4) return fail("table counts: null table or counts%s", "");
  if (((uintptr_t)table & 15) || ((uintptr_t)counts4 & 7)) return fail("table counts: misaligned table or counts%s", "");
  HIP_TRY(hipMemcpyAsync(counts4, table, 32, hipMemcpyDeviceToDevice, ST(s)));
  return 0;
}

PDHT_API int pdht_get_resolve_dev(const void *replies, size_t reply_stride, size_t head, size_t value_offset,
                                  const void *keys, size_t keysize, const void *index, size_t index_stride, size_t m,
                                  void *values, size_t elemsize, size_t value_stride, uint8_t *status,
                                  pdht_hip_stream_t s) {
  return get_resolve(replies, reply_stride, head, value_offset, keys, keysize, index, index_stride, m, values,
                     elemsize, value_stride, status, ST(s));
}
