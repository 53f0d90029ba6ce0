// pdht_table_acc.hip -- the associative accumulate on the device-resident target table
// (include/pdht_hip_table_acc.h; kernels in table_acc.h): argument checks, launcher and the C ABI.
// Every check runs before any device call.
#include "table_acc.h"
#include "table_host.h"

namespace pdht {

static thread_local char g_acc_name[64];

// In-wave sums of the addends that share a slot (EXPERIMENTS.md §R12 has the alternative's times)
constexpr bool kTableAccCombine = true;

static size_t acc_workspace(size_t m, unsigned flags) {
  return (flags & PDHT_ACC_INSERT) ? 4 * m + ((m + 3) & ~(size_t)3) : 0;
}

// The alternative without the in-wave sums exists for the integer types only: k_table_acc<double, *, false>
// is not built (EXPERIMENTS.md §R12: the run that posted one fp64 atomic per record on one word stalled)
template <class T, bool INSERT>
static void acc_launch(const AccArgs &a, unsigned grid, hipStream_t st) {
  if constexpr (std::is_same<T, double>::value) {
    k_table_acc<T, INSERT, true><<<grid, kBlock, 0, st>>>(a);
  } else {
    if (hook_table_acc_combine(kTableAccCombine))
      k_table_acc<T, INSERT, true><<<grid, kBlock, 0, st>>>(a);
    else
      k_table_acc<T, INSERT, false><<<grid, kBlock, 0, st>>>(a);
  }
}

static int table_acc(void *table, u64 capacity, size_t rowbytes, const void *records, size_t record_stride, size_t m,
                     int datatype, int op, size_t value_offset, size_t elems, unsigned flags, void *workspace,
                     size_t workspace_bytes, uint8_t *status, hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  if (m >= (1ull << 32)) return fail("table acc: m must be < 2^32 per call%s", "");
  if (record_stride < 24 + rowbytes || (record_stride & 7))
    return fail("table acc: record_stride must be a multiple of 8 and >= 24 + rowbytes%s", "");
  if ((uintptr_t)records & 7) return fail("table acc: records must be 8-byte aligned%s", "");
  if (datatype != PDHT_ACC_INT32 && datatype != PDHT_ACC_INT64 && datatype != PDHT_ACC_DOUBLE)
    return fail("table acc: datatype must be PDHT_ACC_INT32, PDHT_ACC_INT64 or PDHT_ACC_DOUBLE%s", "");
  if (op != PDHT_ACC_ADD) return fail("table acc: op must be PDHT_ACC_ADD%s", "");
  if (flags & ~PDHT_ACC_INSERT) return fail("table acc: unknown flags%s", "");
  const size_t size = datatype == PDHT_ACC_INT32 ? 4 : 8;
  if (value_offset % size) return fail("table acc: value_offset must be a multiple of the element size%s", "");
  // (rowbytes < 2^31: neither the division nor the sum can wrap)
  if (elems == 0 || value_offset > rowbytes || elems > (rowbytes - value_offset) / size)
    return fail("table acc: elems must be >= 1 and value_offset + elems * size <= rowbytes%s", "");
  const bool insert = (flags & PDHT_ACC_INSERT) != 0;
  const size_t need = acc_workspace(m, flags);
  if (need && ((uintptr_t)workspace & 3)) return fail("table acc: workspace must be 4-byte aligned%s", "");
  if (workspace_bytes < need)
    return fail("table acc: workspace too small (%s%lld bytes needed)", "", (long long)need);
  if (m && !records) return fail("table acc: records must not be NULL%s", "");
  if (need && !workspace) return fail("table acc: workspace must not be NULL%s", "");
  const char *ty = datatype == PDHT_ACC_INT32 ? "i32" : datatype == PDHT_ACC_INT64 ? "i64" : "f64";
  snprintf(g_acc_name, sizeof g_acc_name, insert ? "k_table_acc_claim+k_table_acc<%s,insert>" : "k_table_acc<%s>", ty);
  g_kernel = g_acc_name;
  if (m == 0) return 0;
  int dev;
  if (int rc = current_device(&dev)) return rc;
  AccArgs a{};
  a.t = make_geom(table, capacity, rowbytes);
  a.records = static_cast<const uint8_t *>(records);
  a.record_stride = record_stride;
  a.m = m;
  a.status = status;
  a.value_offset = value_offset;
  a.elems = elems;
  a.gshift = group_shift((u32)std::min<size_t>(elems, 64));
  if (insert) {
    AccClaimArgs c{};
    c.t = a.t;
    c.records = a.records;
    c.record_stride = record_stride;
    c.m = m;
    c.slots = static_cast<u32 *>(workspace);
    c.creator = static_cast<uint8_t *>(workspace) + 4 * m;
    c.value_offset = value_offset;
    c.region_words = elems * size / 4;
    k_table_acc_claim<<<table_grid(m, 64, dev), kBlock, 0, st>>>(c);
    HIP_TRY(hipGetLastError());
    a.slots = c.slots;
    a.creator = c.creator;
  }
  const unsigned grid = table_grid(m, 64u >> a.gshift, dev);
  if (datatype == PDHT_ACC_INT32)
    insert ? acc_launch<u32, true>(a, grid, st) : acc_launch<u32, false>(a, grid, st);
  else if (datatype == PDHT_ACC_INT64)
    insert ? acc_launch<u64, true>(a, grid, st) : acc_launch<u64, false>(a, grid, st);
  else
    insert ? acc_launch<double, true>(a, grid, st) : acc_launch<double, false>(a, grid, st);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace pdht

using namespace pdht;

PDHT_API size_t pdht_table_acc_workspace_bytes(size_t m, unsigned flags) { return acc_workspace(m, flags); }

PDHT_API int pdht_table_acc_records_dev(void *table, uint64_t capacity, size_t rowbytes, const void *records,
                                        size_t record_stride, size_t m, int datatype, int op, size_t value_offset,
                                        size_t elems, unsigned flags, void *workspace, size_t workspace_bytes,
                                        uint8_t *status, pdht_hip_stream_t s) {
  return table_acc(table, capacity, rowbytes, records, record_stride, m, datatype, op, value_offset, elems, flags,
                   workspace, workspace_bytes, status, ST(s));
}
