// pdht_table_reduce.hip -- reductions on the entries of the device-resident target table
// (include/pdht_hip_table_reduce.h; kernels: k_table_acc<T, .., OP> of table_acc.h, k_table_add_reply<W> of
// table_add.h): argument checks, launcher and the C ABI.  Every check runs before any device call.
#include "pdht_hip_table_reduce.h"
#include "table_add.h"
#include "table_host.h"

namespace pdht {

static_assert(PDHT_RED_ADD == kRedAdd && PDHT_RED_MIN == kRedMin && PDHT_RED_MAX == kRedMax &&
                  PDHT_RED_AND == kRedAnd && PDHT_RED_OR == kRedOr && PDHT_RED_XOR == kRedXor,
              "the header's ops are the kernels'");

static thread_local char g_red_name[128];

// In-wave combining of the operands that share a slot, as the accumulate's sums (pdht_table_acc.hip)
constexpr bool kTableRedCombine = true;

static size_t red_workspace(size_t m, unsigned flags, bool replies) {
  return (flags & PDHT_ACC_INSERT) ? 4 * m + ((m + 3) & ~(size_t)3) : replies ? 4 * m : 0;
}

// As the accumulate: the form without combining exists for the integer types only, no k_table_acc<double, *,
// false, *> is built for any op (EXPERIMENTS.md §R12)
template <class T, bool INSERT, int OP>
static void red_launch(const AccArgs &a, unsigned grid, hipStream_t st) {
  if constexpr (std::is_same<T, double>::value) {
    k_table_acc<T, INSERT, true, OP><<<grid, kBlock, 0, st>>>(a);
  } else {
    if (hook_table_acc_combine(kTableRedCombine))
      k_table_acc<T, INSERT, true, OP><<<grid, kBlock, 0, st>>>(a);
    else
      k_table_acc<T, INSERT, false, OP><<<grid, kBlock, 0, st>>>(a);
  }
}

template <class T, bool INSERT>
static void red_op(int op, const AccArgs &a, unsigned grid, hipStream_t st) {
  switch (op) {
    case kRedAdd:
      return red_launch<T, INSERT, kRedAdd>(a, grid, st);
    case kRedMin:
      return red_launch<T, INSERT, kRedMin>(a, grid, st);
    case kRedMax:
      return red_launch<T, INSERT, kRedMax>(a, grid, st);
  }
  if constexpr (!std::is_same<T, double>::value) {  // (the checks let no bitwise op on doubles through)
    switch (op) {
      case kRedAnd:
        return red_launch<T, INSERT, kRedAnd>(a, grid, st);
      case kRedOr:
        return red_launch<T, INSERT, kRedOr>(a, grid, st);
      case kRedXor:
        return red_launch<T, INSERT, kRedXor>(a, grid, st);
    }
  }
}

static int table_reduce(void *table, u64 capacity, size_t rowbytes, const void *records, size_t record_stride,
                        size_t m, int datatype, int op, size_t value_offset, size_t elems, unsigned flags,
                        void *workspace, size_t workspace_bytes, uint8_t *status, void *replies, size_t reply_stride,
                        hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  if (m >= (1ull << 32)) return fail("table reduce: m must be < 2^32 per call%s", "");
  if (record_stride < 24 + rowbytes || (record_stride & 7))
    return fail("table reduce: record_stride must be a multiple of 8 and >= 24 + rowbytes%s", "");
  if ((uintptr_t)records & 7) return fail("table reduce: records must be 8-byte aligned%s", "");
  if (datatype != PDHT_ACC_INT32 && datatype != PDHT_ACC_INT64 && datatype != PDHT_ACC_DOUBLE)
    return fail("table reduce: datatype must be PDHT_ACC_INT32, PDHT_ACC_INT64 or PDHT_ACC_DOUBLE%s", "");
  if (op < PDHT_RED_ADD || op > PDHT_RED_XOR) return fail("table reduce: op must be PDHT_RED_ADD .. PDHT_RED_XOR%s", "");
  if (datatype == PDHT_ACC_DOUBLE && op >= PDHT_RED_AND)
    return fail("table reduce: PDHT_RED_AND, _OR and _XOR are not defined for PDHT_ACC_DOUBLE%s", "");
  if (flags & ~PDHT_ACC_INSERT) return fail("table reduce: unknown flags%s", "");
  const size_t size = datatype == PDHT_ACC_INT32 ? 4 : 8;
  if (value_offset % size) return fail("table reduce: value_offset must be a multiple of the element size%s", "");
  // (rowbytes < 2^31: neither the division nor the sum can wrap)
  if (elems == 0 || value_offset > rowbytes || elems > (rowbytes - value_offset) / size)
    return fail("table reduce: elems must be >= 1 and value_offset + elems * size <= rowbytes%s", "");
  const bool insert = (flags & PDHT_ACC_INSERT) != 0;
  const size_t need = red_workspace(m, flags, replies != nullptr);
  if (need && ((uintptr_t)workspace & 3)) return fail("table reduce: workspace must be 4-byte aligned%s", "");
  if (workspace_bytes < need)
    return fail("table reduce: workspace too small (%s%lld bytes needed)", "", (long long)need);
  if (replies) {  // (without replies the stride means nothing)
    if ((uintptr_t)replies & 7) return fail("table reduce: replies must be 8-byte aligned%s", "");
    if (reply_stride < 8 + rowbytes || (reply_stride & 7))
      return fail("table reduce: reply_stride must be a multiple of 8 and >= 8 + rowbytes%s", "");
  }
  if (m && !records) return fail("table reduce: records must not be NULL%s", "");
  if (need && !workspace) return fail("table reduce: workspace must not be NULL%s", "");
  static const char *const kOps[] = {"", ",min", ",max", ",and", ",or", ",xor"};
  const char *ty = datatype == PDHT_ACC_INT32 ? "i32" : datatype == PDHT_ACC_INT64 ? "i64" : "f64";
  const u32 nw = (u32)(rowbytes / 8) + 1;  // the get's piece rule for the replies
  const bool w2 = replies && (((uintptr_t)replies | reply_stride) & 15) == 0 && (nw & 1) == 0;
  int n = snprintf(g_red_name, sizeof g_red_name, insert ? "k_table_acc_claim+k_table_acc<%s%s,insert>" : "k_table_acc<%s%s>",
                   ty, kOps[op]);
  if (replies) snprintf(g_red_name + n, sizeof g_red_name - n, "+k_table_add_reply<%d>", w2 ? 16 : 8);
  g_kernel = g_red_name;
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
  u32 *slots = static_cast<u32 *>(workspace);
  if (insert) {
    AccClaimArgs c{};
    c.t = a.t;
    c.records = a.records;
    c.record_stride = record_stride;
    c.m = m;
    c.slots = slots;
    c.creator = static_cast<uint8_t *>(workspace) + 4 * m;
    c.value_offset = value_offset;
    c.region_words = elems * size / 4;
    const u64 fill = red_identity_bits(op, size, datatype == PDHT_ACC_DOUBLE);
    c.fill[0] = (u32)fill;
    c.fill[1] = (u32)(fill >> 32);
    k_table_acc_claim<<<table_grid(m, 64, dev), kBlock, 0, st>>>(c);
    HIP_TRY(hipGetLastError());
    a.slots = c.slots;
    a.creator = c.creator;
  } else if (replies) {
    a.slot_out = slots;
  }
  const unsigned grid = table_grid(m, 64u >> a.gshift, dev);
  if (datatype == PDHT_ACC_INT32)
    insert ? red_op<u32, true>(op, a, grid, st) : red_op<u32, false>(op, a, grid, st);
  else if (datatype == PDHT_ACC_INT64)
    insert ? red_op<u64, true>(op, a, grid, st) : red_op<u64, false>(op, a, grid, st);
  else
    insert ? red_op<double, true>(op, a, grid, st) : red_op<double, false>(op, a, grid, st);
  HIP_TRY(hipGetLastError());
  if (!replies) return 0;
  // behind k_table_acc no kernel of the call writes a row: plain loads of the reduced rows
  AddReplyArgs r{};
  r.t = a.t;
  r.slots = slots;
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

PDHT_API size_t pdht_table_reduce_workspace_bytes(size_t m, unsigned flags, int with_replies) {
  return red_workspace(m, flags, with_replies != 0);
}

PDHT_API int pdht_table_reduce_records_dev(void *table, uint64_t capacity, size_t rowbytes, const void *records,
                                           size_t record_stride, size_t m, int datatype, int op, size_t value_offset,
                                           size_t elems, unsigned flags, void *workspace, size_t workspace_bytes,
                                           uint8_t *status, void *replies, size_t reply_stride, pdht_hip_stream_t s) {
  return table_reduce(table, capacity, rowbytes, records, record_stride, m, datatype, op, value_offset, elems, flags,
                      workspace, workspace_bytes, status, replies, reply_stride, ST(s));
}
