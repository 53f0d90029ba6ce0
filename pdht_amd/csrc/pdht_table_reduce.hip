// pdht_table_reduce.hip -- the accumulate and the reductions on the entries of the device-resident target
// table (include/pdht_hip_table_acc.h, include/pdht_hip_table_reduce.h; kernels: k_table_acc<T, .., OP> of
// table_acc.h, the replies k_table_get<W, .., slots> of table.h): argument checks, launcher and the C ABI.
// The accumulate is the reduce with the sum and without replies: one implementation behind both entry points.
// Every check runs before any device call.
#include "pdht_hip_table_reduce.h"
#include "table_acc.h"
#include "table_host.h"

namespace pdht {

static_assert(PDHT_RED_ADD == kRedAdd && PDHT_RED_MIN == kRedMin && PDHT_RED_MAX == kRedMax &&
                  PDHT_RED_AND == kRedAnd && PDHT_RED_OR == kRedOr && PDHT_RED_XOR == kRedXor,
              "the header's ops are the kernels'");

static thread_local char g_red_name[128];

// In-wave combining of the operands that share a slot (EXPERIMENTS.md §R12 has the alternative's times)
constexpr bool kTableRedCombine = true;

static size_t red_workspace(size_t m, unsigned flags, bool replies) {
  return (flags & PDHT_ACC_INSERT) ? claim_workspace(m) : replies ? 4 * m : 0;
}

// The form without combining exists for the integer types only: no k_table_acc<double, *, false, *> is built
// for any op (EXPERIMENTS.md §R12: the run that posted one fp64 atomic per record on one word stalled)
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

// acc: the call came in as pdht_table_acc_records_dev -- its own name in the messages, no op but the sum, no replies
static int table_reduce(bool acc, void *table, u64 capacity, size_t rowbytes, const void *records,
                        size_t record_stride, size_t m, int datatype, int op, size_t value_offset, size_t elems,
                        unsigned flags, void *workspace, size_t workspace_bytes, uint8_t *status, void *replies,
                        size_t reply_stride, hipStream_t st) {
  const char *name = acc ? "acc" : "reduce";
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  if (int rc = records_check(name, rowbytes, records, record_stride, m)) return rc;
  if (datatype != PDHT_ACC_INT32 && datatype != PDHT_ACC_INT64 && datatype != PDHT_ACC_DOUBLE)
    return fail("table %s: datatype must be PDHT_ACC_INT32, PDHT_ACC_INT64 or PDHT_ACC_DOUBLE", name);
  if (acc && op != PDHT_ACC_ADD) return fail("table acc: op must be PDHT_ACC_ADD");
  if (op < PDHT_RED_ADD || op > PDHT_RED_XOR) return fail("table reduce: op must be PDHT_RED_ADD .. PDHT_RED_XOR");
  if (datatype == PDHT_ACC_DOUBLE && op >= PDHT_RED_AND)
    return fail("table reduce: PDHT_RED_AND, _OR and _XOR are not defined for PDHT_ACC_DOUBLE");
  if (flags & ~PDHT_ACC_INSERT) return fail("table %s: unknown flags", name);
  const size_t size = datatype == PDHT_ACC_INT32 ? 4 : 8;
  if (value_offset % size) return fail("table %s: value_offset must be a multiple of the element size", name);
  // (rowbytes < 2^31: neither the division nor the sum can wrap)
  if (elems == 0 || value_offset > rowbytes || elems > (rowbytes - value_offset) / size)
    return fail("table %s: elems must be >= 1 and value_offset + elems * size <= rowbytes", name);
  const bool insert = (flags & PDHT_ACC_INSERT) != 0;
  const size_t need = red_workspace(m, flags, replies != nullptr);
  if (int rc = buffers_check(name, rowbytes, records, m, need ? workspace : nullptr, workspace_bytes, need, replies,
                             reply_stride))
    return rc;
  static const char *const kOps[] = {"", ",min", ",max", ",and", ",or", ",xor"};
  const char *ty = datatype == PDHT_ACC_INT32 ? "i32" : datatype == PDHT_ACC_INT64 ? "i64" : "f64";
  const bool w2 = replies_w2(rowbytes, replies, reply_stride);
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
  launch_table_reply(a.t, slots, m, replies, reply_stride, w2, dev, st);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace pdht

using namespace pdht;

PDHT_API size_t pdht_table_acc_workspace_bytes(size_t m, unsigned flags) { return red_workspace(m, flags, false); }

PDHT_API int pdht_table_acc_records_dev(void *table, uint64_t capacity, size_t rowbytes, const void *records,
                                        size_t record_stride, size_t m, int datatype, int op, size_t value_offset,
                                        size_t elems, unsigned flags, void *workspace, size_t workspace_bytes,
                                        uint8_t *status, pdht_hip_stream_t s) {
  return table_reduce(true, table, capacity, rowbytes, records, record_stride, m, datatype, op, value_offset, elems,
                      flags, workspace, workspace_bytes, status, nullptr, 0, ST(s));
}

PDHT_API size_t pdht_table_reduce_workspace_bytes(size_t m, unsigned flags, int with_replies) {
  return red_workspace(m, flags, with_replies != 0);
}

PDHT_API int pdht_table_reduce_records_dev(void *table, uint64_t capacity, size_t rowbytes, const void *records,
                                           size_t record_stride, size_t m, int datatype, int op, size_t value_offset,
                                           size_t elems, unsigned flags, void *workspace, size_t workspace_bytes,
                                           uint8_t *status, void *replies, size_t reply_stride, pdht_hip_stream_t s) {
  return table_reduce(false, table, capacity, rowbytes, records, record_stride, m, datatype, op, value_offset, elems,
                      flags, workspace, workspace_bytes, status, replies, reply_stride, ST(s));
}
