// table_host.h -- the host side that the translation units of the device-resident target table share
// (pdht_table.hip: put, get, resolve; pdht_table_rmw.hip: update, compare-and-swap; pdht_table_add.hip:
// insert-if-absent; pdht_table_reduce.hip: accumulate and reduce; pdht_table_iter.hip: export): the
// geometry checks, the layout of the caller's buffer as pointers, the launch arithmetic of the lane-group
// kernels, the checks of a records batch, and the launchers of the kernels that several operations end with.
#pragma once
#include "table.h"

namespace pdht {

// Store policy of the get replies and of a put's rows (EXPERIMENTS.md §R9: measured per rowbytes); the
// replies of a compare-and-swap and the rows of an update follow them (pdht_table_rmw.hip)
constexpr bool kTableReplyNt = true;
constexpr bool kTablePutNt = true;

static bool geom_ok(u64 capacity, size_t rowbytes) {
  return capacity >= 64 && capacity <= (1ull << 31) && (capacity & (capacity - 1)) == 0 && rowbytes != 0 &&
         (rowbytes & 7) == 0 && rowbytes < (1ull << 31);
}

static size_t table_bytes(u64 capacity, size_t rowbytes) {
  return kTableTagsAt + (size_t)(capacity + 1) * (16 + rowbytes);
}

static int geom_check(const void *table, u64 capacity, size_t rowbytes) {
  if (capacity < 64 || capacity > (1ull << 31) || (capacity & (capacity - 1)))
    return fail("table: capacity must be a power of two in 64 .. 2^31%s", "");
  if (rowbytes == 0 || (rowbytes & 7) || rowbytes >= (1ull << 31))
    return fail("table: rowbytes must be a multiple of 8, >= 8 and < 2^31%s", "");
  if (!table) return fail("table: table must not be NULL%s", "");
  if ((uintptr_t)table & 15) return fail("table: table must be 16-byte aligned%s", "");
  return 0;
}

static TableGeom make_geom(const void *table, u64 capacity, size_t rowbytes) {
  TableGeom t{};
  uint8_t *b = static_cast<uint8_t *>(const_cast<void *>(table));
  t.counters = reinterpret_cast<u64 *>(b);
  t.tags = reinterpret_cast<u64 *>(b + kTableTagsAt);
  t.win = t.tags + capacity + 1;
  t.rows = reinterpret_cast<uint8_t *>(t.win + capacity + 1);
  t.mask = capacity - 1;
  t.shift = 64 - (u32)__builtin_ctzll(capacity);
  t.cap = (u32)capacity;
  t.rowbytes = rowbytes;
  return t;
}

static u32 group_shift(u32 pieces) {
  u32 s = 0;
  while (s < 6 && (1u << s) < pieces) ++s;
  return s;
}

// workgroups for `m` items at `per_wave` items per wave
static unsigned table_grid(u64 m, u64 per_wave, int dev) {
  const u64 waves = (m + per_wave - 1) / per_wave;
  return grid_for((waves + kWavesPerBlock - 1) / kWavesPerBlock, 8, dev);
}

// The checks of a records batch, op = "put", "update", "acc", "add" or "reduce" for the messages.  They
// come in two parts because the accumulate and the reduce check their datatype, op and region in between.
static int records_check(const char *op, size_t rowbytes, const void *records, size_t record_stride, size_t m) {
  if (m >= (1ull << 32)) return fail("table %s: m must be < 2^32 per call", op);
  if (record_stride < 24 + rowbytes || (record_stride & 7))
    return fail("table %s: record_stride must be a multiple of 8 and >= 24 + rowbytes", op);
  if ((uintptr_t)records & 7) return fail("table %s: records must be 8-byte aligned", op);
  return 0;
}

// need: the workspace bytes of this call.  replies: null without replies (then the stride means nothing).
// A call that needs no workspace passes a null one, whatever the caller gave.
static int buffers_check(const char *op, size_t rowbytes, const void *records, size_t m, const void *workspace,
                         size_t workspace_bytes, size_t need, const void *replies = nullptr,
                         size_t reply_stride = 0) {
  if ((uintptr_t)workspace & 3) return fail("table %s: workspace must be 4-byte aligned", op);
  if (workspace_bytes < need) return fail("table %s: workspace too small (%lld bytes needed)", op, (long long)need);
  if (replies) {
    if ((uintptr_t)replies & 7) return fail("table %s: replies must be 8-byte aligned", op);
    if (reply_stride < 8 + rowbytes || (reply_stride & 7))
      return fail("table %s: reply_stride must be a multiple of 8 and >= 8 + rowbytes", op);
  }
  if (m && !records) return fail("table %s: records must not be NULL", op);
  if (need && !workspace) return fail("table %s: workspace must not be NULL", op);
  return 0;
}

// Workspace of the operations that may create entries (accumulate, insert-if-absent, reduce): every
// record's slot, then its creator mark, rounded up to whole words
static size_t claim_workspace(size_t m) { return 4 * m + ((m + 3) & ~(size_t)3); }

// The put's piece rule: 16-byte row pieces where rows and records allow them
static bool rows_p16(size_t rowbytes, const void *records, size_t record_stride) {
  return (rowbytes & 15) == 0 && (record_stride & 15) == 0 && (((uintptr_t)records + 24) & 15) == 0;
}

// k_table_write of a put (absent 2) or an update (absent 3) behind the kernel that left slots and winner
// words.  (This launcher and the next are templates only so that a unit builds the kernels when it calls them.)
template <int P = 16>
static void launch_table_write(WriteArgs w, bool p16, u32 absent, int dev, hipStream_t st) {
  w.np = (u32)(w.t.rowbytes / (p16 ? P : P / 2));
  w.gshift = group_shift(w.np);
  w.absent = absent;
  const unsigned grid = table_grid(w.m, (u64)(64u >> w.gshift) * kRowsInFlight, dev);
  const bool nt = hook_table_put_nt(kTablePutNt);
  if (p16)
    nt ? k_table_write<P, true><<<grid, kBlock, 0, st>>>(w) : k_table_write<P, false><<<grid, kBlock, 0, st>>>(w);
  else
    nt ? k_table_write<P / 2, true><<<grid, kBlock, 0, st>>>(w) : k_table_write<P / 2, false><<<grid, kBlock, 0, st>>>(w);
}

// The get's piece rule for the replies of an insert-if-absent or a reduce: two words a lane where they allow it
static bool replies_w2(size_t rowbytes, const void *replies, size_t reply_stride) {
  return replies && (((uintptr_t)replies | reply_stride) & 15) == 0 && ((rowbytes / 8 + 1) & 1) == 0;
}

// "k_table_add_reply<W>": k_table_get<W> on the slots a call's first kernel left in its workspace.  Behind
// the call's last writing kernel no kernel writes a row: plain loads.
template <int W = 2>
static void launch_table_reply(const TableGeom &t, const u32 *slots, size_t m, void *replies, size_t reply_stride,
                               bool w2, int dev, hipStream_t st) {
  const u32 nw = (u32)(t.rowbytes / 8) + 1;
  GetArgs r{};
  r.t = t;
  r.slots = slots;
  r.m = m;
  r.replies = static_cast<uint8_t *>(replies);
  r.reply_stride = reply_stride;
  r.np = w2 ? nw / 2 : nw;
  r.gshift = group_shift(r.np);
  const unsigned grid = table_grid(m, 64u >> r.gshift, dev);
  const bool nt = hook_table_reply_nt(kTableReplyNt);
  if (w2)
    nt ? k_table_get<W, true, true><<<grid, kBlock, 0, st>>>(r) : k_table_get<W, false, true><<<grid, kBlock, 0, st>>>(r);
  else
    nt ? k_table_get<W / 2, true, true><<<grid, kBlock, 0, st>>>(r)
       : k_table_get<W / 2, false, true><<<grid, kBlock, 0, st>>>(r);
}

}  // namespace pdht
