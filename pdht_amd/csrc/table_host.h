// table_host.h -- host-side geometry of the device-resident target table, shared by its translation
// units (pdht_table.hip: put, get, resolve; pdht_table_rmw.hip: update, compare-and-swap;
// pdht_table_iter.hip: export): the geometry checks, the layout of the caller's buffer as pointers, and
// the launch arithmetic of the lane-group kernels.
#pragma once
#include "table_geom.h"

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

}  // namespace pdht
