// table_geom.h -- the geometry of the device-resident target table (layout: table.h) as
// its kernels receive it: shared by table.h (put, get, resolve) and table_iter.h (export).
#pragma once
#include "rows.h"

namespace pdht {

constexpr u64 kTableMix = 0x9E3779B97F4A7C15ull;  // 2^64 / golden ratio
constexpr u32 kTableNoSlot = 0xFFFFFFFFu;         // workspace mark of a dropped record
constexpr size_t kTableTagsAt = 64;

struct TableGeom {
  u64 *counters;
  u64 *tags;
  u64 *win;
  uint8_t *rows;
  u64 mask;   // C - 1
  u32 shift;  // 64 - log2 C
  u32 cap;    // C (<= 2^31): the private slot's index
  u64 rowbytes;
};

}  // namespace pdht
