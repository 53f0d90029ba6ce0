// table_iter.h -- the target table's entries in slot order (include/pdht_hip_table_iter.h): a stable
// stream compaction of the live slots of a slot range, the batch form of the owner's walk
// (pdht_iterate / pdht_getnext, libpdht/iter.c:24-91).
//
// The range is cut into tiles of kExportTile consecutive slots, counted from first_slot.  Three
// kernels, the kernel boundaries their only synchronisation (no ticket, no look-back, no polling:
// nothing waits on another wave, and the order of the output does not depend on the schedule):
//   k_table_export_count  persistent grid, a workgroup per tile: each wave reads 4 x 64 tags coalesced,
//                         8 B per lane, and counts the live ones by ballot and popcount; the tile's
//                         count -> workspace (u32 per tile).
//   k_table_export_scan   one workgroup: the exclusive scan of the tile counts in place (they become the
//                         tile bases) and count2.
//   k_table_export_write  persistent grid, a workgroup per tile: reads the tags again, ranks each live slot
//                         as tile base + ballot prefix, compacts slot index and mbits into LDS, stores them
//                         from there in entry order (contiguous), then copies the rows in the shape of
//                         k_rows / k_table_write: a lane group per entry works from the compacted slot list,
//                         kRowsInFlight rows loaded without a branch (clamped) ahead of the predicated stores,
//                         rows of more than 64 pieces swept by the whole wave.
// Ranks and slot indices are <= 2^31 and kept in 32 bits; every byte offset is a 64-bit product.
#pragma once
#include "table_geom.h"

namespace pdht {

constexpr u32 kExportTile = 1024;     // slots per tile: kBlock lanes x kExportPerLane
constexpr int kExportPerLane = 4;     // tags a lane has in flight; a wave owns 4 x 64 consecutive slots
constexpr int kExportScanBlock = 1024;
static_assert(kExportTile == (u32)kBlock * kExportPerLane, "a tile is one load round of a workgroup");

struct ExportArgs {
  const u64 *tags;
  const uint8_t *rows;
  u64 rowbytes;
  u64 first;   // first slot of the range
  u64 nslots;  // slots of the range (>= 1)
  u64 ntiles;
  u32 cap;     // the private slot's index: its mbits is 0
  u32 *tiles;  // workspace: the tiles' counts, then (after the scan) their bases
  u64 *count2;
  u64 max_entries;
  uint8_t *mbits_out;
  u64 mbits_stride;
  uint8_t *rows_out;  // may be null
  u64 row_stride;
  uint8_t *slot_out;  // may be null
  u64 slot_stride;
  u32 np;      // pieces of a row
  u32 gshift;  // log2 of the lane group (G = the power of two >= np, at most 64)
};

// The tags of this lane's kExportPerLane slots of tile `tile` (0 = not live for slots past the range:
// those lanes read the range's last slot), their ballots, and the wave's live count.
__device__ __forceinline__ u32 export_tile_tags(const ExportArgs &a, u64 tile, u64 (&tag)[kExportPerLane],
                                                u64 (&slot)[kExportPerLane], u64 (&live)[kExportPerLane]) {
  const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const u64 rel0 = tile * kExportTile + (u64)wave * (64 * kExportPerLane) + lane;
#pragma unroll
  for (int k = 0; k < kExportPerLane; ++k) {
    const u64 rel = rel0 + (u64)k * 64;
    slot[k] = a.first + (rel < a.nslots ? rel : a.nslots - 1);
    tag[k] = a.tags[slot[k]];
  }
  u32 n = 0;
#pragma unroll
  for (int k = 0; k < kExportPerLane; ++k) {
    live[k] = __ballot(tag[k] != 0 && rel0 + (u64)k * 64 < a.nslots);
    n += (u32)__popcll(live[k]);
  }
  return n;
}

__global__ __launch_bounds__(kBlock) void k_table_export_count(const ExportArgs a) {
  __shared__ u32 s_n[2][kWavesPerBlock];  // by round parity: one barrier per tile
  u32 par = 0;
  for (u64 tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x, par ^= 1) {
    u64 tag[kExportPerLane], slot[kExportPerLane], live[kExportPerLane];
    const u32 n = export_tile_tags(a, tile, tag, slot, live);
    if ((threadIdx.x & 63) == 0) s_n[par][threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
      u32 sum = 0;
#pragma unroll
      for (int w = 0; w < kWavesPerBlock; ++w) sum += s_n[par][w];
      a.tiles[tile] = sum;
    }
  }
}

// One workgroup of kExportScanBlock lanes walks the tile counts in rounds of kExportScanBlock: a shuffle
// scan inside each wave, the wave totals through LDS, the running total carried in a register.
__global__ __launch_bounds__(kExportScanBlock) void k_table_export_scan(const ExportArgs a) {
  constexpr int kWaves = kExportScanBlock / 64;
  __shared__ u32 s_w[2][kWaves];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 carry = 0;
  u32 par = 0;
  for (u64 t0 = 0; t0 < a.ntiles; t0 += kExportScanBlock, par ^= 1) {
    const u64 t = t0 + threadIdx.x;
    const u32 c = t < a.ntiles ? a.tiles[t] : 0;
    u32 inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const u32 up = __shfl_up(inc, o);
      if (lane >= (u32)o) inc += up;
    }
    if (lane == 63) s_w[par][wave] = inc;
    __syncthreads();
    u32 before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const u32 v = s_w[par][w];
      before += (u32)w < wave ? v : 0;
      all += v;
    }
    if (t < a.ntiles) a.tiles[t] = (u32)(carry + before + inc - c);
    carry += all;
  }
  if (threadIdx.x == 0) {
    a.count2[0] = carry;
    a.count2[1] = carry < a.max_entries ? carry : a.max_entries;
  }
}

// One tile of the write pass, from the tags, slots and ballots of export_tile_tags on: ranks, the compacted
// lists in LDS (s_n: kWavesPerBlock words, s_slot / s_mb: kExportTile entries), the stores.  Ends with
// the barrier behind which the lists may be rewritten.  P: 16 or 8 bytes per piece of a row.  NT:
// non-temporal stores of the outputs (A/B only: the product stores plain).
template <int P, bool NT>
__device__ __forceinline__ void export_write_tile(const ExportArgs &a, u64 tile, const u64 (&tag)[kExportPerLane],
                                                  const u64 (&slot)[kExportPerLane],
                                                  const u64 (&live)[kExportPerLane], u32 mine, u32 *s_n,
                                                  u32 *s_slot, u64 *s_mb) {
  typedef typename RowPiece<P>::type T;
  constexpr int R = kRowsInFlight;
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u32 l = lane & ((1u << a.gshift) - 1), g = lane >> a.gshift, rpi = 64u >> a.gshift;
  const u64 lo = (u64)(l < a.np ? l : 0) * P;
  const u64 base = a.tiles[tile];  // entries ahead of this tile
  if (lane == 0) s_n[wave] = mine;
  __syncthreads();
  u32 rank = 0, n = 0;  // live slots of the tile ahead of this wave / in the tile
#pragma unroll
  for (int w = 0; w < kWavesPerBlock; ++w) {
    const u32 v = s_n[w];
    rank += (u32)w < wave ? v : 0;
    n += v;
  }
#pragma unroll
  for (int k = 0; k < kExportPerLane; ++k) {
    if ((live[k] >> lane) & 1) {
      const u32 r = rank + (u32)__popcll(live[k] & ((1ull << lane) - 1));
      s_slot[r] = (u32)slot[k];
      s_mb[r] = slot[k] == a.cap ? 0 : tag[k];
    }
    rank += (u32)__popcll(live[k]);
  }
  __syncthreads();
  // entries of this tile below max_entries (uniform over the workgroup)
  const u32 nw = base >= a.max_entries ? 0 : (u32)(a.max_entries - base < n ? a.max_entries - base : n);
  for (u32 e = threadIdx.x; e < nw; e += kBlock) {
    st<NT>(s_mb[e], reinterpret_cast<u64 *>(a.mbits_out + (base + e) * a.mbits_stride));
    if (a.slot_out) st<NT>(s_slot[e], reinterpret_cast<u32 *>(a.slot_out + (base + e) * a.slot_stride));
  }
  if (a.rows_out && nw) {
    const u32 step = rpi * R, last = nw - 1;
    for (u32 e0 = wave * step; e0 < nw; e0 += kWavesPerBlock * step) {
      u32 ent[R], from[R];
      T v[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        ent[r] = e0 + (u32)r * rpi + g;
        from[r] = s_slot[ent[r] < last ? ent[r] : last];
      }
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = *reinterpret_cast<const T *>(a.rows + (u64)from[r] * a.rowbytes + lo);
#pragma unroll
      for (int r = 0; r < R; ++r) rows_keep(v[r]);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (ent[r] >= nw) continue;
        uint8_t *d = a.rows_out + (base + ent[r]) * a.row_stride;
        if (l < a.np) st<NT>(v[r], reinterpret_cast<T *>(d + lo));
        const uint8_t *s = a.rows + (u64)from[r] * a.rowbytes;  // rows of more pieces than a wave has lanes
        for (u32 c = l + 64; c < a.np; c += 64)
          st<NT>(*reinterpret_cast<const T *>(s + (u64)c * P), reinterpret_cast<T *>(d + (u64)c * P));
      }
    }
  }
  __syncthreads();  // the lists are rewritten in the next round
}

template <int P, bool NT>
__global__ __launch_bounds__(kBlock) void k_table_export_write(const ExportArgs a) {
  __shared__ u32 s_n[kWavesPerBlock];
  __shared__ u32 s_slot[kExportTile];
  __shared__ u64 s_mb[kExportTile];
  for (u64 tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    u64 tag[kExportPerLane], slot[kExportPerLane], live[kExportPerLane];
    const u32 mine = export_tile_tags(a, tile, tag, slot, live);
    export_write_tile<P, NT>(a, tile, tag, slot, live, mine, s_n, s_slot, s_mb);
  }
}

}  // namespace pdht
