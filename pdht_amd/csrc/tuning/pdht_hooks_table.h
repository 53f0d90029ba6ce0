// tuning/pdht_hooks_table.h -- the TUNING build's alternative to the table
// export of pdht_table_iter.hip (product/pdht_hooks_table.h takes none).
//
// 343: the write pass learns liveness from the 64-bit ballot masks that the
// count pass saved in the workspace (1 bit per slot) instead of reading the
// tags again (8 B per slot); only the tags of live slots are fetched, for
// their mbits.  Every workspace of this build reserves the masks behind the
// tile words: 8 B per 64 slots.
#pragma once

namespace pdht {

static inline size_t export_masks_at(u64 ntiles) { return (size_t)((ntiles * 4 + 15) & ~15ull); }

static inline size_t hook_table_export_workspace(size_t bytes, u64 nslots) {
  const u64 ntiles = (nslots + kExportTile - 1) / kExportTile;
  return bytes ? export_masks_at(ntiles) + (size_t)ntiles * (kExportTile / 64) * 8 : 0;
}

__device__ __forceinline__ u64 *export_masks(const ExportArgs &a, u64 tile) {
  uint8_t *ws = reinterpret_cast<uint8_t *>(a.tiles);
  return reinterpret_cast<u64 *>(ws + ((a.ntiles * 4 + 15) & ~15ull)) + tile * (kExportTile / 64) +
         (threadIdx.x >> 6) * kExportPerLane;
}

__global__ __launch_bounds__(kBlock) void k_table_export_count_masks(const ExportArgs a) {
  __shared__ u32 s_n[2][kWavesPerBlock];
  u32 par = 0;
  for (u64 tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x, par ^= 1) {
    u64 tag[kExportPerLane], slot[kExportPerLane], live[kExportPerLane];
    const u32 n = export_tile_tags(a, tile, tag, slot, live);
    const u32 lane = threadIdx.x & 63;
    if (lane < (u32)kExportPerLane) {
      u64 mine = 0;
#pragma unroll
      for (int k = 0; k < kExportPerLane; ++k) mine = lane == (u32)k ? live[k] : mine;
      export_masks(a, tile)[lane] = mine;
    }
    if (lane == 0) s_n[par][threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
      u32 sum = 0;
#pragma unroll
      for (int w = 0; w < kWavesPerBlock; ++w) sum += s_n[par][w];
      a.tiles[tile] = sum;
    }
  }
}

template <int P, bool NT>
__global__ __launch_bounds__(kBlock) void k_table_export_write_masks(const ExportArgs a) {
  __shared__ u32 s_n[kWavesPerBlock];
  __shared__ u32 s_slot[kExportTile];
  __shared__ u64 s_mb[kExportTile];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (u64 tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    u64 tag[kExportPerLane], slot[kExportPerLane], live[kExportPerLane];
    const u64 *masks = export_masks(a, tile);
    const u64 rel0 = tile * kExportTile + (u64)wave * (64 * kExportPerLane) + lane;
    u32 mine = 0;
#pragma unroll
    for (int k = 0; k < kExportPerLane; ++k) {
      live[k] = masks[k];
      const u64 rel = rel0 + (u64)k * 64;
      slot[k] = a.first + (rel < a.nslots ? rel : a.nslots - 1);
      tag[k] = (live[k] >> lane) & 1 ? a.tags[slot[k]] : 0;  // the mbits of the live slots only
      mine += (u32)__popcll(live[k]);
    }
    export_write_tile<P, NT>(a, tile, tag, slot, live, mine, s_n, s_slot, s_mb);
  }
}

static inline int hook_table_export(const ExportArgs &a, unsigned grid, bool p16, bool nt, hipStream_t st) {
  if (tuning_variant() != 343) return kNoVariant;
  k_table_export_count_masks<<<grid, kBlock, 0, st>>>(a);
  HIP_TRY(hipGetLastError());
  k_table_export_scan<<<1, kExportScanBlock, 0, st>>>(a);
  HIP_TRY(hipGetLastError());
  if (!a.max_entries) return 0;
  if (p16)
    nt ? k_table_export_write_masks<16, true><<<grid, kBlock, 0, st>>>(a)
       : k_table_export_write_masks<16, false><<<grid, kBlock, 0, st>>>(a);
  else
    nt ? k_table_export_write_masks<8, true><<<grid, kBlock, 0, st>>>(a)
       : k_table_export_write_masks<8, false><<<grid, kBlock, 0, st>>>(a);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace pdht
