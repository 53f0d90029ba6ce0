// pdht_bucket.hip -- destination bucketing (include/pdht_hip.h
// pdht_bucket_batch_dev / pdht_bucket_records_dev, include/pdht_hip_put.h
// pdht_bucket_put_records_dev; kernels in bucket.h, the value mover in rows.h).
#include "bucket.h"
#include "rows.h"
#include "runtime.h"

// ------------------------------------------------- destination bucketing ---
#ifndef PDHT_TP_EVEN_SEG  // compile-time A/B only
#define PDHT_TP_EVEN_SEG 1
#endif
namespace pdht {
struct BucketWs {
  u32 *counts, *chunks;
  u64 *totals, *base;
  u32 *tickets;  // [8] per-XCD tile tickets of the dynamic scatter
  // the two-pass region (8/16/32-B keys from two_pass_min_ranks()): the
  // tile-local sort's per-tile f-run starts, per-chunk rank histograms, key
  // rows and their u16 indices inside the tile
  uint8_t *region;
  uint16_t *tl_starts, *tl_lidx;
  u32 *tl_chunkcnt;
  uint8_t *tl_keys;
  size_t bytes;
};
static size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }
static bool two_pass_keysize(size_t keysize) { return keysize == 8 || keysize == 16 || keysize == 32; }
// Two-pass bucketing from this many ranks up.  The one-pass staged scatter
// wins while its owner-table shapes fit (staged_shape): arrays of 8/16-B keys
// on 8 x 16 tiles up to 1574 ranks, 16-B records on 4 x 16 tiles up to 1462,
// 8-B records (ballots) up to 2047, 32-B arrays to 2048; 32-B records take
// two passes from 256 ranks (below not measured).  Measured in r06 with these
// shapes and grids: profiles/r06/ab/bucket_two_pass_thresholds.log, EXPERIMENTS.md §R6.
constexpr u32 two_pass_min_ranks(size_t keysize, bool records) {
  if (records) return keysize == 8 ? 2048 : keysize == 16 ? 1463 : 256;
  return keysize == 32 ? 2049 : 1575;
}
// Tile-local two-pass sort (r06, bucket.h k_bucket_tl_*): pass-1 tiles of 4096 keys for 8-B keys, 2048 for 16/32-B
// keys (8 waves x 4 keys per lane, spill-free; 16-B keys in 4096-key tiles spilled 23 VGPRs and ran 0.4-1.9 %
// slower, profiles/r06/ab/bucket_16_tl_pass1_tiles.log), one sub-tile each; count-chunks of ct tiles, ct the
// largest power of two <= 8 that still leaves >= 512 chunks (two pass-1 workgroups on each of 256 CUs), so that a
// chunk's histogram never counts past 32768 keys (u16 halves in LDS).  Both depend on n only, so the workspace
// size does too.
static u32 tl_tile_shift(size_t keysize) { return hook_tl_tile_shift(keysize == 8 ? 12 : 11, keysize); }
static u32 tl_chunk_tiles(u64 ntiles, u32 tshift) {
  u32 ct = std::min<u32>(8, 32768u >> tshift);
  while (ct > 1 && ntiles / ct < 512) ct >>= 1;
  return ct;
}
// Workgroups per CU that a workgroup's total (dynamic + fixed) LDS allows, of
// gfx950's 160 KiB per CU (the allocation granule is unmeasured)
constexpr size_t kLdsPerCu = 160 * 1024;
constexpr int lds_wgs_per_cu(size_t total) { return total <= 53 * 1024 ? 3 : total <= 80 * 1024 ? 2 : 1; }
// Before kernel Fn launches with `lds`; first use in the process: its static LDS is within the fixed bytes
template <auto Fn>
static int set_lds(LdsBytes lds) {
  static const std::pair<hipError_t, size_t> fixed = [] {
    hipFuncAttributes at{};
    const hipError_t e = hipFuncGetAttributes(&at, reinterpret_cast<const void *>(Fn));
    return std::make_pair(e, at.sharedSizeBytes);
  }();
  HIP_TRY(fixed.first);
  if (fixed.second > lds.fixed) {  // (__PRETTY_FUNCTION__ names the kernel instantiation Fn)
    snprintf(g_err, sizeof g_err, "%s: %zu B of static LDS, its launch counts %zu", __PRETTY_FUNCTION__,
             fixed.second, lds.fixed);
    return PDHT_HIP_ERROR;
  }
  if (lds.dyn > 65536)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(Fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds.dyn));
  return 0;
}
// f(the packed key size 8 / 16 / 32 as a constant); PDHT_KEY_TAG: the kernel tag "stem<8B...>" of key size L
// (a file-scope macro on purpose: the hook headers included below, bucket_two_pass_r05.h, use it too)
template <class F>
static int with_keysize(size_t keysize, F &&f) {
  using std::integral_constant;
  return keysize == 8 ? f(integral_constant<int, 8>{}) : keysize == 16 ? f(integral_constant<int, 16>{})
                                                                       : f(integral_constant<int, 32>{});
}
#define PDHT_KEY_TAG(L, stem, x) ((L) == 8 ? stem "<8B" x ">" : (L) == 16 ? stem "<16B" x ">" : stem "<32B" x ">")

struct BucketArgs {
  const uint8_t *k;
  u64 n;
  FastMod rk;
  u32 nranks, nbits;
  TileStarts ts;
  u64 ntiles;
};

template <int L, class Out, bool PACK = false, int W = kStW, int KPL = kStKPL, bool DYN = false, int OB = 0,
          bool NTK = false>
static int launch_staged(const BucketArgs &a, const Out &out, hipStream_t st, int dev, u32 *tickets = nullptr) {
  g_kernel = OB && W == 8 ? PDHT_KEY_TAG(L, "k_bucket_scatter_staged", ",own,8x16")
             : OB         ? PDHT_KEY_TAG(L, "k_bucket_scatter_staged", ",own")
             : PACK       ? PDHT_KEY_TAG(L, "k_bucket_scatter_staged", ",u16")
                          : PDHT_KEY_TAG(L, "k_bucket_scatter_staged", "");
  const LdsBytes lds = staged_lds<W, KPL, PACK, OB>(a.nranks);
  constexpr auto fn = &k_bucket_scatter_staged<L, Out, W, KPL, PACK, DYN, OB, NTK>;
  if (int rc = set_lds<fn>(lds)) return rc;
  const int per_cu = lds_wgs_per_cu(lds.total());
  unsigned g = (unsigned)std::min<u64>(a.ntiles, (u64)std::max(1, g_dev[dev].cus) * per_cu);
  if (g >= 8) g &= ~7u;  // a multiple of 8: XCD-contiguous tile order (TileOrder)
  // (DYN: 8 XCD groups need a grid that is a multiple of 8; small grids use
  // the static order)
  if (DYN && g % 8 == 0)
    fn<<<g, W * 64, lds.dyn, st>>>(a.k, a.n, a.rk, a.nranks, a.nbits, a.ts, a.ntiles, out, tickets);
  else
    k_bucket_scatter_staged<L, Out, W, KPL, PACK, false, OB, NTK>
        <<<g, W * 64, lds.dyn, st>>>(a.k, a.n, a.rk, a.nranks, a.nbits, a.ts, a.ntiles, out, nullptr);
  return 0;
}

template <int W, class Out>
static int launch_wg(const BucketArgs &a, const Out &out, u32 L, hipStream_t st, int dev) {
  g_kernel = W == 8 ? "k_bucket_scatter_wg<8>" : "k_bucket_scatter_wg<4>";
  const size_t bytes = (size_t)W * a.nranks * 4;  // (no static LDS)
  if (int rc = set_lds<&k_bucket_scatter_wg<W, Out>>(LdsBytes{bytes, 0})) return rc;
  k_bucket_scatter_wg<W, Out><<<grid_for(a.ntiles, 4, dev), W * 64, bytes, st>>>(
      a.k, L, a.n, a.rk, a.nranks, a.nbits, a.ts, a.ntiles, out);
  return 0;
}

// The tile-local two-pass sort (bucket.h k_bucket_tl_*): pass 1 (sorts
// each tile by f in place, counts ranks per chunk), the rank scan down the
// chunks (and in-block prefixes of the rank totals), pass 2 (forms the bucket
// bases and writes bucket_offsets, gathers the f-runs of each segment, sorts
// by c, stores at the final slots).  Pass 1 in W1 x KPL1 (one tile) @ PER_CU1,
// pass 2 in W x KPL @ PER_CU.
template <int L, class Out, int W, int KPL, int PER_CU, int W1, int KPL1, int PER_CU1, int PROBE = 0,
          bool NTG = (L == 32 && Out::kPair8), bool NTK1 = true, bool ONE = (L == 8 && !Out::kPair8)>
static int launch_tl(const BucketArgs &a, const TwoPassTL &tl, const Out &out, const BucketWs &w,
                     uint64_t *bucket_offsets, hipStream_t st, int dev) {
  if ((1u << tl.tshift) != (u32)(W1 * KPL1 * 64)) return fail("tile-local pass 1: tile/shape mismatch%s", "");
  constexpr int WPE = PER_CU * W / 4 > 8 ? 8 : PER_CU * W / 4;
  constexpr int WPE1 = PER_CU1 * W1 / 4 > 8 ? 8 : PER_CU1 * W1 / 4;
  static_assert(PER_CU1 * tl_pass1_lds<W1, KPL1>(kBucketMaxRanks).total() <= kLdsPerCu, "pass 1: LDS per CU");
  static_assert(PER_CU * tl_pass2_lds<W, KPL>().total() <= kLdsPerCu, "pass 2: LDS per CU");
  const LdsBytes b1 = tl_pass1_lds<W1, KPL1>(a.nranks), b2 = tl_pass2_lds<W, KPL>();
  constexpr auto f1 = &k_bucket_tl_pass1<L, W1, KPL1, WPE1, NTK1>;
  constexpr auto f2 = &k_bucket_tl_pass2<L, Out, W, KPL, WPE, ONE, PROBE, NTG>;
  if (int rc = set_lds<f1>(b1)) return rc;
  if (int rc = set_lds<f2>(b2)) return rc;
  const u64 cus = (u64)std::max(1, g_dev[dev].cus);
  unsigned g1 = (unsigned)std::min<u64>(tl.nchunks, cus * PER_CU1);
  if (g1 >= 8) g1 &= ~7u;  // XCD-contiguous chunk order (TileOrder)
  f1<<<g1, W1 * 64, b1.dyn, st>>>(a.k, a.rk, a.nranks, tl);
  k_bucket_chunkscan_tl<<<(a.nranks + 63) / 64, 64 * kCsWaves, 0, st>>>(tl.chunkcnt, tl.nchunks, a.nranks,
                                                                       w.totals, tl.inpre, tl.bsum);
  unsigned g2 = (unsigned)std::min<u64>(tl.nseg, cus * PER_CU);
  if (g2 >= 8) g2 &= ~7u;
  f2<<<g2, W * 64, b2.dyn, st>>>(a.rk, a.nranks, tl, out);
  g_kernel = PDHT_KEY_TAG(L, "k_bucket_tl_pass2", "");
  return 0;
}

// Tile-local shapes: pass 1 one tile per sub-tile (8 x 8 = 4096 keys; 16/32-B
// keys 8 x 4 = 2048, spill-free) at 2 WG/CU; pass 2 the shapes measured best
// per key size and output kind (r05, re-measured in r06: 16-B keys in 8 x 4 @ 2,
// profiles/r06/ab/bucket_16_tl_pass2_shapes.log)
template <int L, class Out, bool NTG = (L == 32 && Out::kPair8), bool NTK1 = true>
static int launch_tl_product(const BucketArgs &a, const TwoPassTL &tl, const Out &out, const BucketWs &w,
                             uint64_t *bucket_offsets, hipStream_t st, int dev) {
  if constexpr ((L == 32 && !Out::kPair8) || L == 16)
    return launch_tl<L, Out, 8, 4, 2, 8, 4, 2, 0, NTG, NTK1>(a, tl, out, w, bucket_offsets, st, dev);
  else if constexpr (L == 32)
    return launch_tl<L, Out, 4, 4, 4, 8, 4, 2, 0, NTG, NTK1>(a, tl, out, w, bucket_offsets, st, dev);
  else if constexpr (L == 8 && !Out::kPair8)
    return launch_tl<L, Out, 8, 8, 2, 8, 8, 2, 0, NTG, NTK1>(a, tl, out, w, bucket_offsets, st, dev);
  else
    return launch_tl<L, Out, 8, 4, 2, 8, 8, 2, 0, NTG, NTK1>(a, tl, out, w, bucket_offsets, st, dev);
}

// The two digits of rank = c * F + f.  Array outputs of 8/16-B keys take one
// fine bit more than the balanced split (8192 ranks: F = 256, C = 32): pass 2
// writes 24 / 32 B per key in runs of ~4096 / C keys against pass 1's 12 / 20 B
// in runs of ~4096 / F, so longer pass-2 runs pay (-4 to -5.5 %); 32-B keys
// and records lose 1-3 % with it and keep the balanced split (EXPERIMENTS.md
// §4.4, profiles/r03/ab/bucket_two_pass_digits.log; tuning 164, §R6).
struct Digits {
  u32 fbits, F, C, cbits;
};
template <class Out>
static Digits digit_split(u32 nbits, u32 nranks, size_t keysize) {
  Digits d{};
  d.fbits = (nbits + 1) / 2;
  const bool fine_plus = hook_fine_plus(std::is_same<Out, OutSoA>::value && keysize <= 16);
  if (fine_plus && d.fbits + 1 <= std::min<u32>(8, nbits)) ++d.fbits;
  d.F = 1u << d.fbits;
  d.C = (nranks + d.F - 1) >> d.fbits;
  d.cbits = nbits - d.fbits;
  return d;
}

// Pass-2 segments: nsegf per fine bucket, each a run of whole count-chunks
// (chunk = `chunk_keys` keys, ~chunk_keys / F of them in bucket f), split
// evenly.  SG chunks make ~kTpSegKeys keys; when the remainder of
// nchunks / SG leaves at most one extra chunk per segment, take the floor
// (segments of SG or SG + 1 chunks: ~3968 keys at most) rather than the
// ceiling, which costs one more segment per fine bucket.  Only where SG + 1
// chunks stay ~2 sigma under 4096 keys: F = 256 (EXPERIMENTS.md §4.4,
// profiles/r05/ab/bucket_pass2_even_segments.log).  PDHT_TP_EVEN_SEG=0
// (experiment builds): the ceiling.
static void split_segments(u64 nchunks, u64 chunk_keys, u32 F, u64 *SG, u64 *nsegf) {
  *SG = std::max<u64>(1, (u64)F * kTpSegKeys / chunk_keys);
  const u64 nfl = std::max<u64>(1, nchunks / *SG);
  const u64 step = chunk_keys / F;  // keys of one fine bucket per chunk
  const bool floor_ok =
      PDHT_TP_EVEN_SEG && (*SG + 1) * step <= 3968 && nchunks >= nfl * *SG && nchunks - nfl * *SG <= nfl;
  *nsegf = floor_ok ? nfl : (nchunks + *SG - 1) / *SG;
}

enum class BucketKernel { kStaged, kGeneric, kTwoPass };
enum class StagedShape { kBallot4x16 = 0, kOwner4x16 = 1, kOwner8x16 = 2 };  // the indices of kStagedDims

// The one mapping of StagedShape (the index) to the kernel's template arguments; f(index as a constant)
struct StagedDims {
  int W, KPL, OB;
};
constexpr StagedDims kStagedDims[] = {{kStW, kStKPL, 0}, {kStW, kStKPL, 2}, {8, 16, 2}};
template <class F>
constexpr auto with_staged_shape(StagedShape s, F &&f) {
  using std::integral_constant;
  return s == StagedShape::kOwner8x16   ? f(integral_constant<int, (int)StagedShape::kOwner8x16>{})
         : s == StagedShape::kOwner4x16 ? f(integral_constant<int, (int)StagedShape::kOwner4x16>{})
                                        : f(integral_constant<int, (int)StagedShape::kBallot4x16>{});
}
constexpr LdsBytes staged_shape_lds(StagedShape shape, u32 nranks) {
  return with_staged_shape(shape, [&](auto S) {
    constexpr StagedDims d = kStagedDims[decltype(S)::value];
    return staged_lds<d.W, d.KPL, false, d.OB>(nranks);
  });
}
// Staged scatter shape (measurements: DESIGN.md §4.5, EXPERIMENTS.md §4.4):
// ballots below 512 ranks; from there owner-table ranking, on 8 x 16 tiles
// (arrays of 8/16-B keys only) while dynamic + fixed bytes fit the CU's LDS (<= 1574 ranks), else on
// 4 x 16 tiles while the dynamic bytes stay within 80 KiB (<= 1462 ranks, the measured edge); else ballots.
constexpr StagedShape staged_shape(size_t keysize, u32 nranks, bool records) {
  if (nranks < 512) return StagedShape::kBallot4x16;
  if (!records && keysize != 32 && staged_shape_lds(StagedShape::kOwner8x16, nranks).total() <= kLdsPerCu)
    return StagedShape::kOwner8x16;
  if (staged_shape_lds(StagedShape::kOwner4x16, nranks).dyn <= 80 * 1024) return StagedShape::kOwner4x16;
  return StagedShape::kBallot4x16;
}
// Every nranks below the two-pass thresholds has a shape whose LDS fits (r06: at 1575 ranks 8 x 16 did not)
constexpr bool staged_shapes_fit() {
  for (bool records : {false, true})
    for (size_t keysize : {8, 16, 32}) {
      if (two_pass_min_ranks(keysize, records) > kStagedMaxRanks + 1) return false;
      for (u32 nranks = 1; nranks < two_pass_min_ranks(keysize, records); ++nranks)
        if (staged_shape_lds(staged_shape(keysize, nranks, records), nranks).total() > kLdsPerCu) return false;
    }
  return true;
}
static_assert(staged_shapes_fit(), "a staged nranks without a shape that fits the LDS");

// The staged scatter of `shape`, tiles claimed by per-XCD tickets
template <class Out, bool NTK = false>
static int launch_staged_shape(StagedShape shape, size_t keysize, const BucketArgs &a, const Out &out,
                               hipStream_t st, int dev, u32 *tickets) {
  return with_keysize(keysize, [&](auto L) {
    return with_staged_shape(shape, [&](auto S) {
      constexpr StagedDims d = kStagedDims[decltype(S)::value];
      return launch_staged<decltype(L)::value, Out, false, d.W, d.KPL, true, d.OB, NTK>(a, out, st, dev, tickets);
    });
  });
}
}  // namespace pdht

// A/B hook points of the choices below (product/pdht_hooks_bucket.h: none taken)
#include "pdht_hooks_bucket.h"

namespace pdht {
// Sized for the smallest tile any scatter kernel uses, plus the two-pass region when the batch can
// take that path: 8/16/32-B keys from two_pass_min_ranks() up for the output kind (`records`; the
// tuning build forces two passes at any nranks and always reserves it, at least as large as the r02-r05
// form needs: hook_two_pass_region).  16M x 8-B keys at 1024 ranks: 17 MB; from 1575 ranks + 176 MB.
static BucketWs bucket_layout(void *ws, size_t n, size_t keysize, u32 nranks, bool records) {
  const u64 ntiles = (n + kBucketMinTile - 1) / kBucketMinTile;
  const u64 nchunks = (ntiles + kBucketChunk - 1) / kBucketChunk;
  BucketWs w{};
  uint8_t *p = static_cast<uint8_t *>(ws);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    uint8_t *q = p + off;
    off += round256(bytes);
    return q;
  };
  w.counts = reinterpret_cast<u32 *>(take((size_t)nranks * ntiles * 4));
  w.chunks = reinterpret_cast<u32 *>(take((size_t)nranks * nchunks * 4));
  w.totals = reinterpret_cast<u64 *>(take((size_t)nranks * 8));
  w.base = reinterpret_cast<u64 *>(take((size_t)nranks * 8));
  w.tickets = reinterpret_cast<u32 *>(take(256));
  const bool two_pass = hook_bucket_reserve(
      two_pass_keysize(keysize) && nranks >= two_pass_min_ranks(keysize, records), keysize);
  if (two_pass) {
    w.region = p + off;
    const size_t off0 = off;
    const u32 sh = tl_tile_shift(keysize);
    const u64 tl_tiles = (n + (1ull << sh) - 1) >> sh;
    const u64 tl_chunks = (tl_tiles + tl_chunk_tiles(tl_tiles, sh) - 1) / tl_chunk_tiles(tl_tiles, sh);
    w.tl_starts = reinterpret_cast<uint16_t *>(take((size_t)tl_tiles * kTpMaxDigits * 2));
    w.tl_chunkcnt = reinterpret_cast<u32 *>(take((size_t)tl_chunks * nranks * 4));
    w.tl_keys = take(n * keysize);
    w.tl_lidx = reinterpret_cast<uint16_t *>(take(n * 2));
    off = std::max(off, off0 + hook_two_pass_region((size_t)0, n, keysize, nranks));
  }
  w.bytes = off;
  return w;
}

// The tile-local two-pass bucketing (k_bucket_tl_*), n >= 1.
template <class Out>
static int bucket_tl(const BucketArgs &a, const BucketWs &w, size_t keysize, const Out &out,
                     uint64_t *bucket_offsets, hipStream_t st, int dev) {
  const Digits d = digit_split<Out>(a.nbits, a.nranks, keysize);
  if (d.F > kTpMaxDigits || d.C > kTpMaxDigits)  // the kernels' LDS digit tables
    return fail("two-pass digit split: a digit of %s%lld buckets exceeds the LDS tables", "",
                (long long)(d.F > kTpMaxDigits ? d.F : d.C));
  TwoPassTL tl{};
  tl.fbits = d.fbits;
  tl.F = d.F;
  tl.C = d.C;
  tl.cbits = d.cbits;
  tl.tshift = tl_tile_shift(keysize);
  tl.n = a.n;
  tl.ntiles = (a.n + (1ull << tl.tshift) - 1) >> tl.tshift;
  tl.ct = tl_chunk_tiles(tl.ntiles, tl.tshift);
  tl.nchunks = (tl.ntiles + tl.ct - 1) / tl.ct;
  u64 SG = 0;
  split_segments(tl.nchunks, (u64)tl.ct << tl.tshift, tl.F, &SG, &tl.nsegf);
  // a segment's f-runs (one per tile) must fit pass 2's run table
  const u64 seg_tiles = (tl.nchunks + tl.nsegf - 1) / tl.nsegf * tl.ct;
  if (seg_tiles > kTlMaxRuns)
    return fail("tile-local two-pass: %s%lld tiles per segment exceed the run table", "", (long long)seg_tiles);
  tl.og = 1;
  tl.os = (u32)tl.nsegf;
  hook_tl_order(tl.F, tl.nsegf, &tl.og, &tl.os);
  tl.og = std::min(tl.og, tl.F);  // (powers of two: og divides F)
  tl.os = std::max(tl.os, 1u);
  tl.nsgg = (u32)((tl.nsegf + tl.os - 1) / tl.os);
  tl.nseg = (u64)tl.F * tl.nsgg * tl.os;
  tl.startsF = w.tl_starts;
  tl.chunkcnt = w.tl_chunkcnt;
  tl.inpre = reinterpret_cast<u32 *>(w.base);  // (nranks x u64 of space, unused here: 2 x nranks u32)
  tl.bsum = reinterpret_cast<u32 *>(w.base) + a.nranks;
  tl.offsets = bucket_offsets;
  tl.ikeys = w.tl_keys;
  tl.ilidx = w.tl_lidx;
  return with_keysize(keysize, [&](auto L) {
    if (int rc = hook_tl_shape<L, Out>(a, tl, out, w, bucket_offsets, st, dev); rc != kNoVariant) return rc;
    return launch_tl_product<L, Out>(a, tl, out, w, bucket_offsets, st, dev);
  });
}

// Shared by pdht_bucket_batch_dev (OutSoA) and pdht_bucket_records_dev (OutRec): the two passes
// (bucket_tl), or the counting pass, scans, bucket bases and the scatter into `out`.  out_al: alignment
// bits of the output key rows (0 when they are 8-B aligned 8-B pieces, as in records).
template <class Out>
static int bucket_impl(const void *keys, size_t keysize, size_t n, uint32_t nranks, void *workspace,
                       size_t workspace_bytes, const Out &out, uintptr_t out_al, uint64_t *bucket_offsets,
                       hipStream_t st) {
  if (nranks == 0) return fail("nranks must be > 0%s", "");
  if (nranks > kBucketMaxRanks) return fail("bucketing supports up to 8192 ranks%s", "");
  if (n >= (1ull << 32)) return fail("bucketing: n must be < 2^32 per call%s", "");
  if (!bucket_offsets) return fail("bucket_offsets must not be NULL%s", "");
  if ((uintptr_t)bucket_offsets & 7) return fail("bucket_offsets must be 8-byte aligned%s", "");
  // the workspace's pieces start at multiples of 256 B from its base: u32 counters, u64 totals, the tickets'
  // atomics, and the two-pass key rows, which load_key_regs reads as 16-B vectors (the widest access to it)
  if ((uintptr_t)workspace & 15) return fail("workspace must be 16-byte aligned%s", "");
  if (n && (!keys || keysize == 0)) return fail("null keys or zero keysize%s", "");
  const BucketWs w = bucket_layout(workspace, n, keysize, nranks, Out::kPair8);
  if (!workspace || workspace_bytes < w.bytes) return fail("workspace too small%s", "");
  int dev;
  if (int rc = current_device(&dev)) return rc;
  // Kernel choice: packed 8/16/32-B keys (aligned) -> LDS-staged scatter below
  // the two-pass threshold, two passes from it; other lengths -> generic.
  const uintptr_t al = (uintptr_t)keys | out_al;
  const bool fixed = (keysize == 8 && (al & 7) == 0) || ((keysize == 16 || keysize == 32) && (al & 15) == 0);
  const BucketKernel kind = hook_bucket_kind(
      !fixed                                                 ? BucketKernel::kGeneric
      : nranks >= two_pass_min_ranks(keysize, Out::kPair8) ? BucketKernel::kTwoPass
                                                             : BucketKernel::kStaged,
      fixed, nranks);
  BucketArgs a{};
  a.k = static_cast<const uint8_t *>(keys);
  a.n = n;
  a.rk = make_fastmod(nranks);
  a.nranks = nranks;
  while ((1u << a.nbits) < nranks) ++a.nbits;
  const size_t hist_lds = (size_t)nranks * 4;
  // Two passes, tile-local, no counting pass ahead (A/B build: the r02-r05 form under 290, 202, 264-272)
  if (kind == BucketKernel::kTwoPass) {
    if (int rc = hook_two_pass_r05(a, w, keysize, out, bucket_offsets, st, dev); rc != kNoVariant) {
      if (rc) return rc;
    } else if (n == 0) {  // (no totals: k_bucket_base reads them as zeros)
      k_bucket_base<<<1, kBaseThreads, 0, st>>>(nullptr, nranks, w.base, bucket_offsets, nullptr);
      g_kernel = "k_bucket_base";
    } else if (int rc = bucket_tl(a, w, keysize, out, bucket_offsets, st, dev)) {
      return rc;
    }
    HIP_TRY(hipGetLastError());
    return 0;
  }
  const StagedShape shape = hook_staged_shape(staged_shape(keysize, nranks, Out::kPair8));
  const u64 st_tile = (u64)kStagedDims[(int)shape].W * kStagedDims[(int)shape].KPL * 64;
  const int waves = nranks <= 4096 ? 8 : 4;  // generic: W x nranks x 4 B of LDS <= 128 KiB
  const u64 tile = kind == BucketKernel::kStaged ? st_tile : (u64)waves * kScatKPL * 64;
  const u64 ntiles = (n + tile - 1) / tile;
  const u64 nchunks = (ntiles + kBucketChunk - 1) / kBucketChunk;
  a.ts = TileStarts{w.counts, w.chunks, w.base, nranks};
  a.ntiles = ntiles;
  if (ntiles) {
    const unsigned gc = grid_for(ntiles, 8, dev);
    if (fixed)
      with_keysize(keysize, [&](auto L) {
        k_bucket_count_reg<L><<<gc, kBlock, hist_lds, st>>>(a.k, n, a.rk, nranks, w.counts, ntiles, tile);
        return 0;
      });
    else
      k_bucket_count<<<gc, kBlock, hist_lds, st>>>(a.k, (u32)keysize, n, a.rk, nranks, w.counts, ntiles, tile);
    k_bucket_colscan<<<dim3((nranks + 63) / 64, (unsigned)nchunks), 64, 0, st>>>(w.counts, ntiles, nranks, w.chunks);
    k_bucket_chunkscan<<<(nranks + 63) / 64, 64 * kCsWaves, 0, st>>>(w.chunks, nchunks, nranks, w.totals);
  }
  k_bucket_base<<<1, kBaseThreads, 0, st>>>(ntiles ? w.totals : nullptr, nranks, w.base, bucket_offsets, w.tickets);
  g_kernel = "k_bucket_base";
  if (ntiles) {
    int rc = hook_staged_launch(kind == BucketKernel::kStaged, keysize, a, out, st, dev, shape, w.tickets);
    if (rc != kNoVariant) {
      // an A/B alternative ran
    } else if (kind == BucketKernel::kStaged)
      rc = launch_staged_shape(shape, keysize, a, out, st, dev, w.tickets);
    else
      rc = waves == 8 ? launch_wg<8>(a, out, (u32)keysize, st, dev) : launch_wg<4>(a, out, (u32)keysize, st, dev);
    if (rc) return rc;
  }
  HIP_TRY(hipGetLastError());
  return 0;
}
}  // namespace pdht

using namespace pdht;

// Workspace sizes: array outputs (pdht_bucket_batch_dev) and wire records
// (pdht_bucket_records_dev) switch to the two-pass sort at different rank
// counts (two_pass_min_ranks), so each has its own query.  The records one is larger for 16-B
// keys at 1463-1574 ranks and 32-B keys at 256-2048, and smaller for 8-B keys at 1575-2047.
PDHT_API size_t pdht_bucket_workspace_bytes(size_t n, size_t keysize, uint32_t nranks) {
  return bucket_layout(nullptr, n, keysize, nranks, false).bytes;
}
PDHT_API size_t pdht_bucket_records_workspace_bytes(size_t n, size_t keysize, uint32_t nranks) {
  return bucket_layout(nullptr, n, keysize, nranks, true).bytes;
}

PDHT_API int pdht_bucket_batch_dev(const void *keys, size_t keysize, size_t n, uint32_t nptes,
                                   uint32_t nranks, void *workspace, size_t workspace_bytes,
                                   void *keys_out, uint64_t *mbits_out, uint32_t *ptindex_out,
                                   uint32_t *index_out, uint64_t *bucket_offsets,
                                   pdht_hip_stream_t s) {
  if (int rc = check_place(n, mbits_out, nptes, nranks, nullptr, 0)) return rc;
  if ((uintptr_t)mbits_out & 7) return fail("mbits_out must be 8-byte aligned%s", "");
  if ((uintptr_t)ptindex_out & 3) return fail("ptindex_out must be 4-byte aligned%s", "");
  if ((uintptr_t)index_out & 3) return fail("index_out must be 4-byte aligned%s", "");
  const OutSoA out{static_cast<uint8_t *>(keys_out), mbits_out, ptindex_out, index_out, make_fastmod(nptes),
                   (u32)keysize};
  return bucket_impl(keys, keysize, n, nranks, workspace, workspace_bytes, out, (uintptr_t)keys_out,
                     bucket_offsets, ST(s));
}

PDHT_API size_t pdht_bucket_record_bytes(size_t keysize) { return 24 + ((keysize + 7) & ~(size_t)7); }

// Header, index, mbits and key of every record, `stride` bytes apart (the kernels write nothing past the key,
// except the generic-length one, which zero-fills up to the stride: OutRecT::key_copy)
static int bucket_records_impl(const void *keys, size_t keysize, size_t n, uint32_t nranks, uint32_t msg_type,
                               uint32_t src_rank, uint32_t ht_index, void *workspace, size_t workspace_bytes,
                               void *records, size_t stride, uint64_t *bucket_offsets, hipStream_t st) {
  if (n && !records) return fail("records must not be NULL%s", "");
  if ((uintptr_t)records & 7) return fail("records must be 8-byte aligned%s", "");
  const OutRec out{static_cast<uint8_t *>(records), (u64)stride, (u64)msg_type | ((u64)src_rank << 32), ht_index,
                   (u32)keysize};
  if (int rc = hook_records(out, [&](const auto &o2) {
        return bucket_impl(keys, keysize, n, nranks, workspace, workspace_bytes, o2, 0, bucket_offsets, st);
      });
      rc != kNoVariant)
    return rc;
  return bucket_impl(keys, keysize, n, nranks, workspace, workspace_bytes, out, 0, bucket_offsets, st);
}

PDHT_API int pdht_bucket_records_dev(const void *keys, size_t keysize, size_t n, uint32_t nranks,
                                     uint32_t msg_type, uint32_t src_rank, uint32_t ht_index,
                                     void *workspace, size_t workspace_bytes, void *records,
                                     uint64_t *bucket_offsets, pdht_hip_stream_t s) {
  return bucket_records_impl(keys, keysize, n, nranks, msg_type, src_rank, ht_index, workspace, workspace_bytes,
                             records, pdht_bucket_record_bytes(keysize), bucket_offsets, ST(s));
}

// Put records (include/pdht_hip_put.h): the bucketing kernels write header, index, mbits and key into records of
// the put stride; the row mover (rows.h) then reads each record's source index at +12 and writes, as one run
// per record from the end of the key, the zeros of the key-slot gap, value[index] and its zero pad to 8.
PDHT_API size_t pdht_bucket_put_record_bytes(size_t keysize, size_t key_slot, size_t elemsize) {
  if (key_slot && (key_slot < keysize || (key_slot & 7))) return 0;
  const size_t slot = key_slot ? key_slot : (keysize + 7) & ~(size_t)7;
  return 24 + slot + ((elemsize + 7) & ~(size_t)7);
}

PDHT_API int pdht_bucket_put_records_dev(const void *keys, size_t keysize, const void *values, size_t elemsize,
                                         size_t value_stride, size_t n, uint32_t nranks, uint32_t msg_type,
                                         uint32_t src_rank, uint32_t ht_index, size_t key_slot, void *workspace,
                                         size_t workspace_bytes, void *records, uint64_t *bucket_offsets,
                                         pdht_hip_stream_t s) {
  if (elemsize == 0) return fail("put records: elemsize must be >= 1%s", "");
  if (n && !values) return fail("put records: values must not be NULL%s", "");
  if (value_stride < elemsize) return fail("put records: value_stride must be >= elemsize%s", "");
  const size_t stride = pdht_bucket_put_record_bytes(keysize, key_slot, elemsize);
  if (stride == 0) return fail("put records: key_slot must be 0 or a multiple of 8 that is >= keysize%s", "");
  const size_t key_end = 24 + ((keysize + 7) & ~(size_t)7), pad8 = ((elemsize + 7) & ~(size_t)7) - elemsize;
  const RowsCall fill{values,
                      value_stride,
                      elemsize,
                      static_cast<uint8_t *>(records) + 12,
                      stride,
                      n,
                      static_cast<uint8_t *>(records) + key_end,
                      stride,
                      stride - key_end - elemsize - pad8,
                      pad8,
                      false};
  if (n && !records) return fail("records must not be NULL%s", "");
  if ((uintptr_t)records & 7) return fail("records must be 8-byte aligned%s", "");
  if (int rc = rows_check(fill)) return rc;
  if (int rc = bucket_records_impl(keys, keysize, n, nranks, msg_type, src_rank, ht_index, workspace,
                                   workspace_bytes, records, stride, bucket_offsets, ST(s)))
    return rc;
  return rows_launch(fill, ST(s), g_kernel);
}
