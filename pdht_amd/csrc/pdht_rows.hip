// pdht_rows.hip -- row movers by index (include/pdht_hip_put.h
// pdht_gather_rows_dev / pdht_scatter_rows_dev; kernels in rows.h).  The same
// launcher fills the values of pdht_bucket_put_records_dev (pdht_bucket.hip).
#include "rows.h"

namespace pdht {

// Store policy of the movers' stores (EXPERIMENTS.md §R8: measured per shape)
constexpr bool kRowsNtStores = true;

static thread_local char g_kernel_pair[160];

static const char *rows_tag(int piece, bool scatter) {
  switch (piece) {
    case 16: return scatter ? "k_rows_scatter<16>" : "k_rows_gather<16>";
    case 8: return scatter ? "k_rows_scatter<8>" : "k_rows_gather<8>";
    case 4: return scatter ? "k_rows_scatter<4>" : "k_rows_gather<4>";
    default: return scatter ? "k_rows_scatter<1>" : "k_rows_gather<1>";
  }
}

// The widest of 16 / 8 / 4 / 1 bytes that divides every length, stride and base address of the call
static int rows_piece(const RowsCall &c) {
  const uintptr_t bits = (uintptr_t)c.src | (uintptr_t)c.dst | c.src_stride | c.dst_stride | c.rowbytes |
                         c.pre_bytes | c.post_bytes;
  return (bits & 15) == 0 ? 16 : (bits & 7) == 0 ? 8 : (bits & 3) == 0 ? 4 : 1;
}

int rows_check(const RowsCall &c) {
  if (c.m >= (1ull << 32)) return fail("row movers: m must be < 2^32 per call%s", "");
  if (c.rowbytes == 0) return fail("row movers: rowbytes must be >= 1%s", "");
  if (c.src_stride < c.rowbytes) return fail("row movers: src_stride must be >= rowbytes%s", "");
  if (c.dst_stride < c.pre_bytes + c.rowbytes + c.post_bytes)
    return fail("row movers: dst_stride must be >= rowbytes%s", "");
  if (c.index_stride < 4 || (c.index_stride & 3))
    return fail("row movers: index_stride must be a multiple of 4 and >= 4%s", "");
  if ((uintptr_t)c.index & 3) return fail("row movers: index must be 4-byte aligned%s", "");
  if (c.m && (!c.src || !c.dst || !c.index)) return fail("row movers: null src, dst or index%s", "");
  if ((c.pre_bytes + c.rowbytes + c.post_bytes) >> 31) return fail("row movers: rowbytes must be < 2^31%s", "");
  return 0;
}

template <int P, bool SCATTER>
static void rows_start(const RowsArgs &a, unsigned grid, bool nt, hipStream_t st) {
  if (nt)
    k_rows<P, SCATTER, true><<<grid, kBlock, 0, st>>>(a);
  else
    k_rows<P, SCATTER, false><<<grid, kBlock, 0, st>>>(a);
}

int rows_launch(const RowsCall &c, hipStream_t st, const char *ahead) {
  const int piece = rows_piece(c);
  const char *tag = rows_tag(piece, c.scatter);
  if (ahead) {
    snprintf(g_kernel_pair, sizeof g_kernel_pair, "%s+%s", ahead, tag);
    tag = g_kernel_pair;
  }
  if (c.m == 0) {
    g_kernel = tag;
    return 0;
  }
  int dev;
  if (int rc = current_device(&dev)) return rc;
  RowsArgs a{};
  a.src = static_cast<const uint8_t *>(c.src);
  a.src_stride = c.src_stride;
  a.dst = static_cast<uint8_t *>(c.dst);
  a.dst_stride = c.dst_stride;
  a.index = static_cast<const uint8_t *>(c.index);
  a.index_stride = c.index_stride;
  a.m = c.m;
  a.np = (u32)(c.rowbytes / piece);
  a.pre = (u32)(c.pre_bytes / piece);
  a.npd = a.pre + a.np + (u32)(c.post_bytes / piece);
  while (a.gshift < 6 && (1u << a.gshift) < a.npd) ++a.gshift;
  // waves: one per kRowsInFlight instructions' rows (64 / G rows each), or one per swept row
  const u64 per_wave = a.npd <= 64 ? (u64)(64u >> a.gshift) * kRowsInFlight : 1;
  const u64 waves = (c.m + per_wave - 1) / per_wave;
  const unsigned grid = grid_for((waves + kWavesPerBlock - 1) / kWavesPerBlock, 8, dev);
  const bool nt = hook_rows_nt(kRowsNtStores);
  auto go = [&](auto P) {
    if (c.scatter)
      rows_start<decltype(P)::value, true>(a, grid, nt, st);
    else
      rows_start<decltype(P)::value, false>(a, grid, nt, st);
  };
  using std::integral_constant;
  if (piece == 16)
    go(integral_constant<int, 16>{});
  else if (piece == 8)
    go(integral_constant<int, 8>{});
  else if (piece == 4)
    go(integral_constant<int, 4>{});
  else
    go(integral_constant<int, 1>{});
  g_kernel = tag;
  HIP_TRY(hipGetLastError());
  return 0;
}

static int rows_move(const void *src, size_t src_stride, size_t rowbytes, const void *index, size_t index_stride,
                     size_t m, void *dst, size_t dst_stride, bool scatter, hipStream_t st) {
  const RowsCall c{src, src_stride, rowbytes, index, index_stride, m, dst, dst_stride, 0, 0, scatter};
  if (int rc = rows_check(c)) return rc;
  return rows_launch(c, st);
}

}  // namespace pdht

using namespace pdht;

PDHT_API int pdht_gather_rows_dev(const void *src, size_t src_stride, size_t rowbytes, const void *index,
                                  size_t index_stride, size_t m, void *dst, size_t dst_stride,
                                  pdht_hip_stream_t s) {
  return rows_move(src, src_stride, rowbytes, index, index_stride, m, dst, dst_stride, false, ST(s));
}

PDHT_API int pdht_scatter_rows_dev(const void *src, size_t src_stride, size_t rowbytes, const void *index,
                                   size_t index_stride, size_t m, void *dst, size_t dst_stride,
                                   pdht_hip_stream_t s) {
  return rows_move(src, src_stride, rowbytes, index, index_stride, m, dst, dst_stride, true, ST(s));
}
