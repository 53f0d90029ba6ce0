// rows.h -- row movers by index (include/pdht_hip_put.h pdht_gather_rows_dev /
// pdht_scatter_rows_dev, and the value half of pdht_bucket_put_records_dev):
// the payload of a bucketed batch follows its keys into bucket order, and
// replies that come back in bucket order return to the caller's order.
//
// Shape: a row is cut into pieces of P = 16 / 8 / 4 / 1 bytes,
// the widest that divides the row length, both strides and both base
// addresses, so every access is naturally aligned.  G = the power of two >=
// the pieces of a destination row (at most 64) consecutive lanes move one row:
// a group's stores are one contiguous run, and one wave instruction covers
// 64 / G rows.  Each group loads the indices of kRowsInFlight rows, issues all
// their row loads and only then stores.  Rows of more than 64 pieces are swept
// by the whole wave, kRowsInFlight x 64 pieces in flight.  Row offsets are
// 64-bit products.  The index array may lie in the buffer dst points into (the
// put path reads it from the records it fills), so no pointer here is
// __restrict__: loads of an iteration are written, and stay, ahead of its stores.
#pragma once
#include "runtime.h"

namespace pdht {

constexpr int kRowsInFlight = 4;

struct RowsArgs {
  const uint8_t *src;
  u64 src_stride;
  uint8_t *dst;
  u64 dst_stride;
  const uint8_t *index;  // u32 at index + p * index_stride
  u64 index_stride;
  u64 m;
  u32 np;      // pieces of a source row
  u32 pre;     // zero pieces ahead of them in the destination row (put records: the key-slot gap)
  u32 npd;     // pieces of a destination row: pre + np + zero pieces behind (put records: the value's pad)
  u32 gshift;  // log2 G
};

template <int P>
struct RowPiece;
template <>
struct RowPiece<16> {
  typedef u32x4 type;
};
template <>
struct RowPiece<8> {
  typedef u64 type;
};
template <>
struct RowPiece<4> {
  typedef u32 type;
};
template <>
struct RowPiece<1> {
  typedef uint8_t type;
};

// Pins a loaded piece in its register where the loads are issued: without it the compiler sinks a load
// (and the index load it depends on) into the predicated block of its store, one row after the other.
template <class T>
__device__ __forceinline__ void rows_keep(T &v) {
  if constexpr (sizeof(T) < 4) {
    u32 w = v;
    asm volatile("" : "+v"(w));
    v = (T)w;
  } else {
    asm volatile("" : "+v"(v));
  }
}

// SCATTER: dst row index_p = src row p; else dst row p = src row index_p (+ the zero pieces).
// NT: non-temporal stores.
template <int P, bool SCATTER, bool NT>
__global__ __launch_bounds__(kBlock) void k_rows(const RowsArgs a) {
  typedef typename RowPiece<P>::type T;
  constexpr int R = kRowsInFlight;
  const u32 lane = threadIdx.x & 63;
  const u64 wave = (u64)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const u64 nwaves = (u64)gridDim.x * kWavesPerBlock;
  if (a.npd <= 64) {
    const u32 l = lane & ((1u << a.gshift) - 1), g = lane >> a.gshift, rpi = 64u >> a.gshift;
    const bool in_row = l < a.npd;
    const bool from_src = l >= a.pre && l - a.pre < a.np;
    // every lane loads, so that the loads carry no branches: lanes outside the source pieces read piece 0
    // of their group's row, rows past the end read the last row; only the stores are predicated
    const u64 so = from_src ? (u64)(l - a.pre) * P : 0, dof = (u64)l * P;
    const u64 step = (u64)rpi * R, last = a.m - 1;  // (m >= 1 inside the loop)
    for (u64 base = wave * step; base < a.m; base += nwaves * step) {
      u64 row[R], from[R];
      T v[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        row[r] = base + (u64)r * rpi + g;
        from[r] = *reinterpret_cast<const u32 *>(a.index + (row[r] < last ? row[r] : last) * a.index_stride);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const u64 srow = SCATTER ? (row[r] < last ? row[r] : last) : from[r];
        v[r] = *reinterpret_cast<const T *>(a.src + srow * a.src_stride + so);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) rows_keep(v[r]);
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (in_row && row[r] < a.m)
          st<NT>(from_src ? v[r] : T{},
                 reinterpret_cast<T *>(a.dst + (SCATTER ? from[r] : row[r]) * a.dst_stride + dof));
    }
    return;
  }
  for (u64 row = wave; row < a.m; row += nwaves) {
    const u64 other = *reinterpret_cast<const u32 *>(a.index + row * a.index_stride);
    const uint8_t *s = a.src + (SCATTER ? row : other) * a.src_stride;
    uint8_t *d = a.dst + (SCATTER ? other : row) * a.dst_stride;
    for (u32 c = lane; c < a.npd; c += 64 * R) {
      T v[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {  // (clamped into the source row: loads without branches)
        const u32 j = c + 64 * r, k = j < a.pre ? 0 : j - a.pre;
        v[r] = *reinterpret_cast<const T *>(s + (u64)(k < a.np ? k : a.np - 1) * P);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) rows_keep(v[r]);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const u32 j = c + 64 * r;
        if (j < a.npd) st<NT>(j >= a.pre && j - a.pre < a.np ? v[r] : T{}, reinterpret_cast<T *>(d + (u64)j * P));
      }
    }
  }
}

// ------------------------------------------------- host side (pdht_rows.hip) ---
// One mover call: dst row = pre_bytes zeros | rowbytes of the source row | post_bytes zeros
// (gather only; both 0 for the plain movers).
struct RowsCall {
  const void *src;
  size_t src_stride, rowbytes;
  const void *index;
  size_t index_stride, m;
  void *dst;
  size_t dst_stride, pre_bytes, post_bytes;
  bool scatter;
};
// Argument checks (fail(...) with a message; no device call)
int rows_check(const RowsCall &c);
// Launches the mover on `st` (nothing when m == 0) and sets the kernel tag, "<ahead>+<tag>" when
// `ahead` (the tag of a kernel launched before it in the same call) is given.
int rows_launch(const RowsCall &c, hipStream_t st, const char *ahead = nullptr);

}  // namespace pdht
