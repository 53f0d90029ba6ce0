// table_keys_rmw.h -- update, insert-if-absent and compare-and-swap by KEY on the device-resident target
// table (include/pdht_hip_table_keys_rmw.h): the digest of table_keys.h in front of the
// locating probe of table_rmw.h and the claiming probe of table_add.h, for a caller whose keys and values
// already lie on the table's device.  No wire record and no sort; each call is two kernels, the kernel
// boundary their only synchronisation (nothing spins, polls or waits on another lane):
//   update_keys = k_table_locate_keys<L, last>  -> k_table_write_keys<P> of table_keys.h (absent = 3)
//   cswap_keys  = k_table_locate_keys<L, first> -> k_table_cswap of table_rmw.h as it stands
//   add_keys    = k_table_add_claim_keys<L>     -> k_table_add_write_keys<P>
// Matching is by mbits = CityHash64(key) alone, as in the record operations and in put_keys: no kernel here
// compares a row's key bytes.  The probes are table_find and table_claim as they are: the tag protocol, the
// private slot of mbits 0 and the stale-empty rule live in table.h.
#pragma once
#include "table_keys.h"
#include "table_rmw.h"

namespace pdht {

struct KeysLocateArgs {
  TableGeom t;
  const uint8_t *keys;
  u32 keysize;
  u64 m;
  u32 *slots;
  u64 *mbits_out;  // may be null
};

// k_table_locate<FIRST> with the digest in front: one lane per key, table_find (nothing is inserted), the
// slot -> workspace, the digest -> mbits_out, and on a hit the winner word through table_win_post.
template <int L, bool FIRST>
__global__ __launch_bounds__(kBlock) void k_table_locate_keys(const KeysLocateArgs a) {
  const TableGeom &t = a.t;
  const u64 batch = t.counters[2] << 32;  // (only the second kernel of the same call, behind this one, writes it)
  const u32 lane = threadIdx.x & 63;
  const u64 nthreads = (u64)gridDim.x * kBlock;
  const u64 rounds = (a.m + nthreads - 1) / nthreads;  // k_table_locate's shape: whole waves stay together
  u64 p = (u64)blockIdx.x * kBlock + threadIdx.x;
  for (u64 r = 0; r < rounds; ++r, p += nthreads) {
    u32 slot = kTableNoSlot;
    if (p < a.m) {
      const u64 mb = key_digest<L>(a.keys, p, a.keysize);
      slot = table_find(t, mb);
      a.slots[p] = slot;
      if (a.mbits_out) a.mbits_out[p] = mb;
    }
    table_win_post<FIRST>(t, slot, p, batch, lane);
  }
}

struct KeysAddClaimArgs {
  TableGeom t;
  const uint8_t *keys;
  u32 keysize;
  u64 m;
  u32 *slots;
  uint8_t *creator;  // 1: this key's CAS created its slot's tag
  u64 *mbits_out;    // may be null
  uint8_t *status;   // may be null; provisional: 2 dropped, 4 has a slot
};

// k_table_add_claim of table_add.h with the digest in front.  No row byte is touched.
template <int L>
__global__ __launch_bounds__(kBlock) void k_table_add_claim_keys(const KeysAddClaimArgs a) {
  const TableGeom &t = a.t;
  const u64 batch = t.counters[2] << 32;  // (only k_table_add_write_keys of the same call, behind this kernel, writes it)
  const u32 lane = threadIdx.x & 63;
  const u64 nthreads = (u64)gridDim.x * kBlock;
  const u64 rounds = (a.m + nthreads - 1) / nthreads;  // whole waves stay together for the wave-wide steps
  u32 n_new = 0, n_drop = 0, n_seen = 0;
  u64 p = (u64)blockIdx.x * kBlock + threadIdx.x;
  for (u64 r = 0; r < rounds; ++r, p += nthreads) {
    u32 slot = kTableNoSlot;
    if (p < a.m) {
      const u64 mb = key_digest<L>(a.keys, p, a.keysize);
      bool made;
      slot = table_claim(t, mb, made, n_seen);
      n_new += made;
      n_drop += slot == kTableNoSlot;
      a.slots[p] = slot;
      a.creator[p] = made;
      if (a.mbits_out) a.mbits_out[p] = mb;
      if (a.status) a.status[p] = slot == kTableNoSlot ? 2 : 4;  // the creator turns the first key's 4 into 0
    }
    table_win_post<true>(t, slot, p, batch, lane);  // the first position
  }
  table_count(t, n_new, n_drop, n_seen);
}

struct KeysAddWriteArgs {
  TableGeom t;
  RowSource s;
  u64 m;
  const u32 *slots;
  const uint8_t *creator;
  uint8_t *status;  // may be null
  u32 np;           // pieces of a row
  u32 gshift;       // log2 of the lane group (G = the power of two >= np, at most 64)
};

// k_table_add_write of table_add.h with its row source replaced: only the creator of a slot acts.  It reads
// the winner word -- the first key f of the slot --, composes the row of key f (not its own) from key and
// value as k_table_write_keys does, and sets status[f] = 0.  P, A: as k_table_write_keys.  A group's loads
// of kRowsInFlight rows are issued ahead of their predicated stores; a wave none of whose keys created a
// slot reads the marks and nothing else.
template <int P, bool NT, bool A>
__global__ __launch_bounds__(kBlock) void k_table_add_write_keys(const KeysAddWriteArgs a) {
  typedef typename RowPiece<P>::type T;
  constexpr int R = kRowsInFlight;
  const TableGeom &t = a.t;
  const u32 lane = threadIdx.x & 63;
  const u64 wave = (u64)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const u64 nwaves = (u64)gridDim.x * kWavesPerBlock;
  if (wave == 0 && lane == 0) t.counters[2] += 1;  // nothing in this kernel reads it
  const u32 l = lane & ((1u << a.gshift) - 1), g = lane >> a.gshift, rpi = 64u >> a.gshift;
  const PieceSource<P> mine = piece_source<P>(a.s, l < a.np ? l : 0);  // (a lane outside the row loads piece 0)
  const u64 step = (u64)rpi * R, last = a.m - 1;
  for (u64 base = wave * step; base < a.m; base += nwaves * step) {  // (base is wave-uniform)
    u64 row[R], first[R];
    u32 slot[R];
    bool made[R], any = false;
    T v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      row[r] = base + (u64)r * rpi + g;
      made[r] = row[r] < a.m && a.creator[row[r] < last ? row[r] : last];
      any |= made[r];
    }
    if (!__ballot(any)) continue;  // (wave-uniform)
#pragma unroll
    for (int r = 0; r < R; ++r) slot[r] = made[r] ? a.slots[row[r]] : 0;  // loads without a branch: slot 0's
#pragma unroll
    for (int r = 0; r < R; ++r) {
      // the winner word of a slot this batch created carries this batch's number and its first position
      const u64 f = 0xFFFFFFFFu - (u32)t.win[slot[r]];
      first[r] = made[r] ? (f < last ? f : last) : 0;
      v[r] = piece_load<P, A>(mine, first[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) rows_keep(v[r]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!made[r]) continue;
      uint8_t *d = t.rows + (u64)slot[r] * t.rowbytes;
      if (l < a.np) st<NT>(v[r], reinterpret_cast<T *>(d + (u64)l * P));
      for (u32 c = l + 64; c < a.np; c += 64)  // rows of more pieces than a wave has lanes
        st<NT>(piece_load<P, A>(piece_source<P>(a.s, c), first[r]), reinterpret_cast<T *>(d + (u64)c * P));
      if (a.status && l == 0) a.status[first[r]] = 0;
    }
  }
}

}  // namespace pdht
