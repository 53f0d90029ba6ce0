// table_keys.h -- the keyed put and get of the device-resident target table (include/pdht_hip_table_keys.h,
// DESIGN.md §4.7): the hash engine's city64 (city_core.h) joined to the table's probes (table.h), for a
// caller whose keys and values already lie on the table's device.  No wire record, no reply and no sort:
//   put_keys = two kernels, the kernel boundary their only synchronisation, as the put's
//     k_table_claim_keys<L>  one lane per key: read it, city64, table_claim, atomicMax the slot's winner
//                            word with batch | i, slot -> workspace, mbits -> mbits_out
//     k_table_write_keys<P>  a lane group per key: the key that owns its slot's winner word composes its
//                            row (key, zeros up to the slot, value, zeros up to 8) piece by piece; every
//                            group writes its status; one lane advances counters[2]
//   get_keys = one kernel
//     k_table_get_keys<P>    a lane group per key: every lane hashes and probes (table_find), the group
//                            compares the row's key bytes with the key, and the value leaves in pieces
// The probes are table_claim and table_find as they are: the private slot of mbits 0 and the stale-empty
// rule live there.
#pragma once
#include "table.h"

namespace pdht {

// ------------------------------------------------------------------- the digest ---
// CityHash64 of key i of a packed batch, keysize 1 .. 64: the three short branches of city.c:224-232.
// L = 8 / 16 / 32 / 64: keys of that length on an aligned base (8-byte for L = 8, 16-byte beyond) arrive in
// one or a few vector loads and hash out of registers with every offset folded; L = 0: any length at any
// byte address, windows read as aligned dword runs (GlobalReader: no read leaves the key's dwords).
template <int L>
__device__ __forceinline__ u64 key_digest(const uint8_t *keys, u64 i, u32 keysize) {
  if constexpr (L == 0) {
    const GlobalReader r{keys + i * keysize};
    const u64 len = keysize;
    return len <= 16 ? len0to16(r, len) : len <= 32 ? len17to32(r, len) : len33to64(r, len);
  } else {
    RegReader<L / 4> r;
    if constexpr (L == 8) {
      const u64 w = *reinterpret_cast<const u64 *>(keys + i * 8);
      r.d[0] = (u32)w, r.d[1] = (u32)(w >> 32);
      return len0to16(r, 8);
    } else {
      const u32x4 *q = reinterpret_cast<const u32x4 *>(keys + i * L);
#pragma unroll
      for (int j = 0; j < L / 16; ++j) {
        const u32x4 v = q[j];
        r.d[4 * j + 0] = v.x, r.d[4 * j + 1] = v.y, r.d[4 * j + 2] = v.z, r.d[4 * j + 3] = v.w;
      }
      if constexpr (L == 16)
        return len0to16(r, 16);
      else if constexpr (L == 32)
        return len17to32(r, 32);
      else
        return len33to64(r, 64);
    }
  }
}

// The class by a value that is uniform over the grid (the get's kernel, which is built per value piece)
__device__ __forceinline__ u64 key_digest_by(u32 lclass, const uint8_t *keys, u64 i, u32 keysize) {
  switch (lclass) {
    case 8: return key_digest<8>(keys, i, keysize);
    case 16: return key_digest<16>(keys, i, keysize);
    case 32: return key_digest<32>(keys, i, keysize);
    case 64: return key_digest<64>(keys, i, keysize);
    default: return key_digest<0>(keys, i, keysize);
  }
}

// ------------------------------------------------------------------- put_keys ---
struct KeysClaimArgs {
  TableGeom t;
  const uint8_t *keys;
  u32 keysize;
  u64 m;
  u32 *slots;
  u64 *mbits_out;  // may be null
};

// k_table_claim with the digest in front: whole waves stay together for table_count.
template <int L>
__global__ __launch_bounds__(kBlock) void k_table_claim_keys(const KeysClaimArgs a) {
  const TableGeom &t = a.t;
  const u64 batch = t.counters[2] << 32;  // (only k_table_write_keys of the same call, behind this kernel, writes it)
  const u64 nthreads = (u64)gridDim.x * kBlock;
  const u64 rounds = (a.m + nthreads - 1) / nthreads;
  u32 n_new = 0, n_drop = 0, n_seen = 0;
  u64 p = (u64)blockIdx.x * kBlock + threadIdx.x;
  for (u64 r = 0; r < rounds; ++r, p += nthreads) {
    if (p >= a.m) continue;
    const u64 mb = key_digest<L>(a.keys, p, a.keysize);
    bool made;
    const u32 slot = table_claim(t, mb, made, n_seen);
    n_new += made;
    n_drop += slot == kTableNoSlot;
    // the LAST position, one atomic per key (as k_table_claim)
    if (slot != kTableNoSlot) atomicMax((unsigned long long *)(t.win + slot), (unsigned long long)(batch | p));
    a.slots[p] = slot;
    if (a.mbits_out) a.mbits_out[p] = mb;
  }
  table_count(t, n_new, n_drop, n_seen);
}

// Where the words of a row come from: words below the key slot from the key, the rest from the value
struct RowSource {
  const uint8_t *keys;
  const uint8_t *values;
  u64 value_stride;
  u32 keysize;
  u32 slot;      // bytes of the key slot (a multiple of 8)
  u32 elemsize;
};

// nb (1 .. 8) bytes at p as the low bytes of a word, the rest zero.  Reads the aligned dwords that hold one
// of the bytes and no other (the index of a dword past the last is clamped: loads without branches).
__device__ __forceinline__ u64 bytes_word(const uint8_t *p, u32 nb) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const u32 r = (u32)(a & 3), lastd = (r + nb - 1) >> 2;  // 0 .. 2
  gu32 *q = reinterpret_cast<gu32 *>(a & ~(uintptr_t)3);
  const u32 d0 = q[0], d1 = q[lastd < 1 ? lastd : 1], d2 = q[lastd];
  const u32 lo = __builtin_amdgcn_alignbyte(d1, d0, r), hi = __builtin_amdgcn_alignbyte(d2, d1, r);
  const u64 w = ((u64)hi << 32) | lo;
  return nb >= 8 ? w : w & ((1ull << (8 * nb)) - 1);
}

// Word w (8 bytes) of a row -- key bytes, zeros up to the slot, value bytes, zeros up to 8 -- as a place in
// its source that does not depend on the key's index: a lane's piece is the same for every row it moves.
struct WordSource {
  const uint8_t *base;  // of key 0
  u64 stride;
  u32 nb;  // bytes to read, 0 .. 8: a word of nothing but padding reads byte 0 of its source and drops it
};

__device__ __forceinline__ WordSource word_source(const RowSource &s, u32 w) {
  const u32 at = w * 8;
  const bool k = at < s.slot;
  const u32 off = k ? at : at - s.slot, len = k ? s.keysize : s.elemsize;
  const u32 nb = off < len ? (len - off < 8 ? len - off : 8u) : 0u;
  return WordSource{(k ? s.keys : s.values) + (nb ? off : 0), k ? (u64)s.keysize : s.value_stride, nb};
}

// A: whole-word sources (RowSource::aligned), one 8-byte load; else the aligned dwords that hold the bytes
template <bool A>
__device__ __forceinline__ u64 word_load(const WordSource &ws, u64 i) {
  const uint8_t *p = ws.base + i * ws.stride;
  u64 v;
  if constexpr (A)
    v = *reinterpret_cast<const u64 *>(p);
  else
    v = bytes_word(p, ws.nb ? ws.nb : 1);
  return ws.nb ? v : 0;
}

// Piece c (P bytes) of a row as its P / 8 words
template <int P>
struct PieceSource {
  WordSource w[P / 8];
};

template <int P>
__device__ __forceinline__ PieceSource<P> piece_source(const RowSource &s, u32 c) {
  PieceSource<P> ps;
#pragma unroll
  for (int k = 0; k < P / 8; ++k) ps.w[k] = word_source(s, (P / 8) * c + k);
  return ps;
}

template <int P, bool A>
__device__ __forceinline__ typename RowPiece<P>::type piece_load(const PieceSource<P> &ps, u64 i) {
  if constexpr (P == 16) {
    const u64 a = word_load<A>(ps.w[0], i), b = word_load<A>(ps.w[1], i);
    return u32x4{(u32)a, (u32)(a >> 32), (u32)b, (u32)(b >> 32)};
  } else {
    return word_load<A>(ps.w[0], i);
  }
}

struct KeysWriteArgs {
  TableGeom t;
  RowSource s;
  u64 m;
  const u32 *slots;
  uint8_t *status;  // may be null
  u32 np;           // pieces of a row
  u32 gshift;       // log2 of the lane group (G = the power of two >= np, at most 64)
  u32 absent;       // status of a key without a slot: 2 dropped (put_keys), 3 not found (update_keys, table_keys_rmw.h)
};

// P: 16 or 8 bytes per piece of the table's row.  A: keys, keysize, values, value_stride and elemsize are all
// multiples of 8 (whole-word loads).  Shape of k_table_write: a group's loads (slot, winner word, row piece)
// of kRowsInFlight keys are issued ahead of their predicated stores.
template <int P, bool NT, bool A>
__global__ __launch_bounds__(kBlock) void k_table_write_keys(const KeysWriteArgs a) {
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
  for (u64 base = wave * step; base < a.m; base += nwaves * step) {
    u64 row[R];
    u32 slot[R];
    bool own[R];
    T v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      row[r] = base + (u64)r * rpi + g;
      slot[r] = a.slots[row[r] < last ? row[r] : last];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const u64 p = row[r] < last ? row[r] : last;
      // the winner word of a slot this batch touched carries this batch's number: the position decides
      const u64 w = t.win[slot[r] == kTableNoSlot ? 0 : slot[r]];
      own[r] = slot[r] != kTableNoSlot && (u32)w == (u32)p && row[r] < a.m;
      v[r] = piece_load<P, A>(mine, p);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) rows_keep(v[r]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (own[r] && l < a.np) st<NT>(v[r], reinterpret_cast<T *>(t.rows + (u64)slot[r] * t.rowbytes + (u64)l * P));
      if (own[r]) {  // rows of more pieces than a wave has lanes
        uint8_t *d = t.rows + (u64)slot[r] * t.rowbytes;
        for (u32 c = l + 64; c < a.np; c += 64)
          st<NT>(piece_load<P, A>(piece_source<P>(a.s, c), row[r]), reinterpret_cast<T *>(d + (u64)c * P));
      }
      if (a.status && l == 0 && row[r] < a.m) a.status[row[r]] = slot[r] == kTableNoSlot ? a.absent : own[r] ? 0 : 1;
    }
  }
}

// ------------------------------------------------------------------- get_keys ---
struct KeysGetArgs {
  TableGeom t;
  const uint8_t *keys;
  u32 keysize;
  u32 lclass;  // key_digest's L
  u32 slot;    // bytes of the key slot: the value's offset in the row
  u64 m;
  uint8_t *values;
  u64 value_stride;
  u64 *mbits_out;  // may be null
  uint8_t *status;
  u32 np;      // pieces of a value
  u32 gshift;  // log2 of the lane group: lanes for the value pieces, and for the key at 4 bytes a lane
};

// P: 16 / 8 / 4 / 1 bytes per piece of the value, the widest that row + slot, values, value_stride and
// elemsize allow.  A lane group per key: every lane of the group hashes its key and probes (one address per
// group: the wave's loads merge), the row's key bytes are compared across the group, and the value piece is
// loaded without a branch (of slot 0 when there is no row) ahead of the predicated store.
template <int P>
__global__ __launch_bounds__(kBlock) void k_table_get_keys(const KeysGetArgs a) {
  typedef typename RowPiece<P>::type T;
  const TableGeom &t = a.t;
  const u32 lane = threadIdx.x & 63;
  const u64 wave = (u64)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const u64 nwaves = (u64)gridDim.x * kWavesPerBlock;
  const u32 G = 1u << a.gshift, l = lane & (G - 1), g = lane >> a.gshift, rpi = 64u >> a.gshift;
  const u64 gmask = (G == 64 ? ~0ull : (1ull << G) - 1) << (g * G);
  const u64 last = a.m - 1;
  for (u64 base = wave * rpi; base < a.m; base += nwaves * rpi) {
    const u64 p = base + g, pc = p < last ? p : last;
    const u64 mb = key_digest_by(a.lclass, a.keys, pc, a.keysize);
    const u32 slot = table_find(t, mb);
    const bool found = slot != kTableNoSlot;
    const uint8_t *row = t.rows + (u64)(found ? slot : 0) * t.rowbytes;
    const uint8_t *key = a.keys + pc * a.keysize;
    const T v = *reinterpret_cast<const T *>(row + a.slot + (u64)(l < a.np ? l : 0) * P);
    bool differ = false;
    for (u32 c = l; c < a.keysize; c += G) differ |= row[c] != key[c];
    const bool collide = (__ballot(differ) & gmask) != 0;
    const bool ok = found && !collide && p < a.m;
    if (ok) {
      uint8_t *d = a.values + p * a.value_stride;
      if (l < a.np) *reinterpret_cast<T *>(d + (u64)l * P) = v;
      const uint8_t *s = row + a.slot;
      for (u32 c = l + 64; c < a.np; c += 64)
        *reinterpret_cast<T *>(d + (u64)c * P) = *reinterpret_cast<const T *>(s + (u64)c * P);
    }
    if (l == 0 && p < a.m) {
      a.status[p] = !found ? 2 : collide ? 3 : 0;
      if (a.mbits_out) a.mbits_out[p] = mb;
    }
  }
}

}  // namespace pdht
