// table.h -- the device-resident target table (include/pdht_hip_table.h): the
// owner's side of a put and a get (the server loop of libmpipdht/init.c:173-290
// over a table keyed by mbits) and the client's resolve (putget.c:50-59), each
// as one batch.
//
// Layout of the caller's buffer, C = capacity, B = rowbytes:
//   +0            u64 counters[4]   entries / dropped / batches / slots inspected
//   +64           u64 tags[C + 1]   0 = empty, else the mbits stored there
//   +64+8(C+1)    u64 win[C + 1]    (batch << 32) | position of the last writer
//   +64+16(C+1)   rows[C + 1][B]
// Open addressing with linear probing from home = (mbits * 2^64/phi) >> (64 -
// log2 C): the high bits of a multiplicative mix, because a rank only ever
// sees mbits with mbits % nranks == rank.  Slot C is private to mbits 0, whose
// value is the empty mark: tags[C] is 0 (absent) or 1 (present).
//
// A tag only ever changes from empty to an mbits, and only through a 64-bit
// device-scope atomicCAS, which is resolved in memory behind the per-XCD L2s.
// The probes read tags with relaxed device-scope atomic loads (sc1: past the
// CU's L1, which another CU's CAS never refreshes; a random 8-byte probe has
// no L1 reuse to lose).  What such a load can still see stale is "empty" for a
// slot that another XCD has just claimed -- then the CAS fails and returns the
// tag that is there, and the probe goes on from that value; a non-empty tag is
// final.  So no lane waits for another: every loop counts down from C.
//
// What the operations share is here: table_find (the probe that inserts nothing), table_claim (the probe
// that claims an empty slot, with table_count for the counters), table_win_post (the winner word of a slot,
// one atomicMax per slot and wave), k_table_write (the rows of a put or an update) and k_table_get (the
// replies of a get, and on the slots of a workspace those of an insert-if-absent or a reduce).
//
// put = two kernels, the kernel boundary their only synchronisation:
//   k_table_claim  one lane per record: probe, claim when new, atomicMax the
//                  slot's winner word with (batch << 32) | position, slot -> workspace.
//                  batch = counters[2] as the call found it, so winner words of earlier
//                  batches always lose and are never cleared.
//   k_table_write  a lane group per record: the record that owns its slot's winner word
//                  copies its row; every group writes its status; one lane advances counters[2].
#pragma once
#include "table_geom.h"

namespace pdht {

__device__ __forceinline__ u64 tag_load(const u64 *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The slot that holds mb, or kTableNoSlot.  Every lane may call it with its own mb.
__device__ __forceinline__ u32 table_find(const TableGeom &t, u64 mb) {
  if (mb == 0) return tag_load(t.tags + t.cap) ? t.cap : kTableNoSlot;
  u64 h = (mb * kTableMix) >> t.shift;
  for (u64 left = t.mask + 1; left; --left) {
    const u64 tag = tag_load(t.tags + (h & t.mask));
    if (tag == mb) return (u32)(h & t.mask);
    if (tag == 0) return kTableNoSlot;
    h = (h + 1) & t.mask;
  }
  return kTableNoSlot;
}

__device__ __forceinline__ u32 wave_sum(u32 v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ u32 wave_max(u32 v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = max(v, (u32)__shfl_xor(v, o));
  return v;
}

// The inserting probe of the put, the insert-if-absent and the inserting accumulate: the slot that holds
// mb, claimed when no slot held it, or kTableNoSlot when the table is full.  made: this lane's CAS created
// the tag.  n_seen counts the slots inspected.  Every lane may call it with its own mb.
__device__ __forceinline__ u32 table_claim(const TableGeom &t, u64 mb, bool &made, u32 &n_seen) {
  made = false;
  if (mb == 0) {
    ++n_seen;
    made = tag_load(t.tags + t.cap) == 0 && atomicCAS((unsigned long long *)(t.tags + t.cap), 0ull, 1ull) == 0;
    return t.cap;
  }
  u64 h = (mb * kTableMix) >> t.shift;
  for (u64 left = t.mask + 1; left; --left) {
    h &= t.mask;
    ++n_seen;
    u64 tag = tag_load(t.tags + h);
    if (tag == 0) {
      tag = atomicCAS((unsigned long long *)(t.tags + h), 0ull, (unsigned long long)mb);
      if (tag == 0) {
        made = true;
        tag = mb;
      }
    }
    if (tag == mb) return (u32)h;
    ++h;
  }
  return kTableNoSlot;
}

// A claim kernel's counts (entries made, records dropped, slots inspected) into the table's counters: one
// atomic per wave per counter.  Whole waves call it.
__device__ __forceinline__ void table_count(const TableGeom &t, u32 n_new, u32 n_drop, u32 n_seen) {
  n_new = wave_sum(n_new), n_drop = wave_sum(n_drop), n_seen = wave_sum(n_seen);
  if ((threadIdx.x & 63) == 0) {
    if (n_new) atomicAdd((unsigned long long *)(t.counters + 0), (unsigned long long)n_new);
    if (n_drop) atomicAdd((unsigned long long *)(t.counters + 1), (unsigned long long)n_drop);
    if (n_seen) atomicAdd((unsigned long long *)(t.counters + 3), (unsigned long long)n_seen);
  }
}

// The winner word of `slot` takes batch | rank of position p: the FIRST position of a slot wins with rank
// 0xFFFFFFFF - p, the last with rank p.  Whole waves call it, a lane without a slot with kTableNoSlot.
// Lanes of a wave that found the same slot post one atomicMax between them: a batch whose requests pile
// up on one mbits (every claimant of a hot k-mer) would otherwise queue one atomic per request on one
// word (EXPERIMENTS.md §R11).  Two leaders are tried -- the first lane that has a slot, then the first
// lane outside its group -- and every lane left over posts its own.  The maximum of a group's ranks is
// what its atomics would have left, so the winner word ends the same.
constexpr int kLocateLeaders = 2;

template <bool FIRST>
__device__ __forceinline__ void table_win_post(const TableGeom &t, u32 slot, u64 p, u64 batch, u32 lane) {
  const u32 rank = FIRST ? 0xFFFFFFFFu - (u32)p : (u32)p;
  bool todo = slot != kTableNoSlot, cand = todo;
#pragma unroll
  for (int k = 0; k < kLocateLeaders; ++k) {
    const u64 open = __ballot(cand);
    if (!open) break;  // (wave-uniform)
    const u32 leader = (u32)__ffsll((unsigned long long)open) - 1;
    const u32 s = (u32)__shfl((int)slot, (int)leader);
    const bool mine = cand && slot == s;
    cand = cand && !mine;
    if (__popcll(__ballot(mine)) < 2) continue;  // (wave-uniform) the leader stands alone: its own atomic below
    const u32 best = wave_max(mine ? rank : 0u);
    if (lane == leader) atomicMax((unsigned long long *)(t.win + s), (unsigned long long)(batch | best));
    todo = todo && !mine;
  }
  if (todo) atomicMax((unsigned long long *)(t.win + slot), (unsigned long long)(batch | rank));
}

struct ClaimArgs {
  TableGeom t;
  const uint8_t *records;
  u64 record_stride;
  u64 m;
  u32 *slots;
};

// (static: table.h is part of several translation units)
static __global__ __launch_bounds__(kBlock) void k_table_claim(const ClaimArgs a) {
  const TableGeom &t = a.t;
  const u64 batch = t.counters[2] << 32;  // (only k_table_write of the same call, behind this kernel, writes it)
  const u64 nthreads = (u64)gridDim.x * kBlock;
  const u64 rounds = (a.m + nthreads - 1) / nthreads;  // whole waves stay together for the wave-wide counts
  u32 n_new = 0, n_drop = 0, n_seen = 0;
  u64 p = (u64)blockIdx.x * kBlock + threadIdx.x;
  for (u64 r = 0; r < rounds; ++r, p += nthreads) {
    if (p >= a.m) continue;
    bool made;
    const u32 slot = table_claim(t, *reinterpret_cast<const u64 *>(a.records + p * a.record_stride + 16), made, n_seen);
    n_new += made;
    n_drop += slot == kTableNoSlot;
    // the LAST position, one atomic per record (no leaders: table_win_post needs whole waves)
    if (slot != kTableNoSlot) atomicMax((unsigned long long *)(t.win + slot), (unsigned long long)(batch | p));
    a.slots[p] = slot;
  }
  table_count(t, n_new, n_drop, n_seen);
}

struct WriteArgs {
  TableGeom t;
  const uint8_t *records;
  u64 record_stride;
  u64 m;
  const u32 *slots;
  uint8_t *status;  // may be null
  u32 np;           // pieces of a row
  u32 gshift;       // log2 of the lane group (G = the power of two >= np, at most 64)
  u32 absent;       // status of a record without a slot: 2 dropped (put), 3 not found (update, table_rmw.h)
};

// P: 16 or 8 bytes per piece.  Shape of k_rows: a group's loads (slot, winner word, row piece) of
// kRowsInFlight records are issued ahead of their predicated stores.
template <int P, bool NT>
__global__ __launch_bounds__(kBlock) void k_table_write(const WriteArgs a) {
  typedef typename RowPiece<P>::type T;
  constexpr int R = kRowsInFlight;
  const TableGeom &t = a.t;
  const u32 lane = threadIdx.x & 63;
  const u64 wave = (u64)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const u64 nwaves = (u64)gridDim.x * kWavesPerBlock;
  if (wave == 0 && lane == 0) t.counters[2] += 1;  // nothing in this kernel reads it
  const u32 l = lane & ((1u << a.gshift) - 1), g = lane >> a.gshift, rpi = 64u >> a.gshift;
  const u64 lo = (u64)(l < a.np ? l : 0) * P;
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
      v[r] = *reinterpret_cast<const T *>(a.records + p * a.record_stride + 24 + lo);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) rows_keep(v[r]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (own[r] && l < a.np) st<NT>(v[r], reinterpret_cast<T *>(t.rows + (u64)slot[r] * t.rowbytes + lo));
      if (own[r]) {  // rows of more pieces than a wave has lanes
        const uint8_t *s = a.records + row[r] * a.record_stride + 24;
        uint8_t *d = t.rows + (u64)slot[r] * t.rowbytes;
        for (u32 c = l + 64; c < a.np; c += 64)
          st<NT>(*reinterpret_cast<const T *>(s + (u64)c * P), reinterpret_cast<T *>(d + (u64)c * P));
      }
      if (a.status && l == 0 && row[r] < a.m) a.status[row[r]] = slot[r] == kTableNoSlot ? a.absent : own[r] ? 0 : 1;
    }
  }
}

struct GetArgs {
  TableGeom t;
  const uint8_t *mbits;  // the requests, or
  const u32 *slots;      // SLOTS: every request's slot or kTableNoSlot, as a claim or locate kernel left it
  u64 mbits_stride;
  u64 m;
  uint8_t *replies;
  u64 reply_stride;
  u32 head;    // k_table_get_bytes only
  u32 np;      // pieces of a reply: words (1 + B/8) / W, or bytes head + B
  u32 gshift;  // log2 of the lane group
};

// head 8 on aligned replies: the reply is 1 + B/8 words, word 0 the status, word k row word k - 1.  A lane
// moves W = 1 or 2 of them (2: one 16-byte store).  Every lane of a group probes for its request (one
// address per group: the wave's load merges them); the row words are loaded without a branch (of slot 0
// when there is no row) ahead of the predicated stores.
// SLOTS: the replies of the insert-if-absent and of the reduce ("k_table_add_reply<W>" in last_kernel), whose
// first kernel left every record's slot in the workspace: no probe, no tag line is touched.
template <int W, bool NT, bool SLOTS = false>
__global__ __launch_bounds__(kBlock) void k_table_get(const GetArgs a) {
  const TableGeom &t = a.t;
  const u32 lane = threadIdx.x & 63;
  const u64 wave = (u64)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const u64 nwaves = (u64)gridDim.x * kWavesPerBlock;
  const u32 l = lane & ((1u << a.gshift) - 1), g = lane >> a.gshift, rpi = 64u >> a.gshift;
  const u64 last = a.m - 1;
  const u32 nw = (u32)(t.rowbytes >> 3) + 1;
  for (u64 base = wave * rpi; base < a.m; base += nwaves * rpi) {
    const u64 p = base + g, pc = p < last ? p : last;
    u32 slot;
    if constexpr (SLOTS)
      slot = a.slots[pc];
    else
      slot = table_find(t, *reinterpret_cast<const u64 *>(a.mbits + pc * a.mbits_stride));
    const bool found = slot != kTableNoSlot;
    const u64 *row = reinterpret_cast<const u64 *>(t.rows + (u64)(found ? slot : 0) * t.rowbytes);
    for (u32 c = l; c < a.np; c += 64) {
      u64 w[W];
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const u32 j = c * W + k;  // reply word
        w[k] = row[j ? (j < nw ? j - 1 : 0) : 0];
      }
#pragma unroll
      for (int k = 0; k < W; ++k) {
        rows_keep(w[k]);
        w[k] = c * W + k == 0 ? (u64)found : found ? w[k] : 0;
      }
      if (p < a.m) {
        uint8_t *d = a.replies + p * a.reply_stride + (u64)c * (8 * W);
        if constexpr (W == 2) {
          u32x4 q = {(u32)w[0], (u32)(w[0] >> 32), (u32)w[1], (u32)(w[1] >> 32)};
          st<NT>(q, reinterpret_cast<u32x4 *>(d));
        } else {
          st<NT>(w[0], reinterpret_cast<u64 *>(d));
        }
      }
    }
  }
}

// Any head, address and stride: byte pieces (head 1 is reply_t + value of init.c:195-219, packed).
template <bool NT>
__global__ __launch_bounds__(kBlock) void k_table_get_bytes(const GetArgs a) {
  const TableGeom &t = a.t;
  const u32 lane = threadIdx.x & 63;
  const u64 wave = (u64)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const u64 nwaves = (u64)gridDim.x * kWavesPerBlock;
  const u32 l = lane & ((1u << a.gshift) - 1), g = lane >> a.gshift, rpi = 64u >> a.gshift;
  const u64 last = a.m - 1;
  for (u64 base = wave * rpi; base < a.m; base += nwaves * rpi) {
    const u64 p = base + g;
    const u64 mb = *reinterpret_cast<const u64 *>(a.mbits + (p < last ? p : last) * a.mbits_stride);
    const u32 slot = table_find(t, mb);
    const bool found = slot != kTableNoSlot;
    const uint8_t *row = t.rows + (u64)(found ? slot : 0) * t.rowbytes;
    for (u32 c = l; c < a.np; c += 64) {
      uint8_t b = row[c >= a.head ? c - a.head : 0];
      rows_keep(b);
      b = c == 0 ? (uint8_t)found : (c >= a.head && found) ? b : (uint8_t)0;
      if (p < a.m) st<NT>(b, a.replies + p * a.reply_stride + c);
    }
  }
}

struct ResolveArgs {
  const uint8_t *replies;
  u64 reply_stride;
  u32 head;
  u32 keysize;
  u64 value_offset;
  const uint8_t *keys;
  const uint8_t *index;  // may be null
  u64 index_stride;
  u64 m;
  uint8_t *values;
  u64 value_stride;
  uint8_t *status;
  u32 np;      // pieces of a value
  u32 gshift;  // log2 of the lane group
};

// A lane group per reply: index load, key compare across the group (bytes: keys are packed at any
// length), then the value pieces to row i and the status byte.
template <int P>
__global__ __launch_bounds__(kBlock) void k_get_resolve(const ResolveArgs a) {
  typedef typename RowPiece<P>::type T;
  const u32 lane = threadIdx.x & 63;
  const u64 wave = (u64)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const u64 nwaves = (u64)gridDim.x * kWavesPerBlock;
  const u32 G = 1u << a.gshift, l = lane & (G - 1), g = lane >> a.gshift, rpi = 64u >> a.gshift;
  const u64 gmask = (G == 64 ? ~0ull : (1ull << G) - 1) << (g * G);
  const u64 last = a.m - 1;
  for (u64 base = wave * rpi; base < a.m; base += nwaves * rpi) {
    const u64 p = base + g, pc = p < last ? p : last;
    const u64 i = a.index ? *reinterpret_cast<const u32 *>(a.index + pc * a.index_stride) : pc;
    const uint8_t *rep = a.replies + pc * a.reply_stride;
    const uint8_t *key = a.keys + i * a.keysize;
    const uint8_t found = rep[0];
    const T v = *reinterpret_cast<const T *>(rep + a.head + a.value_offset + (u64)(l < a.np ? l : 0) * P);
    bool differ = false;
    for (u32 c = l; c < a.keysize; c += G) differ |= rep[a.head + c] != key[c];
    const bool collide = (__ballot(differ) & gmask) != 0;
    const bool ok = found && !collide && p < a.m;
    if (ok) {
      uint8_t *d = a.values + i * a.value_stride;
      if (l < a.np) *reinterpret_cast<T *>(d + (u64)l * P) = v;
      const uint8_t *s = rep + a.head + a.value_offset;
      for (u32 c = l + 64; c < a.np; c += 64)
        *reinterpret_cast<T *>(d + (u64)c * P) = *reinterpret_cast<const T *>(s + (u64)c * P);
    }
    if (l == 0 && p < a.m) a.status[i] = !found ? 2 : collide ? 3 : 0;
  }
}

}  // namespace pdht
