// table_add.h -- insert-if-absent on the device-resident target table (include/pdht_hip_table_add.h;
// layout and probes: table.h): the put of the Portals library (libpdht/putget.c:244-267 queue a put, the
// poll thread appends it BEHIND the entries already on the match list, libpdht/poll.c:205-263, so every
// later match reaches the first put of an mbits) as one batch whose result is that of its records applied
// one after the other in position order -- "find by mbits; if absent, insert it with this record's row; if
// present, do nothing".
//
//   k_table_add_claim     one lane per record: k_table_acc_claim's probe and counters; the slot and the
//                         creator mark (1: this lane's CAS made the tag) -> workspace; the winner word
//                         takes the FIRST position (0xFFFFFFFF - p, two leaders per wave); the status is
//                         written provisionally: 2 without a slot, else 4.  No row byte is touched.
//   k_table_add_write<P>  a lane group per record: only the creator of a slot acts.  It reads the winner
//                         word -- the first record f of the slot --, copies the row of record f (not its
//                         own) and sets status[f] = 0.  One lane advances counters[2].
//   k_table_add_reply<W>  (only with replies) k_table_get<W> with the slot from the workspace instead of a
//                         probe: no tag line is touched.
//   The kernel boundary is the only synchronisation: nothing spins, polls or waits on another lane.
//
// Why the status comes from two kernels: the creator of a slot is whichever lane's CAS came first, in
// general not the first record, and the first record cannot know that its slot is new -- it may have found
// the tag another lane made a moment before.  So every record with a slot says 4 in the first kernel, and
// behind the boundary the creator, who alone knows the slot is new, turns the first record's 4 into 0.
//
// Why the replies are a launch of their own: a record that is not the creator of its new slot would read a
// row that the creator writes in the same launch, and whether a slot is new is known to the creator only.
// Behind k_table_add_write no kernel of the call writes a row, so plain loads are safe.
//
// The tag protocol of table.h holds as it stands: a tag only goes from empty to an mbits through the CAS, a
// stale "empty" is corrected by the CAS, a non-empty tag is final, and every probe counts down from C.
#pragma once
#include "table_acc.h"

namespace pdht {

struct AddClaimArgs {
  TableGeom t;
  const uint8_t *records;
  u64 record_stride;
  u64 m;
  u32 *slots;
  uint8_t *creator;  // 1: this record's CAS created its slot's tag
  uint8_t *status;   // may be null; provisional: 2 dropped, 4 has a slot
};

static __global__ __launch_bounds__(kBlock) void k_table_add_claim(const AddClaimArgs a) {
  const TableGeom &t = a.t;
  const u64 batch = t.counters[2] << 32;  // (only k_table_add_write of the same call, behind this kernel, writes it)
  const u32 lane = threadIdx.x & 63;
  const u64 nthreads = (u64)gridDim.x * kBlock;
  const u64 rounds = (a.m + nthreads - 1) / nthreads;  // whole waves stay together for the wave-wide steps
  u32 n_new = 0, n_drop = 0, n_seen = 0;
  u64 p = (u64)blockIdx.x * kBlock + threadIdx.x;
  for (u64 r = 0; r < rounds; ++r, p += nthreads) {
    u32 slot = kTableNoSlot;
    if (p < a.m) {
      const u64 mb = *reinterpret_cast<const u64 *>(a.records + p * a.record_stride + 16);
      bool made = false;
      if (mb == 0) {
        ++n_seen;
        slot = t.cap;
        made = tag_load(t.tags + t.cap) == 0 && atomicCAS((unsigned long long *)(t.tags + t.cap), 0ull, 1ull) == 0;
      } else {
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
          if (tag == mb) {
            slot = (u32)h;
            break;
          }
          ++h;
        }
        if (slot == kTableNoSlot) ++n_drop;
      }
      n_new += made;
      a.slots[p] = slot;
      a.creator[p] = made;
      if (a.status) a.status[p] = slot == kTableNoSlot ? 2 : 4;  // the creator turns the first record's 4 into 0
    }
    // the first position into the winner word, one atomicMax per slot and wave where lanes share a slot
    // (k_table_locate<true>'s scheme)
    const u32 rank = 0xFFFFFFFFu - (u32)p;
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
  // one atomic per wave per counter
  n_new = wave_sum(n_new), n_drop = wave_sum(n_drop), n_seen = wave_sum(n_seen);
  if (lane == 0) {
    if (n_new) atomicAdd((unsigned long long *)(t.counters + 0), (unsigned long long)n_new);
    if (n_drop) atomicAdd((unsigned long long *)(t.counters + 1), (unsigned long long)n_drop);
    if (n_seen) atomicAdd((unsigned long long *)(t.counters + 3), (unsigned long long)n_seen);
  }
}

struct AddWriteArgs {
  TableGeom t;
  const uint8_t *records;
  u64 record_stride;
  u64 m;
  const u32 *slots;
  const uint8_t *creator;
  uint8_t *status;  // may be null
  u32 np;           // pieces of a row
  u32 gshift;       // log2 of the lane group (G = the power of two >= np, at most 64)
};

// P: 16 or 8 bytes per piece.  Shape of k_table_write: a group's loads of kRowsInFlight records are issued
// ahead of their predicated stores.  A wave none of whose records created a slot -- every wave of a batch
// that finds all its mbits present -- reads the marks and nothing else.
template <int P, bool NT>
__global__ __launch_bounds__(kBlock) void k_table_add_write(const AddWriteArgs a) {
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
      v[r] = *reinterpret_cast<const T *>(a.records + first[r] * a.record_stride + 24 + lo);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) rows_keep(v[r]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!made[r]) continue;
      const uint8_t *s = a.records + first[r] * a.record_stride + 24;
      uint8_t *d = t.rows + (u64)slot[r] * t.rowbytes;
      if (l < a.np) st<NT>(v[r], reinterpret_cast<T *>(d + lo));
      for (u32 c = l + 64; c < a.np; c += 64)  // rows of more pieces than a wave has lanes
        st<NT>(*reinterpret_cast<const T *>(s + (u64)c * P), reinterpret_cast<T *>(d + (u64)c * P));
      if (a.status && l == 0) a.status[first[r]] = 0;
    }
  }
}

struct AddReplyArgs {
  TableGeom t;
  const u32 *slots;
  u64 m;
  uint8_t *replies;
  u64 reply_stride;
  u32 np;      // pieces of a reply: words (1 + B/8) / W
  u32 gshift;  // log2 of the lane group
};

// k_table_get<W> (head 8 on aligned replies: 1 + B/8 words, word 0 the status, a lane moves W = 1 or 2 of
// them) with the slot k_table_add_claim left in the workspace: the row words are loaded without a branch (of
// slot 0 when there is no row) ahead of the predicated stores.
template <int W, bool NT>
__global__ __launch_bounds__(kBlock) void k_table_add_reply(const AddReplyArgs a) {
  const TableGeom &t = a.t;
  const u32 lane = threadIdx.x & 63;
  const u64 wave = (u64)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const u64 nwaves = (u64)gridDim.x * kWavesPerBlock;
  const u32 l = lane & ((1u << a.gshift) - 1), g = lane >> a.gshift, rpi = 64u >> a.gshift;
  const u64 last = a.m - 1;
  const u32 nw = (u32)(t.rowbytes >> 3) + 1;
  for (u64 base = wave * rpi; base < a.m; base += nwaves * rpi) {
    const u64 p = base + g;
    const u32 slot = a.slots[p < last ? p : last];
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

}  // namespace pdht
