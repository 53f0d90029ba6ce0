// table_add.h -- insert-if-absent on the device-resident target table (include/pdht_hip_table_add.h;
// layout and probes: table.h): the put of the Portals library (libpdht/putget.c:244-267 queue a put, the
// poll thread appends it BEHIND the entries already on the match list, libpdht/poll.c:205-263, so every
// later match reaches the first put of an mbits) as one batch whose result is that of its records applied
// one after the other in position order -- "find by mbits; if absent, insert it with this record's row; if
// present, do nothing".
//
//   k_table_add_claim     one lane per record: table_claim's probe and table_count's counters; the slot and the
//                         creator mark (1: this lane's CAS made the tag) -> workspace; the winner word
//                         takes the FIRST position (table_win_post<true>: 0xFFFFFFFF - p); the status is
//                         written provisionally: 2 without a slot, else 4.  No row byte is touched.
//   k_table_add_write<P>  a lane group per record: only the creator of a slot acts.  It reads the winner
//                         word -- the first record f of the slot --, copies the row of record f (not its
//                         own) and sets status[f] = 0.  One lane advances counters[2].
//   k_table_add_reply<W>  (only with replies) k_table_get<W, .., slots> of table.h: the slot from the workspace
//                         instead of a probe, no tag line is touched.
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
#include "table.h"

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
      bool made;
      slot = table_claim(t, *reinterpret_cast<const u64 *>(a.records + p * a.record_stride + 16), made, n_seen);
      n_new += made;
      n_drop += slot == kTableNoSlot;
      a.slots[p] = slot;
      a.creator[p] = made;
      if (a.status) a.status[p] = slot == kTableNoSlot ? 2 : 4;  // the creator turns the first record's 4 into 0
    }
    table_win_post<true>(t, slot, p, batch, lane);  // the first position
  }
  table_count(t, n_new, n_drop, n_seen);
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

}  // namespace pdht
