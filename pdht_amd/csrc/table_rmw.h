// table_rmw.h -- update and compare-and-swap on the device-resident target table
// (include/pdht_hip_table_rmw.h; layout and the put's two kernels: table.h): pdht_update
// (libpdht/putget.c:278: overwrite an entry that is there, never create one) and pdht_atomic_cswap
// (libpdht/atomics.c:81-154: swap one int64 of the entry, matched by mbits alone), each as one batch
// whose result is that of its records applied one after the other in position order.
//
// Both are two kernels on one stream, the kernel boundary their only synchronisation (nothing spins,
// polls or waits on another lane), with the put's winner words between them:
//   k_table_locate<FIRST>  one lane per record: table_find (no CAS: nothing is inserted), the slot ->
//                          workspace, and on a hit atomicMax of the slot's winner word with
//                          (batch << 32) | (FIRST ? 0xFFFFFFFF - position : position), through
//                          table_win_post of table.h: lanes of a wave with one slot post their maximum once.
//                          batch = counters[2] as the call found it, as in k_table_claim: winner words
//                          of earlier puts, updates and swaps always lose and are never cleared.
//   update:  k_table_write (table.h) with status 3 for a record without a slot: the LAST record of an
//            mbits leaves its row.
//   cswap:   k_table_cswap: the FIRST request of an mbits swaps, the others derive what they would have
//            seen behind it (the argument stands at the kernel).
#pragma once
#include "table.h"

namespace pdht {

struct LocateArgs {
  TableGeom t;
  const uint8_t *mbits;  // u64 at mbits + p * mbits_stride
  u64 mbits_stride;
  u64 m;
  u32 *slots;
};

template <bool FIRST>
__global__ __launch_bounds__(kBlock) void k_table_locate(const LocateArgs a) {
  const TableGeom &t = a.t;
  const u64 batch = t.counters[2] << 32;  // (only the second kernel of the same call, behind this one, writes it)
  const u32 lane = threadIdx.x & 63;
  const u64 nthreads = (u64)gridDim.x * kBlock;
  const u64 rounds = (a.m + nthreads - 1) / nthreads;  // k_table_claim's shape: whole waves stay together
  u64 p = (u64)blockIdx.x * kBlock + threadIdx.x;
  for (u64 r = 0; r < rounds; ++r, p += nthreads) {
    u32 slot = kTableNoSlot;
    if (p < a.m) {
      slot = table_find(t, *reinterpret_cast<const u64 *>(a.mbits + p * a.mbits_stride));
      a.slots[p] = slot;
    }
    table_win_post<FIRST>(t, slot, p, batch, lane);
  }
}

struct CswapArgs {
  TableGeom t;
  const u32 *slots;
  u64 m;
  u64 word_offset;  // of the swapped word inside a row: a multiple of 8, + 8 <= rowbytes
  u64 compare, desired;
  uint8_t *replies;
  u64 reply_stride;
};

// One lane per request.  Sequentially, request p of a slot whose word holds v0 sees
//   old = v0                              when it is the first request of the slot in the batch,
//   old = (v0 == compare ? desired : v0)  behind it: the first has swapped exactly when v0 == compare,
//                                         and no later request changes the word again (it holds
//                                         `desired`, or a v0 != compare that nobody swaps; with
//                                         compare == desired it never changes at all).
// The first request (the one whose inverted position k_table_locate<true> left in the winner word) loads
// x = v0 and stores `desired` when x == compare.  Every other request of the slot loads the word while
// that store may be in flight and answers x == compare ? desired : x, which is the sequential old
// whichever of the two values the load returns: `compare` means v0 == compare and the first is about to
// swap (old = desired); anything else is an untouched v0 != compare or the `desired` just written, and
// both are the sequential answer as they stand.  The word is one aligned 8-byte access, single-copy
// atomic, so a load returns one of the two values whole: no atomic read-modify-write on the row and no
// device-scope flush inside the kernel.  (Relaxed device-scope atomics, so that the one store and the
// loads that race with it are no data race in the language either; they compile to plain 8-byte
// accesses past the CU's L1.)
// WIDE: one 16-byte reply store (replies and reply_stride multiples of 16), else two 8-byte stores.
template <bool WIDE, bool NT>
__global__ __launch_bounds__(kBlock) void k_table_cswap(const CswapArgs a) {
  const TableGeom &t = a.t;
  const u64 nthreads = (u64)gridDim.x * kBlock;
  u64 p = (u64)blockIdx.x * kBlock + threadIdx.x;
  if (p == 0) t.counters[2] += 1;  // nothing in this kernel reads it
  for (; p < a.m; p += nthreads) {
    const u32 slot = a.slots[p];
    const bool found = slot != kTableNoSlot;
    const u64 s = found ? slot : 0;  // loads without a branch: slot 0's when there is no row
    // the winner word of a slot this batch touched carries this batch's number: the position decides
    const u64 w = t.win[s];
    u64 *word = reinterpret_cast<u64 *>(t.rows + s * t.rowbytes + a.word_offset);
    const u64 x = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool first = found && (u32)w == 0xFFFFFFFFu - (u32)p;
    if (first && x == a.compare)
      __hip_atomic_store(word, a.desired, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const u64 old = !found ? 0 : (first || x != a.compare) ? x : a.desired;
    uint8_t *d = a.replies + p * a.reply_stride;
    if constexpr (WIDE) {
      u32x4 q = {(u32)found, 0u, (u32)old, (u32)(old >> 32)};
      st<NT>(q, reinterpret_cast<u32x4 *>(d));
    } else {
      st<NT>((u64)found, reinterpret_cast<u64 *>(d));
      st<NT>(old, reinterpret_cast<u64 *>(d + 8));
    }
  }
}

// k_table_cswap behind the kernel that left slots and winner words (k_table_locate<true>, or
// k_table_locate_keys of table_keys_rmw.h), on that kernel's grid.  nt: the store policy of the replies.
static void launch_table_cswap(const CswapArgs &c, bool nt, unsigned grid, hipStream_t st) {
  const bool wide = (((uintptr_t)c.replies | c.reply_stride) & 15) == 0;
  if (wide)
    nt ? k_table_cswap<true, true><<<grid, kBlock, 0, st>>>(c) : k_table_cswap<true, false><<<grid, kBlock, 0, st>>>(c);
  else
    nt ? k_table_cswap<false, true><<<grid, kBlock, 0, st>>>(c) : k_table_cswap<false, false><<<grid, kBlock, 0, st>>>(c);
}

}  // namespace pdht
