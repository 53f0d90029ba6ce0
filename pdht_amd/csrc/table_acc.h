// table_acc.h -- the associative accumulate on the device-resident target table
// (include/pdht_hip_table_acc.h; layout and probes: table.h): pdht_acc (libpdht/pdht.h:349, a stub in
// libpdht/assoc.c:26-29) as one batch whose result is that of its records applied one after the other
// in position order -- "find the entry, add to `elems` words of its row".
//
//   flags 0   k_table_acc<T>          a lane group per record: table_find, then device-scope atomic adds
//                                     of the record's region into the row's, then the status byte.
//                                     No winner words, no counters: one kernel.
//   INSERT    k_table_acc_claim       one lane per record: table_claim's probe and table_count's counters;
//                                     the winner word takes the FIRST position (table_win_post<true>:
//                                     0xFFFFFFFF - p); the lane whose CAS created the tag marks
//                                     its record as the creator and zeroes the region of the new row
//                                     (no other lane touches that row in this kernel).
//             k_table_acc<T, insert>  every record with a slot adds as above; the creator's group reads
//                                     the winner word -- the first record f of the slot -- and copies the
//                                     row bytes OUTSIDE the region from record f: disjoint from the
//                                     atomics, so nothing races.  One lane advances counters[2].
//   The kernel boundary is the only synchronisation: nothing spins, polls or waits on another lane.
//
// Integer sums wrap (unsigned arithmetic throughout), so any order of the adds gives the sequential
// result.  Double sums depend on the order the schedule picks (pdht_hip_table_acc.h has the bound).
//
// Lanes of a wave whose records found the same slot add their addends together first and post one
// atomic per element between them -- table_win_post's leader scheme with a sum in place of the
// maximum: a hot mbits would otherwise queue one atomic per record on one word.
//
// OP (include/pdht_hip_table_reduce.h) puts another operation in the place of the sum: min and max
// (signed for the integers, IEEE 754 totalOrder for doubles) and bitwise and / or / xor (integers only).
// Each is associative and commutative and only selects or combines bits, so any order gives the sequential
// result for every type.  The kernels are the same ones: the in-wave fold uses the op in place of +=, lanes
// without an operand feed its identity, the post is one integer atomic per element, and INSERT starts a new
// row's region from the identity where the sum starts it from zero.  None of them is an fp atomic.
// For replies (k_table_get<W, .., slots> of table.h, a launch behind these) the flags-0 kernel also stores every
// record's slot to the workspace, where k_table_acc_claim leaves it under INSERT.
#pragma once
#include <limits>

#include "table.h"

namespace pdht {

template <class T>
struct AccWord;  // the integer of T's size that moves T's bytes unchanged
template <>
struct AccWord<u32> {
  typedef u32 type;
};
template <>
struct AccWord<u64> {
  typedef u64 type;
};
template <>
struct AccWord<double> {
  typedef u64 type;
};

// device-scope, no return value used: one global atomic add instruction each (fp64: -munsafe-fp-atomics)
__device__ __forceinline__ void acc_add(u32 *p, u32 v) { atomicAdd(p, v); }
__device__ __forceinline__ void acc_add(u64 *p, u64 v) {
  atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}
__device__ __forceinline__ void acc_add(double *p, double v) { atomicAdd(p, v); }

// What a lane without an addend feeds the in-wave sums: x + neutral == x bit for bit.  For doubles that is
// -0.0 (x + +0.0 would turn a sum of -0.0s into +0.0).
template <class T>
__device__ __forceinline__ T acc_neutral() {
  if constexpr (sizeof(T) == 8 && !std::is_integral<T>::value)
    return -0.0;
  else
    return T(0);
}

__device__ __forceinline__ u32 acc_shfl_xor(u32 v, int o) { return (u32)__shfl_xor((int)v, o); }
__device__ __forceinline__ u64 acc_shfl_xor(u64 v, int o) {
  return (u64)__shfl_xor((unsigned long long)v, o);
}
__device__ __forceinline__ double acc_shfl_xor(double v, int o) { return __shfl_xor(v, o); }
__device__ __forceinline__ int acc_shfl_xor(int v, int o) { return __shfl_xor(v, o); }
__device__ __forceinline__ long long acc_shfl_xor(long long v, int o) { return __shfl_xor(v, o); }

// The operations (PDHT_RED_* of include/pdht_hip_table_reduce.h; kRedAdd is the accumulate's sum)
constexpr int kRedAdd = 0, kRedMin = 1, kRedMax = 2, kRedAnd = 3, kRedOr = 4, kRedXor = 5;

template <class T>
struct AccKey;  // the signed integer of T's size that min, max and the bitwise ops work on
template <>
struct AccKey<u32> {
  typedef int type;
};
template <>
struct AccKey<u64> {
  typedef long long type;
};
template <>
struct AccKey<double> {
  typedef long long type;
};

// The bits of a double <-> a signed key whose integer order is IEEE 754 totalOrder (-NaN < -inf < .. < -0.0
// < +0.0 < .. < +inf < +NaN): the sign bit set turns the other 63 bits over.  The map is its own inverse,
// and only integer instructions touch the bits: a signalling NaN stays one, a subnormal is not flushed.
__device__ __forceinline__ long long f64_key(long long b) { return b ^ (long long)((u64)(b >> 63) >> 1); }

// What the kernel does with an operand: load it (as V), fold two of them, feed the fold from a lane that
// has none, and post the result on the entry's word.  The sum is the accumulate's own code.
template <class T, int OP>
struct Red {
  typedef typename AccKey<T>::type V;
  static constexpr bool kF64 = !std::is_integral<T>::value;
  static_assert(OP == kRedMin || OP == kRedMax || (!kF64 && (OP == kRedAnd || OP == kRedOr || OP == kRedXor)),
                "min and max for every type, and / or / xor for the integers");
  static __device__ __forceinline__ V load(const T *p) {
    const V b = *reinterpret_cast<const V *>(p);
    if constexpr (kF64)
      return f64_key(b);
    else
      return b;
  }
  static __device__ __forceinline__ V neutral() {  // op(x, neutral) == x
    if constexpr (OP == kRedMin)
      return std::numeric_limits<V>::max();
    else if constexpr (OP == kRedMax)
      return std::numeric_limits<V>::min();
    else if constexpr (OP == kRedAnd)
      return V(-1);
    else
      return V(0);
  }
  static __device__ __forceinline__ V fold(V x, V y) {
    if constexpr (OP == kRedMin)
      return y < x ? y : x;
    else if constexpr (OP == kRedMax)
      return y > x ? y : x;
    else if constexpr (OP == kRedAnd)
      return x & y;
    else if constexpr (OP == kRedOr)
      return x | y;
    else
      return x ^ y;
  }
  // One device-scope integer atomic, no return value used.
  // Doubles: the operand's bits b go to the word w as an integer atomic picked by b's sign alone --
  //   max, b's sign clear: signed max.   w's sign clear: signed order is totalOrder among the non-negative
  //                        patterns.  w's sign set: w is negative as an integer, b wins, and totalOrder puts
  //                        every sign-set pattern below every sign-clear one.
  //   max, b's sign set:   unsigned min.  w's sign set: among the sign-set patterns totalOrder is the
  //                        reverse of the unsigned order (a larger magnitude is further down), so the
  //                        unsigned minimum is the maximum.  w's sign clear: w < 2^63 <= b unsigned, w stays,
  //                        and w is above b in totalOrder.
  //   min, b's sign clear: signed min.   w's sign clear: as the first case.  w's sign set: w is negative as
  //                        an integer and stays; it is below b in totalOrder.
  //   min, b's sign set:   unsigned max.  w's sign set: the reversed order again, the unsigned maximum is
  //                        the minimum.  w's sign clear: b >= 2^63 > w unsigned, b wins; it is below w.
  // The result is always one operand's bits.
  static __device__ __forceinline__ void post(T *p, V v) {
    if constexpr (kF64) {
      const long long b = f64_key(v);
      long long *s = reinterpret_cast<long long *>(p);
      unsigned long long *u = reinterpret_cast<unsigned long long *>(p);
      if constexpr (OP == kRedMax) {
        if (b < 0)
          atomicMin(u, (unsigned long long)b);
        else
          atomicMax(s, b);
      } else {
        if (b < 0)
          atomicMax(u, (unsigned long long)b);
        else
          atomicMin(s, b);
      }
    } else if constexpr (sizeof(T) == 4) {
      if constexpr (OP == kRedMin)
        atomicMin(reinterpret_cast<int *>(p), v);
      else if constexpr (OP == kRedMax)
        atomicMax(reinterpret_cast<int *>(p), v);
      else if constexpr (OP == kRedAnd)
        atomicAnd(reinterpret_cast<unsigned *>(p), (unsigned)v);
      else if constexpr (OP == kRedOr)
        atomicOr(reinterpret_cast<unsigned *>(p), (unsigned)v);
      else
        atomicXor(reinterpret_cast<unsigned *>(p), (unsigned)v);
    } else {
      if constexpr (OP == kRedMin)
        atomicMin(reinterpret_cast<long long *>(p), v);
      else if constexpr (OP == kRedMax)
        atomicMax(reinterpret_cast<long long *>(p), v);
      else if constexpr (OP == kRedAnd)
        atomicAnd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
      else if constexpr (OP == kRedOr)
        atomicOr(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
      else
        atomicXor(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
    }
  }
};
template <class T>
struct Red<T, kRedAdd> {
  typedef T V;
  static __device__ __forceinline__ V load(const T *p) { return *p; }
  static __device__ __forceinline__ V neutral() { return acc_neutral<T>(); }
  static __device__ __forceinline__ V fold(V x, V y) { return x + y; }
  static __device__ __forceinline__ void post(T *p, V v) { acc_add(p, v); }
};

// The 64 bits a new row's region starts from under INSERT (k_table_acc_claim's fill; 32-bit types: the
// pattern twice): op(identity, x) == x, so "the first record's region, then the later records" is every
// record applying the op.  Doubles: the bits of the key-space extreme, the last of totalOrder for min and
// the first for max.  size: of an element; f64: a double.
static inline u64 red_identity_bits(int op, size_t size, bool f64) {
  switch (op) {
    case kRedMin:  // INT_MAX of the width; the double's is the same pattern as the 64-bit integer's
      return size == 4 ? 0x7FFFFFFF7FFFFFFFull : 0x7FFFFFFFFFFFFFFFull;
    case kRedMax:
      return size == 4 ? 0x8000000080000000ull : f64 ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull;
    case kRedAnd:
      return 0xFFFFFFFFFFFFFFFFull;
    default:
      return 0;
  }
}

struct AccClaimArgs {
  TableGeom t;
  const uint8_t *records;
  u64 record_stride;
  u64 m;
  u32 *slots;
  uint8_t *creator;  // 1: this record's CAS created its slot's tag
  u64 value_offset;  // of the region inside a row (a multiple of 4)
  u64 region_words;  // its length in 32-bit words
  u32 fill[2];       // what a new row's region starts from, by the parity of the word (0: the sum's zero)
};

static __global__ __launch_bounds__(kBlock) void k_table_acc_claim(const AccClaimArgs a) {
  const TableGeom &t = a.t;
  const u64 batch = t.counters[2] << 32;  // (only k_table_acc of the same call, behind this kernel, writes it)
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
      if (made) {  // a new entry starts from the op's identity, the sums from zero: every record of it
        // applies the op, the first included
        u32 *z = reinterpret_cast<u32 *>(t.rows + (u64)slot * t.rowbytes + a.value_offset);
        for (u64 c = 0; c < a.region_words; ++c) z[c] = a.fill[c & 1];
      }
    }
    table_win_post<true>(t, slot, p, batch, lane);  // the first position
  }
  table_count(t, n_new, n_drop, n_seen);
}

struct AccArgs {
  TableGeom t;
  const uint8_t *records;
  u64 record_stride;
  u64 m;
  const u32 *slots;        // INSERT: k_table_acc_claim's
  const uint8_t *creator;  // INSERT
  uint8_t *status;         // may be null
  u64 value_offset;        // of the region inside a row (a multiple of sizeof(T))
  u64 elems;               // elements of T in the region
  u32 gshift;              // log2 of the lane group (G = the power of two >= elems, at most 64)
  u32 *slot_out;           // flags 0, may be null: every record's slot or kTableNoSlot, for the reply kernel
};

// T: u32, u64 (two's complement sums of either signedness) or double.  A group of G lanes per record,
// lane l of it element l; 64 / G records per wave instruction.  COMBINE: the in-wave sums (the product's
// form; the A/B alternative posts every addend on its own).  OP: the sum, or one of Red's operations.
template <class T, bool INSERT, bool COMBINE, int OP = kRedAdd>
__global__ __launch_bounds__(kBlock) void k_table_acc(const AccArgs a) {
  typedef typename AccWord<T>::type W;
  typedef Red<T, OP> R;
  typedef typename R::V V;
  const TableGeom &t = a.t;
  const u32 lane = threadIdx.x & 63;
  const u64 wave = (u64)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const u64 nwaves = (u64)gridDim.x * kWavesPerBlock;
  if (INSERT && wave == 0 && lane == 0) t.counters[2] += 1;  // nothing in this kernel reads it
  const u32 G = 1u << a.gshift, l = lane & (G - 1), g = lane >> a.gshift, rpi = 64u >> a.gshift;
  for (u64 base = wave * rpi; base < a.m; base += nwaves * rpi) {  // (base is wave-uniform)
    const u64 p = base + g;
    const bool live = p < a.m;
    u32 slot = kTableNoSlot;
    if (live) {
      if constexpr (INSERT)
        slot = a.slots[p];
      else
        slot = table_find(t, *reinterpret_cast<const u64 *>(a.records + p * a.record_stride + 16));
    }
    const bool has = slot != kTableNoSlot;
    const T *add = reinterpret_cast<const T *>(a.records + (live ? p : 0) * a.record_stride + 24 + a.value_offset);
    T *sum = reinterpret_cast<T *>(t.rows + (u64)(has ? slot : 0) * t.rowbytes + a.value_offset);
    if (a.elems <= G) {  // (wave-uniform)
      const bool on = has && l < a.elems;
      const V v = on ? R::load(add + l) : R::neutral();
      bool todo = on;
      if (COMBINE && rpi > 1) {
        bool cand = has;  // a group's lanes stand and fall together
#pragma unroll
        for (int k = 0; k < kLocateLeaders; ++k) {
          const u64 open = __ballot(cand);
          if (!open) break;  // (wave-uniform)
          const u32 leader = (u32)__ffsll((unsigned long long)open) - 1;  // lane 0 of its group
          const u32 s = (u32)__shfl((int)slot, (int)leader);
          const bool mine = cand && slot == s;
          cand = cand && !mine;
          if ((u32)__popcll(__ballot(mine)) <= G) continue;  // (wave-uniform) one group: its own atomics below
          V part = mine ? v : R::neutral();  // (v is neutral in the lanes past the region)
          for (u32 o = 32; o >= G; o >>= 1) part = R::fold(part, acc_shfl_xor(part, (int)o));  // over the groups, element by element
          if (mine && g == (leader >> a.gshift) && l < a.elems) R::post(sum + l, part);
          todo = todo && !mine;
        }
      }
      if (todo) R::post(sum + l, v);
    } else if (has) {  // more elements than a wave has lanes: G = 64, one record per wave
      for (u64 c = l; c < a.elems; c += 64) R::post(sum + c, R::load(add + c));
    }
    if constexpr (INSERT) {
      if (has && a.creator[p]) {  // (has implies live)
        // the winner word of a slot this batch created carries this batch's number and its first position
        const u64 f = 0xFFFFFFFFu - (u32)t.win[slot];
        const W *src = reinterpret_cast<const W *>(a.records + f * a.record_stride + 24);
        W *dst = reinterpret_cast<W *>(t.rows + (u64)slot * t.rowbytes);
        const u64 lo = a.value_offset / sizeof(T), hi = lo + a.elems, n = t.rowbytes / sizeof(T);
        for (u64 c = l; c < n; c += G)
          if (c < lo || c >= hi) dst[c] = src[c];
      }
    }
    if (a.status && l == 0 && live) a.status[p] = has ? 0 : INSERT ? 2 : 3;
    if constexpr (!INSERT) {
      if (a.slot_out && l == 0 && live) a.slot_out[p] = slot;
    }
  }
}

}  // namespace pdht
