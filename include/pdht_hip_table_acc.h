/*
 * pdht_hip_table_acc.h -- the associative accumulate on the device-resident
 * target table of pdht_hip_table.h.  Part of the C-ABI of pdht_hip.h (which
 * includes this header; ABI revision 4, these entry points only add to it) and
 * exported by the same libraries.
 *
 * pdht_acc(dht, key, type, op, value) (libpdht/pdht.h:349, AssocOpAdd with
 * IntType / LongType / DoubleType, pdht.h:282-295) is declared by the
 * reference and left a stub (libpdht/assoc.c:26-29): a Portals target cannot
 * add into a matched entry.  A table in device memory can, for a whole batch
 * in one call at the owner:
 *   pdht_bucket_put_records_dev -> exchange -> pdht_table_acc_records_dev
 * -- counting k-mers (bench/Meraculous) and summing contributions into a tree
 * node (bench/diff) are both "find the entry, add to some of its words".
 *
 * The sequential contract.  The result of a call -- table and status -- equals
 * applying its records one after the other in position order:
 *   flags 0           find by mbits; if present, region[k] += record's
 *                     region[k] for every k, and no other byte of the row
 *                     changes; if absent nothing happens (status 3).  Nothing
 *                     is inserted or dropped, the winner words are not used
 *                     and no batch number is taken: all four counters of
 *                     pdht_table_counts_dev keep their values.
 *   PDHT_ACC_INSERT   find-or-insert.  An absent mbits is created with the
 *                     whole row of its FIRST record in the batch -- key slot
 *                     and value, as a put would store it -- and every later
 *                     record of that mbits adds its region; a present mbits
 *                     only accumulates.  A new mbits that finds no free slot
 *                     is dropped (status 2) under the rules of
 *                     pdht_table_put_records_dev: present mbits are never
 *                     dropped, all records of one mbits share one fate, which
 *                     new mbits lose is left to the schedule, and the number
 *                     inserted is min(new distinct mbits, free slots).
 *                     counts4[0], [1] and [3] advance as a put advances them,
 *                     and counts4[2] by one: the call takes a batch number
 *                     ("batches that used the winner words": put, update,
 *                     cswap, the inserting accumulate, the add of
 *                     pdht_hip_table_add.h, the keyed put of
 *                     pdht_hip_table_keys.h and the keyed update, add and
 *                     cswap of pdht_hip_table_keys_rmw.h).
 * The region is `elems` elements of `datatype` at value_offset inside the row,
 * at the same place in the record's row (record + 24) and in the table's row.
 *
 * Integers (PDHT_ACC_INT32, PDHT_ACC_INT64) wrap modulo 2^32 / 2^64.  That
 * arithmetic is associative and commutative, so table and status are
 * byte-exact against the sequential order and the same on every run, whatever
 * the schedule of the waves.
 *
 * Doubles (PDHT_ACC_DOUBLE) are the one exception to "byte for byte": the
 * additions into one word happen in an order the schedule picks, and
 * floating-point addition is not associative, so the last bits of a sum may
 * differ from the position-order sum and from run to run.  What holds for any
 * order: with n addends x_1 .. x_n of one word, the word's old value among
 * them (+0.0 for an entry the call creates),
 *   |result - exact sum| <= gamma_n * sum |x_i|,
 *   gamma_n = n*u / (1 - n*u),  u = 2^-53,
 * while no partial sum overflows (an order that passes DBL_MAX on the way
 * leaves an infinity even where the exact sum is finite).
 * Sums whose every partial sum is an integer below 2^53 in magnitude are
 * exact and therefore reproducible.  Special values follow IEEE 754 addition
 * in whatever order the schedule picks, in the in-wave sums and in the atomics
 * alike: a word with a NaN among its old value and addends ends NaN (the
 * payload is not specified); +inf without -inf and NaN ends +inf, the
 * mirrored case -inf, both together NaN; addends of one sign whose exact sum
 * passes DBL_MAX end in that infinity.  Subnormals are not flushed, neither as
 * addends nor as results: every double is a multiple of 2^-1074, and words
 * whose sum |x_i| stays below 2^53 * 2^-1074 add exactly -- down to an exact
 * +0.0 and up across 2^-1022 into the normals.  The sign of a zero: adding into a present
 * entry keeps it as some sequential order would (-0.0 + -0.0 = -0.0); an
 * entry the call creates starts from +0.0, so a created word whose records
 * all carry -0.0 holds +0.0 where the first record's own bytes are -0.0.  A
 * reproducible double sum in general is out of scope.
 * Unmeasured: lanes of a wave add up the addends of one slot ahead of the
 * atomics only while a region has at most 32 elements; from 33 elements on
 * a wave holds one record, and a batch that piles up on one mbits posts one
 * fp64 atomic per record and word on that entry.  What many same-word fp64
 * atomics cost on this part is not known -- a run that posted 15M of them on
 * one word did not finish (EXPERIMENTS.md R12) -- so treat a hot mbits with a
 * double region of more than 32 elements as possibly very slow.  The adds are hardware fp64 atomics: for
 * PDHT_ACC_DOUBLE the table must lie in ordinary (coarse-grained) device
 * memory, as hipMalloc and torch give it -- not in fine-grained, managed or
 * host memory, where that instruction is not performed.
 *
 * Calls on one stream are ordered by the stream; concurrent calls on one
 * table from different streams are undefined.  Nothing blocks, spins or takes
 * a lock, and the call can be captured into a graph: flags 0 is one kernel,
 * PDHT_ACC_INSERT two with nothing but the kernel boundary between them.
 */
#ifndef PDHT_HIP_TABLE_ACC_H_
#define PDHT_HIP_TABLE_ACC_H_

#include "pdht_hip.h" /* pdht_hip_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

/* datatype: the reference's pdht_datatype_t (libpdht/pdht.h:282-289).
 * CharType (3) and BoolType (4) are refused: the reference gives them no
 * meaning, and there are no 8-bit global atomics. */
#define PDHT_ACC_INT32 0  /* IntType    */
#define PDHT_ACC_INT64 1  /* LongType   */
#define PDHT_ACC_DOUBLE 2 /* DoubleType */
/* op: the reference's pdht_oper_t (pdht.h:291-295) */
#define PDHT_ACC_ADD 0 /* AssocOpAdd */
/* flags */
#define PDHT_ACC_INSERT 1u /* create absent entries */

/* Applies m put records (the records, alignment rules and m < 2^32 of
 * pdht_table_put_records_dev: mbits at +16, the row at +24 .. +24 + rowbytes,
 * records 8-byte aligned, record_stride a multiple of 8 and >= 24 + rowbytes)
 * as accumulates, under the contract above.
 * datatype / op: PDHT_ACC_INT32, _INT64 or _DOUBLE / PDHT_ACC_ADD; anything
 * else is refused.  value_offset: a multiple of the element size (4 or 8);
 * elems >= 1; value_offset + elems * size <= rowbytes.  flags: 0 or
 * PDHT_ACC_INSERT; unknown bits are refused.  Every refusal happens on the
 * host before any launch.
 * status (may be NULL), one uint8 per record, the numbering of
 * pdht_table_update_records_dev:
 *   0  added (with PDHT_ACC_INSERT also: the entry was created from, or
 *      behind, this record)
 *   2  dropped: PDHT_ACC_INSERT, a new mbits and no free slot
 *   3  not found: flags 0, the table does not hold the mbits
 * -- no record is ever "superseded" (1).
 * workspace: pdht_table_acc_workspace_bytes(m, flags) bytes (device, 4-byte
 * aligned).  flags 0: 0 bytes, and workspace may be NULL.  PDHT_ACC_INSERT:
 * 4*m bytes of slots and m bytes of creator marks, rounded up to a multiple
 * of 4: 4*m + ((m + 3) & ~3).  Its contents on entry do not matter.
 * pdht_hip_last_kernel() names the form and the type, <T> one of i32, i64,
 * f64:  "k_table_acc<T>"  for flags 0,
 *       "k_table_acc_claim+k_table_acc<T,insert>"  for PDHT_ACC_INSERT. */
size_t pdht_table_acc_workspace_bytes(size_t m, unsigned flags);
int pdht_table_acc_records_dev(void *table, uint64_t capacity, size_t rowbytes,
                               const void *records, size_t record_stride, size_t m,
                               int datatype, int op, size_t value_offset, size_t elems,
                               unsigned flags, void *workspace, size_t workspace_bytes,
                               uint8_t *status, pdht_hip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDHT_HIP_TABLE_ACC_H_ */
