/*
 * pdht_hip_table_reduce.h -- reductions on the entries of the device-resident
 * target table of pdht_hip_table.h: the accumulate of pdht_hip_table_acc.h with
 * an operation of the caller's choice, and with replies.  Part of the C-ABI of
 * pdht_hip.h (which includes this header; ABI revision 4, these entry points
 * only add to it) and exported by the same libraries.
 *
 * The reference pairs its sum with a minimum and a maximum wherever it reduces
 * (PdhtReduceOpSum / Min / Max, libpdht/pdht.h:298-300).  At the owner of a
 * table that is "keep the best candidate of a key", "relax a distance", "keep
 * the smallest label", "or a set of flags into an entry" -- one trip,
 *   pdht_bucket_put_records_dev -> exchange -> pdht_table_reduce_records_dev
 *   [-> exchange the replies -> pdht_get_resolve_dev]
 * where get -> combine at the client -> update takes two and is no reduction
 * when two sources touch one key in the same round.
 *
 * The sequential contract.  The result of a call -- table, status and replies
 * -- equals applying its records one after the other in position order:
 *   find by mbits; if present, region[k] = op(region[k], record's region[k])
 *   for every k, and no other byte of the row changes; if absent:
 *   flags 0           nothing happens (status 3).  All four counters of
 *                     pdht_table_counts_dev keep their values.
 *   PDHT_ACC_INSERT   the entry is created with the whole row of this, the
 *                     FIRST, record of the mbits -- key slot and value, as a put
 *                     would store it --, every later record of the mbits applies
 *                     the op; a new mbits that finds no free slot is dropped
 *                     (status 2) under the rules of pdht_table_put_records_dev.
 *                     counts4[0], [1] and [3] advance as a put advances them and
 *                     counts4[2] by one: the call takes a batch number.
 * exactly as pdht_table_acc_records_dev has it, whose region (`elems` elements
 * of `datatype` at value_offset, at the same place in the record's row and in
 * the table's), datatypes, record layout, alignment rules and m < 2^32 these
 * are.
 *
 * The operations:
 *                 PDHT_ACC_INT32 / _INT64          PDHT_ACC_DOUBLE
 *   PDHT_RED_ADD  the accumulate's sum (wraps)     the accumulate's sum: its
 *                                                  any-order bound, its rule on
 *                                                  the table's memory
 *   _MIN, _MAX    SIGNED compare (IntType and      IEEE 754 totalOrder on the
 *                 LongType are signed)             64 bits
 *   _AND, _OR,    bitwise                          refused
 *   _XOR
 * totalOrder for doubles:
 *   -NaN (larger payload first) < -inf < ... < -0.0 < +0.0 < ... < +inf
 *   < +NaN (larger payload last).
 * It agrees with < wherever both operands are non-NaN and unequal, and it is
 * defined for every bit pattern.  The result of a min or max is always one of
 * its operands, bit for bit: a signalling NaN is not quieted, a subnormal is not
 * flushed, -0.0 and +0.0 are different values (-0.0 the smaller), and a NaN is
 * an ordinary value at the end its sign puts it.  No hardware floating-point
 * min / max semantics enter the contract; only integer instructions touch the
 * bits.
 *
 * Byte-exactness.  Min, max and the bitwise operations are associative and
 * commutative and only select or combine bits, so for every type, doubles
 * included, table, status and replies are byte for byte those of the sequential
 * order and the same on every run, whatever the schedule of the waves.
 * PDHT_RED_ADD on doubles remains the one exception, as in
 * pdht_hip_table_acc.h.  Every operation but that one is an integer atomic:
 * the restriction to ordinary (coarse-grained) device memory applies to
 * PDHT_RED_ADD on doubles only.
 *
 * Replies (optional).  Reply p is byte for byte the head-8 reply that
 * pdht_table_get_dev would give for record p's mbits after the call: byte 0 =
 * 1, bytes 1..7 zero and the entry's row -- the reduced region in it, which
 * tells a caller who proposed a minimum whether its proposal won --, or byte 0
 * = 0 and zeros for a record with status 2 or 3.  For
 * pdht_get_resolve_dev behind an exchange, as the replies of
 * pdht_table_add_records_dev, whose form and alignment rules they have.
 *
 * Calls on one stream are ordered by the stream; concurrent calls on one
 * table from different streams are undefined.  Nothing blocks, spins or takes
 * a lock, and the call can be captured into a graph: one kernel for flags 0,
 * two with PDHT_ACC_INSERT, one more with replies, with nothing but the kernel
 * boundaries between them.
 */
#ifndef PDHT_HIP_TABLE_REDUCE_H_
#define PDHT_HIP_TABLE_REDUCE_H_

#include "pdht_hip.h"           /* pdht_hip_stream_t */
#include "pdht_hip_table_acc.h" /* PDHT_ACC_INT32 / _INT64 / _DOUBLE, PDHT_ACC_INSERT */

#ifdef __cplusplus
extern "C" {
#endif

/* op */
#define PDHT_RED_ADD 0 /* PdhtReduceOpSum; PDHT_ACC_ADD */
#define PDHT_RED_MIN 1 /* PdhtReduceOpMin */
#define PDHT_RED_MAX 2 /* PdhtReduceOpMax */
#define PDHT_RED_AND 3
#define PDHT_RED_OR 4
#define PDHT_RED_XOR 5

/* Bytes of workspace (device, 4-byte aligned; contents on entry do not matter):
 *   flags 0 without replies   0, and workspace may be NULL
 *   flags 0 with replies      4*m  (the slot of every record)
 *   PDHT_ACC_INSERT           4*m + ((m + 3) & ~3), with or without replies
 *                             (slots and creator marks) */
size_t pdht_table_reduce_workspace_bytes(size_t m, unsigned flags, int with_replies);

/* Applies m put records as reductions under the contract above.  table ..
 * record_stride, m, datatype, value_offset, elems, flags, status: as
 * pdht_table_acc_records_dev; status (may be NULL): 0 applied / 2 dropped /
 * 3 not found.  op: PDHT_RED_ADD .. PDHT_RED_XOR; anything else, and
 * PDHT_RED_AND / _OR / _XOR with PDHT_ACC_DOUBLE, is refused.
 * workspace: pdht_table_reduce_workspace_bytes(m, flags, replies != NULL)
 * bytes.  replies (may be NULL: none; reply_stride is then not looked at): m
 * replies of 8 + rowbytes bytes, 8-byte aligned, reply_stride a multiple of 8
 * and >= 8 + rowbytes; bytes between the replies are not written.
 * Every refusal happens on the host before any launch.  m == 0 launches
 * nothing.
 * pdht_hip_last_kernel() names the form, <T> one of i32, i64, f64 and <op> one
 * of min, max, and, or, xor:
 *   PDHT_RED_ADD   "k_table_acc<T>" / "k_table_acc_claim+k_table_acc<T,insert>"
 *                  -- the accumulate's kernels
 *   the others     "k_table_acc<T,op>" /
 *                  "k_table_acc_claim+k_table_acc<T,op,insert>"
 *   with replies   "+k_table_add_reply<W>" behind either, W = 16 where replies
 *                  and reply_stride are multiples of 16 and 8 + rowbytes is
 *                  one, else 8. */
int pdht_table_reduce_records_dev(void *table, uint64_t capacity, size_t rowbytes,
                                  const void *records, size_t record_stride, size_t m,
                                  int datatype, int op, size_t value_offset, size_t elems,
                                  unsigned flags, void *workspace, size_t workspace_bytes,
                                  uint8_t *status, void *replies, size_t reply_stride,
                                  pdht_hip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDHT_HIP_TABLE_REDUCE_H_ */
