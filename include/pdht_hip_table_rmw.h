/*
 * pdht_hip_table_rmw.h -- update and compare-and-swap on the device-resident
 * target table of pdht_hip_table.h.  Part of the C-ABI of pdht_hip.h (which
 * includes this header; ABI revision 4, these entry points only add to it) and
 * exported by the same libraries.
 *
 * The reference's applications spend their time in two operations that are
 * neither a put nor a get:
 *   pdht_update         (libpdht/putget.c:278; bench/diff/diff3d.c:396,
 *                       bench/Meraculous/UU_traversal_final.h:444) overwrites
 *                       an entry that is already there and never creates one;
 *   pdht_atomic_cswap   (libpdht/atomics.c:81-154, test/atomic.c:73) swaps one
 *                       int64 at offset + PDHT_MAXKEYSIZE inside the entry,
 *                       matched by mbits alone, and returns what was there: a
 *                       rank claims a k-mer by swapping its `used` flag from
 *                       UNUSED to USED and proceeds only if the old value was
 *                       UNUSED (UU_traversal_final.h:252, :408, :663).
 * Here each is one batch call on device memory, at the owner:
 *   update: pdht_bucket_put_records_dev -> exchange ->
 *           pdht_table_update_records_dev
 *   claim:  pdht_bucket_records_dev -> exchange -> pdht_table_cswap_dev ->
 *           exchange back -> pdht_scatter_rows_dev
 *
 * The sequential contract.  The result of either call -- table, status,
 * replies -- equals applying its records one after the other in position
 * order, byte for byte and on every run: the schedule of the waves decides
 * nothing, so exactly one of the claimants of an entry sees the old value, and
 * it is the first in the batch.  Neither call inserts: an absent mbits stays
 * absent, the entry count (counts4[0]), the dropped count ([1]) and the slots
 * inspected by puts ([3]) keep their values, and no probe is longer than the
 * capacity, so a full table ends the call normally.
 *
 * Both calls use the per-slot winner words of the put and take a batch number
 * from counts4[2], which they advance by one as a put does: counts4[2] of
 * pdht_table_counts_dev is "batches that used the winner words (put, update,
 * cswap)", and a table takes 2^32 such batches, of all three kinds together,
 * between two pdht_table_init_dev calls -- together also with the inserting
 * accumulate of pdht_hip_table_acc.h, the add of pdht_hip_table_add.h,
 * the keyed put of pdht_hip_table_keys.h and the keyed update, add and cswap
 * of pdht_hip_table_keys_rmw.h, which take their batch numbers from
 * the same word.  Calls on one stream
 * are ordered by the stream; concurrent calls on one table from different
 * streams are undefined.  Each call is two kernels with nothing but the kernel boundary
 * between them: nothing blocks, spins or takes a lock, and both can be
 * captured into a graph.
 */
#ifndef PDHT_HIP_TABLE_RMW_H_
#define PDHT_HIP_TABLE_RMW_H_

#include "pdht_hip.h" /* pdht_hip_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- update --------------------------------------------------------------- */
/* Applies m put records (the records, alignment rules, m < 2^32 and the piece
 * rule of pdht_table_put_records_dev) to "find by mbits; if present overwrite
 * the row, else do nothing", one after the other in position order: among the
 * records of a present mbits the one at the highest position leaves its row.
 * status (may be NULL), one uint8 per record:
 *   0  this record's row is in the table
 *   1  superseded by a later record of the same batch
 *   3  not found: the table does not hold the mbits, and still does not
 * (3, not PdhtStatusNotFound = 2: 2 is "dropped" in the put's status, and one
 * status array may collect both kinds of batch).
 * workspace: pdht_table_update_workspace_bytes(m) = 4*m bytes (device, 4-byte
 * aligned), the slot of every record between the two kernels
 * (pdht_hip_last_kernel(): "k_table_locate<last>+k_table_write<16>" when
 * rowbytes and record_stride are multiples of 16 and records + 24 is 16-byte
 * aligned, "...<8>" otherwise). */
size_t pdht_table_update_workspace_bytes(size_t m);
int pdht_table_update_records_dev(void *table, uint64_t capacity, size_t rowbytes,
                                  const void *records, size_t record_stride, size_t m,
                                  void *workspace, size_t workspace_bytes,
                                  uint8_t *status, pdht_hip_stream_t stream);

/* ---- compare-and-swap ----------------------------------------------------- */
/* For each of m requests, in position order:
 *   old = word; if (word == compare) word = desired;
 * on the uint64 at word_offset inside the row of the request's mbits
 * (word_offset a multiple of 8, word_offset + 8 <= rowbytes; for a put
 * record's row it is key slot + offset, the reference's offset +
 * PDHT_MAXKEYSIZE).  compare and desired are per call: every claimant swaps
 * the same pair.  So, for compare != desired, request p performed the swap
 * exactly when its old == compare, and among the requests of one mbits that is
 * the one at the lowest position or none.  No other byte of any row changes.
 * The mbits of request p is the uint64 at (char*)mbits + p*mbits_stride (the
 * rules of pdht_table_get_dev: stride 8 is a dense array, stride = record
 * stride with mbits = records + 16 reads records in place).
 * Reply p is 16 bytes at (char*)replies + p*reply_stride (replies 8-byte
 * aligned, reply_stride a multiple of 8 and >= 16):
 *   byte 0         1 found, 0 not found
 *   bytes 1 .. 7   zero
 *   bytes 8 .. 15  old (uint64); 0 when not found
 * -- byte for byte a head-8 reply of pdht_table_get_dev whose row is that one
 * word, so the replies travel back and into the caller's order as get replies
 * do.  Bytes of the stride beyond 16 are not written.
 * workspace: pdht_table_cswap_workspace_bytes(m) = 4*m bytes (device, 4-byte
 * aligned) (pdht_hip_last_kernel(): "k_table_locate<first>+k_table_cswap"). */
size_t pdht_table_cswap_workspace_bytes(size_t m);
int pdht_table_cswap_dev(void *table, uint64_t capacity, size_t rowbytes,
                         const void *mbits, size_t mbits_stride, size_t m,
                         size_t word_offset, uint64_t compare, uint64_t desired,
                         void *replies, size_t reply_stride,
                         void *workspace, size_t workspace_bytes,
                         pdht_hip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDHT_HIP_TABLE_RMW_H_ */
