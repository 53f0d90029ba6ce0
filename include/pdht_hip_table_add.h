/*
 * pdht_hip_table_add.h -- insert-if-absent on the device-resident target
 * table of pdht_hip_table.h: the first record of an mbits wins.  Part of the
 * C-ABI of pdht_hip.h (which includes this header; ABI revision 4, these entry
 * points only add to it) and exported by the same libraries.
 *
 * In the Portals library a put creates and never overwrites: pdht_put and
 * pdht_add (libpdht/putget.c:244-267) both queue the entry, the poll thread
 * appends every arrived put as a new match entry BEHIND the ones already on
 * the active list (libpdht/poll.c:205-263), and matching walks that list in
 * order -- so every later get, update and cswap reaches the entry of the
 * first put of an mbits, and a second put of the same mbits is dead storage.
 * Only the MPI variant overwrites (libmpipdht/init.c:223-241), and
 * pdht_table_put_records_dev mirrors that one.  This call is the other:
 *   create: pdht_bucket_put_records_dev -> exchange ->
 *           pdht_table_add_records_dev [-> exchange back ->
 *           pdht_get_resolve_dev on its replies]
 * -- "create this entry unless it is already there, and leave it alone if it
 * is": a k-mer re-sent after a cswap marked it USED keeps its flag, and many
 * ranks may create one tree node at once.
 *
 * The sequential contract.  The result of a call -- table, status and
 * replies -- equals applying its records one after the other in position
 * order to "find by mbits; if absent, insert it with this record's row; if
 * present, do nothing", byte for byte and the same on every run, whatever the
 * schedule of the waves:
 *   - an mbits present before the call keeps every byte of its row;
 *   - a new mbits gets the whole row of its record at the LOWEST position;
 *   - no later record of the batch changes that row.
 * A new mbits that finds no free slot is dropped under the rules of
 * pdht_table_put_records_dev: a present mbits is never dropped, all records
 * of one mbits share one fate, which of several new mbits lose when the table
 * fills is the one thing left to the schedule, and a batch is never short of
 * stored entries while free slots remain: the number created is min(distinct
 * new mbits, free slots).
 *
 * Counters (pdht_table_counts_dev), the put's rules: counts4[0] += entries
 * created, [1] += records dropped, [3] += slots inspected, and [2] += 1: the
 * call uses the per-slot winner words and takes a batch number, so it counts
 * among the 2^32 batches that used the winner words (put, update, cswap, the
 * inserting accumulate, this add, the keyed put of pdht_hip_table_keys.h
 * and the keyed update, add and cswap of pdht_hip_table_keys_rmw.h)
 * which a table takes between two pdht_table_init_dev calls.
 *
 * Calls on one stream are ordered by the stream; concurrent calls on one
 * table from different streams are undefined.  Nothing blocks, spins or takes
 * a lock, every probe is bounded by the capacity, and the call can be
 * captured into a graph: two kernels, three with replies, with nothing but
 * the kernel boundary between them.
 */
#ifndef PDHT_HIP_TABLE_ADD_H_
#define PDHT_HIP_TABLE_ADD_H_

#include "pdht_hip.h" /* pdht_hip_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

/* Applies m put records (the records, alignment rules, m < 2^32 and the piece
 * rule of pdht_table_put_records_dev: mbits at +16, the row at +24 .. +24 +
 * rowbytes, records 8-byte aligned, record_stride a multiple of 8 and >= 24 +
 * rowbytes; rows move in 16-byte pieces when rowbytes, record_stride and
 * records + 24 are multiples of 16, else in 8-byte pieces) under the contract
 * above.  m == 0 launches nothing and returns 0.  Every refusal happens on
 * the host before any launch.
 * status (may be NULL), one uint8 per record:
 *   0  this record created the entry, and its row is in the table
 *   4  exists: the table already held the mbits -- from before the call or
 *      from an earlier record of this batch -- and that row stands
 *   2  dropped: a new mbits and no free slot left
 * Sequentially a later duplicate of a new mbits finds the entry present, so
 * it is 4 and has no code of its own.  The value 4 is used by no other call,
 * so one status array can collect put (0/1/2), update (0/1/3) and add
 * (0/4/2) batches.
 * replies (may be NULL; reply_stride is then ignored): reply p, 8 + rowbytes
 * bytes at (char*)replies + p*reply_stride, is byte for byte the head-8 reply
 * of a pdht_table_get_dev issued after the call: byte 0 = 1, bytes 1..7 zero,
 * then the row the table holds for the record's mbits -- the record's own
 * when its status is 0, the surviving row when it is 4; for a dropped record
 * byte 0 = 0 and the row bytes are zeros.  So a client learns in one trip
 * whether its create won and what the table holds, and pdht_get_resolve_dev
 * on these replies reports Collision when another key owns the mbits, which
 * a put cannot tell.  Only the aligned form is built, as for
 * pdht_table_cswap_dev: replies 8-byte aligned, reply_stride a multiple of 8
 * and >= 8 + rowbytes, anything else is refused; 16-byte pieces when replies
 * and reply_stride are multiples of 16 and 8 + rowbytes is too, else 8-byte
 * pieces.  Bytes of the stride beyond the reply are not written.  The packed
 * head-1 wire form (reply_t + value) is a pdht_table_get_dev away.
 * workspace: pdht_table_add_workspace_bytes(m) bytes (device, 4-byte aligned):
 * 4*m bytes of slots and m bytes of creator marks rounded up to a multiple of
 * 4, 4*m + ((m + 3) & ~3), the formula of the inserting accumulate.  Its
 * contents on entry do not matter.
 * pdht_hip_last_kernel() names what ran, P and W each 16 or 8:
 *   "k_table_add_claim+k_table_add_write<P>"                       no replies
 *   "k_table_add_claim+k_table_add_write<P>+k_table_add_reply<W>"  replies
 * -- also for m == 0, where nothing is launched. */
size_t pdht_table_add_workspace_bytes(size_t m);
int pdht_table_add_records_dev(void *table, uint64_t capacity, size_t rowbytes,
                               const void *records, size_t record_stride, size_t m,
                               void *workspace, size_t workspace_bytes,
                               uint8_t *status,
                               void *replies, size_t reply_stride,
                               pdht_hip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDHT_HIP_TABLE_ADD_H_ */
