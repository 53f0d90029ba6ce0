/*
 * pdht_hip_table.h -- the owner's side of a put and a get: a device-resident
 * target table keyed by the 64-bit match bits, with batch put, get and the
 * client's resolve.  Part of the C-ABI of pdht_hip.h (which includes this
 * header; ABI revision 4, these entry points only add to it) and exported by
 * the same libraries.
 *
 * The reference's owner is the server loop of libmpipdht/init.c:173-290 over
 * a table keyed by mbits (ht_t, libmpipdht/pdht.h:110-116):
 *   put  (init.c:223-241)  find by mbits, insert if absent, then overwrite the
 *                          entry with the PDHT_MAXKEYSIZE + elemsize bytes
 *                          behind the header;
 *   get  (init.c:192-220)  find by mbits, reply {status, key slot, value}
 *                          (reply_t, pdht.h:131-135);
 *   client (putget.c:50-59) status 0 is NotFound, a key mismatch Collision,
 *                          otherwise the value is copied out.
 * Here each is one batch call on device memory:
 *   put: pdht_bucket_put_records_dev -> exchange -> pdht_table_put_records_dev
 *   get: pdht_bucket_records_dev (type get) -> exchange -> pdht_table_get_dev
 *        -> exchange back -> pdht_get_resolve_dev
 *
 * The table is ONE caller-owned device buffer of pdht_table_bytes(capacity,
 * rowbytes) bytes, 16-byte aligned; nothing here allocates, and the geometry
 * is passed on every call (the host keeps no state).  It stores opaque rows
 * of rowbytes bytes (a multiple of 8, >= 8, < 2^31) under a uint64 mbits;
 * capacity is a power of two in 64 .. 2^31.  For put records rowbytes is the
 * record stride - 24: the key slot plus the padded value, the bytes the
 * reference's put copies.  The table never hashes: it trusts the mbits of a
 * record at +16 as the server loop does, and reads no other header word.
 * Every uint64 is an ordinary mbits (0, the table's "empty" mark, has a
 * private slot of its own beside the `capacity` ordinary ones).  The layout
 * inside the buffer is private.
 *
 * Calls on one stream are ordered by the stream.  Concurrent calls on the same
 * table from different streams are undefined.  No call here blocks, spins or
 * takes a lock; every probe is bounded by the capacity, so a full table ends
 * the call normally.  All can be captured into a graph.  A table takes 2^32
 * put, update, cswap, inserting-accumulate and add batches, of all kinds
 * together, between two pdht_table_init_dev calls.  The number taken so far
 * is counts4[2] of pdht_table_counts_dev: a long-lived owner reads it and
 * renews the numbers before it reaches 2^32 -- by a rehash into a new table
 * (pdht_hip_table_iter.h: export as records, then one put; the new table
 * starts from the few batches of that put), or by pdht_table_init_dev when
 * the table may be emptied.  Nothing checks the limit: past it the batch
 * number in the winner words wraps, older winner words beat newer ones, and
 * puts are silently lost (status says "superseded" and the row is not
 * written).  How many batches per second an owner applies is unmeasured, so
 * no lifetime in hours is given here.
 */
#ifndef PDHT_HIP_TABLE_H_
#define PDHT_HIP_TABLE_H_

#include "pdht_hip.h" /* pdht_hip_stream_t, the status codes */

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of a table: 64 + (capacity + 1) * (16 + rowbytes).  0 = refused
 * (capacity not a power of two in 64 .. 2^31; rowbytes 0, not a multiple of
 * 8, or >= 2^31). */
size_t pdht_table_bytes(uint64_t capacity, size_t rowbytes);
/* Empties the table (all four counters too); calling it again is "clear". */
int pdht_table_init_dev(void *table, size_t table_bytes, uint64_t capacity,
                        size_t rowbytes, pdht_hip_stream_t stream);

/* ---- put ------------------------------------------------------------------ */
/* Applies m put records (records + p*record_stride; mbits at +16, the row at
 * +24 .. +24+rowbytes; records 8-byte aligned, record_stride a multiple of 8
 * and >= 24 + rowbytes; m < 2^32).  The result equals applying the records
 * one after the other, in position order, to find-or-insert-then-overwrite:
 * among records of the batch with equal mbits the one at the highest position
 * leaves its row, an mbits already present is overwritten, and the stored
 * rows do not depend on how the waves were scheduled.
 * status (may be NULL), one uint8 per record:
 *   0  this record's row is in the table
 *   1  superseded by a later record of the same batch
 *   2  dropped: new mbits and no free slot left
 * A record whose mbits is present is never dropped.  When a batch brings more
 * new mbits than there are free slots, which of them are dropped is the one
 * thing left to the schedule; all records of one mbits share that fate.
 * workspace: pdht_table_put_workspace_bytes(m) = 4*m bytes (device, 4-byte
 * aligned), the slot of every record between the two kernels
 * (pdht_hip_last_kernel(): "k_table_claim+k_table_write<16>"). */
size_t pdht_table_put_workspace_bytes(size_t m);
int pdht_table_put_records_dev(void *table, uint64_t capacity, size_t rowbytes,
                               const void *records, size_t record_stride, size_t m,
                               void *workspace, size_t workspace_bytes,
                               uint8_t *status, pdht_hip_stream_t stream);

/* ---- get ------------------------------------------------------------------ */
/* head + rowbytes; 0 = refused (head not 1 or 8, or a rowbytes that
 * pdht_table_bytes refuses). */
size_t pdht_table_reply_bytes(size_t head, size_t rowbytes);
/* Answers m requests.  The mbits of request p is the uint64 at (char*)mbits +
 * p*mbits_stride (8-byte aligned, stride a multiple of 8): stride 8 is a dense
 * array, stride = record stride with mbits = records + 16 reads get records in
 * place.  Reply p at (char*)replies + p*reply_stride (reply_stride >= head +
 * rowbytes):
 *   byte 0                     1 found, 0 not found
 *   bytes 1 .. head-1          zero
 *   bytes head .. head+rowbytes-1   the row when found, zeros otherwise
 * Every one of these bytes is defined on return; bytes of the stride beyond
 * them are not written.  head = 1 with key slot 32 is byte for byte reply_t +
 * value (init.c:195-219), at any address and byte alignment (byte pieces);
 * head = 8 is the aligned form: with replies 8-byte aligned and reply_stride a
 * multiple of 8 it moves 8- or 16-byte pieces ("k_table_get<8>", "<16>"),
 * byte pieces otherwise ("k_table_get_bytes").  Repeated mbits are allowed. */
int pdht_table_get_dev(const void *table, uint64_t capacity, size_t rowbytes,
                       const void *mbits, size_t mbits_stride, size_t m,
                       void *replies, size_t reply_stride, size_t head,
                       pdht_hip_stream_t stream);

/* counts4[0..3] (device, 8-byte aligned) = entries stored / records dropped,
 * cumulative / batches that used the winner words (put, the update and
 * cswap of pdht_hip_table_rmw.h, the inserting accumulate of
 * pdht_hip_table_acc.h, the add of pdht_hip_table_add.h, the keyed put of
 * pdht_hip_table_keys.h and the keyed update, add and cswap of
 * pdht_hip_table_keys_rmw.h) / slots inspected by puts, inserting accumulates,
 * adds, keyed puts and keyed adds, cumulative (a retry on one slot after a lost
 * compare-and-swap is not a new slot). */
int pdht_table_counts_dev(const void *table, uint64_t *counts4, pdht_hip_stream_t stream);

/* ---- resolve (client side) ------------------------------------------------ */
/* putget.c:50-59 over a batch of m replies that came back in bucket order.
 * For reply p (at replies + p*reply_stride), i = index ? the uint32 at
 * (char*)index + p*index_stride : p (index rules of the row movers,
 * pdht_hip_put.h: in place from the client's own records at +12):
 *   status[i] = 2 (PdhtStatusNotFound)   reply byte 0 is 0
 *               3 (PdhtStatusCollision)  the keysize bytes at reply + head
 *                                        differ from keys + i*keysize
 *               0 (PdhtStatusOK)         otherwise; then values row i (at
 *                                        values + i*value_stride) receives the
 *                                        elemsize bytes at reply + head +
 *                                        value_offset (the key slot)
 * (pdht_status_t, pdht.h:199-204).  Rows of values whose status is not 0 keep
 * their bytes.  The indices must be distinct.  Any alignment works; values
 * move in pieces of the widest of 16 / 8 / 4 / 1 bytes that fits. */
int pdht_get_resolve_dev(const void *replies, size_t reply_stride, size_t head, size_t value_offset,
                         const void *keys, size_t keysize,
                         const void *index, size_t index_stride, size_t m,
                         void *values, size_t elemsize, size_t value_stride,
                         uint8_t *status, pdht_hip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDHT_HIP_TABLE_H_ */
