/*
 * pdht_hip_table_keys_rmw.h -- update, insert-if-absent and compare-and-swap
 * by KEY on the device-resident target table of pdht_hip_table.h, for a
 * caller whose keys and values already lie on the table's device: the write
 * operations that the reference's applications use by key (the claim of a
 * k-mer, pdht_atomic_cswap, bench/Meraculous/UU_traversal_final.h:252; the
 * write-back, pdht_update, :444; the build with the Portals put, which is
 * insert-if-absent, libpdht/putget.c:244-267), without wire records.  Part of
 * the C-ABI of pdht_hip.h (which includes this header; ABI revision 4, these
 * entry points only add to it) and exported by the same libraries.  It
 * finishes the local route that pdht_hip_table_keys.h began with the put and
 * the get.
 *
 * Each call computes byte for byte what its record route computes at one rank
 * (there the bucketing is stable, so record position = key index):
 *   update_keys: pdht_bucket_put_records_dev(keys, values, nranks = 1,
 *                key_slot) -> pdht_table_update_records_dev
 *   add_keys:    pdht_bucket_put_records_dev(..) -> pdht_table_add_records_dev
 *                without replies
 *   cswap_keys:  pdht_bucket_records_dev(keys, nranks = 1) ->
 *                pdht_table_cswap_dev(mbits = records + 16, the record stride)
 * and keeps no records and no sort.
 *
 * Matching is by mbits = CityHash64(key) alone: the key bytes of a row are
 * not compared, as in the reference (libpdht/atomics.c:81-154, putget.c:278),
 * in the record operations and in pdht_table_put_keys_dev.  An update
 * replaces the whole row, key slot included.  pdht_table_get_keys_dev remains
 * the call that reports a collision.
 *
 * Geometry of update_keys and add_keys, that of pdht_hip_table_keys.h: slot =
 * key_slot ? key_slot : keysize rounded up to 8; key_slot is 0 or a multiple
 * of 8 that is >= keysize; rowbytes must equal slot + elemsize rounded up to
 * 8; keysize is 1 .. 64; keys are packed, m x keysize bytes, at any byte
 * address; values: row i at (char*)values + i*value_stride, any address,
 * value_stride >= elemsize; m < 2^32.  The row of a key is the key, zeros up
 * to slot, the value, zeros up to 8.  The byte paths read whole aligned
 * dwords: up to 3 bytes before the first and after the last byte of keys and
 * values are read (never written) when those are not 4-byte aligned.
 * cswap_keys has no slot or value geometry: keysize 1 .. 64, m < 2^32, and
 * word_offset, replies and reply_stride as in pdht_table_cswap_dev.
 *
 * mbits_out (may be NULL; 8-byte aligned): mbits_out[i] = CityHash64(key i).
 * workspace (device, 4-byte aligned): its contents on entry do not matter.
 * Every refusal happens on the host before any device call and leaves its
 * message in pdht_hip_last_error(); the table geometry checks of
 * pdht_hip_table.h come first.  m == 0 launches nothing, returns 0 and still
 * names its kernels in pdht_hip_last_kernel().  Calls on one stream are
 * ordered by the stream; concurrent calls on one table from different streams
 * are undefined.  Each call is two kernels with only the kernel boundary
 * between them: nothing blocks, spins or takes a lock, every probe is bounded
 * by the capacity, no host state is kept, and every call can be captured into
 * a graph.  Each call uses the per-slot winner words and takes a batch
 * number: counts4[2] += 1, so it counts among the 2^32 batches (put, update,
 * cswap, inserting accumulate, add, keyed put, keyed update, keyed add, keyed
 * cswap) a table takes between two pdht_table_init_dev calls.
 */
#ifndef PDHT_HIP_TABLE_KEYS_RMW_H_
#define PDHT_HIP_TABLE_KEYS_RMW_H_

#include "pdht_hip.h" /* pdht_hip_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

/* update_keys: overwrites the row under keys[i] with the row of (keys[i],
 * values[i]) when an entry is there, and does nothing otherwise (pdht_update,
 * libpdht/putget.c:278).  Among equal mbits the highest index leaves its row.
 * Nothing is inserted or dropped: of counts4 only [2] moves, by one.
 * status (may be NULL), one uint8 per key: 0 row stored / 1 superseded by a
 * later key of the batch with the same mbits / 3 not found.
 * workspace: pdht_table_update_keys_workspace_bytes(m) = 4*m bytes: the
 * slots between the two kernels.
 * pdht_hip_last_kernel(), P = 16 when rowbytes is a multiple of 16, else 8:
 *   "k_table_locate_keys<last>+k_table_write_keys<P>" */
size_t pdht_table_update_keys_workspace_bytes(size_t m);
int pdht_table_update_keys_dev(void *table, uint64_t capacity, size_t rowbytes,
                               const void *keys, size_t keysize, size_t key_slot,
                               const void *values, size_t elemsize, size_t value_stride,
                               size_t m, void *workspace, size_t workspace_bytes,
                               uint64_t *mbits_out, uint8_t *status,
                               pdht_hip_stream_t stream);

/* add_keys: inserts the row of (keys[i], values[i]) when no entry is under
 * its mbits, and does nothing otherwise (the Portals put: the first wins).
 * Among equal new mbits the lowest index leaves its row; an entry that is
 * present keeps every byte; a new mbits that finds no free slot is dropped
 * under the put's rules (which new mbits lose is left to the schedule, all
 * keys of one mbits share the fate, a present mbits is never dropped).
 * Counters, those of pdht_table_add_records_dev: counts4[0] += entries
 * created, [1] += keys dropped, [3] += slots inspected, [2] += 1.
 * status (may be NULL), one uint8 per key: 0 created by this key / 4 exists,
 * from before or from an earlier key of the batch / 2 dropped, table full.
 * There are no replies: pdht_table_get_keys_dev after the call reads the
 * entries.
 * workspace: pdht_table_add_keys_workspace_bytes(m) = 4*m + m rounded up to
 * 4 bytes (= pdht_table_add_workspace_bytes(m)): the slots and the creator
 * marks between the two kernels.
 * pdht_hip_last_kernel(), P as above:
 *   "k_table_add_claim_keys+k_table_add_write_keys<P>" */
size_t pdht_table_add_keys_workspace_bytes(size_t m);
int pdht_table_add_keys_dev(void *table, uint64_t capacity, size_t rowbytes,
                            const void *keys, size_t keysize, size_t key_slot,
                            const void *values, size_t elemsize, size_t value_stride,
                            size_t m, void *workspace, size_t workspace_bytes,
                            uint64_t *mbits_out, uint8_t *status,
                            pdht_hip_stream_t stream);

/* cswap_keys: compare-and-swap of the uint64 at word_offset (a multiple of 8,
 * <= rowbytes - 8) of the row under every key, as pdht_atomic_cswap would one
 * request after the other in index order: old = word; if word == compare:
 * word = desired.  Among the requests of one mbits only the first can see
 * `compare`.  Nothing is inserted: of counts4 only [2] moves, by one.
 * replies (required for m > 0; 8-byte aligned, reply_stride a multiple of 8
 * and >= 16), reply i for key i, the 16 bytes of pdht_table_cswap_dev: byte 0
 * = 1 found / 0 not found, bytes 1..7 zero, bytes 8..15 the old word (0 when
 * not found).
 * workspace: pdht_table_cswap_keys_workspace_bytes(m) = 4*m bytes.
 * pdht_hip_last_kernel():
 *   "k_table_locate_keys<first>+k_table_cswap" */
size_t pdht_table_cswap_keys_workspace_bytes(size_t m);
int pdht_table_cswap_keys_dev(void *table, uint64_t capacity, size_t rowbytes,
                              const void *keys, size_t keysize, size_t m,
                              size_t word_offset, uint64_t compare, uint64_t desired,
                              void *replies, size_t reply_stride,
                              void *workspace, size_t workspace_bytes,
                              uint64_t *mbits_out, pdht_hip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDHT_HIP_TABLE_KEYS_RMW_H_ */
