/*
 * pdht_hip_table_keys.h -- put and get by KEY on the device-resident target
 * table of pdht_hip_table.h, for a caller whose keys and values already lie on
 * the table's device: hash, probe and move rows without wire records.  Part
 * of the C-ABI of pdht_hip.h (which includes this header; ABI revision 4,
 * these entry points only add to it) and exported by the same libraries.
 *
 * Every other operation of the table is reached through records, because a
 * record is what travels between ranks.  When sender and owner are one device
 * (a one-GPU user, a world of one rank, a rehash whose caller kept the keys)
 * the record route is
 *   put: pdht_bucket_put_records_dev(nranks = 1) -> pdht_table_put_records_dev
 *   get: pdht_bucket_records_dev(nranks = 1) -> pdht_table_get_dev(head 8) ->
 *        pdht_get_resolve_dev(value_offset = slot)
 * -- a counting sort into one bucket, a record buffer of 24 + rowbytes bytes
 * per key that is written once and read twice, a reply buffer, and headers
 * that mean nothing.  The two calls below compute byte for byte what that
 * route computes and keep no records, no replies and no sort.
 *
 * Geometry, that of pdht_hip_put.h: slot = key_slot ? key_slot : keysize
 * rounded up to 8; key_slot is 0 or a multiple of 8 that is >= keysize; the
 * table's rowbytes must equal slot + elemsize rounded up to 8, which is
 * pdht_bucket_put_record_bytes(keysize, key_slot, elemsize) - 24; anything
 * else is refused.  The row of a key is the key, zeros up to slot, the value,
 * zeros up to 8.  keysize is 1 .. 64 (the three short branches of CityHash64;
 * the reference's PDHT_MAXKEYSIZE is 32); longer keys are refused and keep the
 * record route.  keys are packed, m x keysize bytes, at any byte address: keys
 * of 8 bytes on an 8-byte boundary, and of 16, 32 or 64 bytes on a 16-byte
 * one, are read in vector loads, anything else as aligned dword runs.  values:
 * row i at (char*)values + i*value_stride, any address, value_stride >=
 * elemsize.  m < 2^32.  Like the hash kernels, the byte paths read whole
 * aligned dwords: up to 3 bytes before the first and after the last byte of
 * keys and values are read (never written) when those are not 4-byte aligned.
 *
 * Every refusal happens on the host before any device call and leaves its
 * message in pdht_hip_last_error(); the table geometry checks of
 * pdht_hip_table.h come first.  Calls on one stream are ordered by the
 * stream; concurrent calls on one table from different streams are undefined.
 * Nothing blocks, spins or takes a lock, every probe is bounded by the
 * capacity, no host state is kept, and both calls can be captured into a
 * graph.
 */
#ifndef PDHT_HIP_TABLE_KEYS_H_
#define PDHT_HIP_TABLE_KEYS_H_

#include "pdht_hip.h" /* pdht_hip_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

/* put_keys: stores values[i] under keys[i] for i in 0 .. m-1.  The table,
 * status and counts4[0..2] after the call equal those after
 * pdht_bucket_put_records_dev(keys, values, nranks = 1, key_slot) ->
 * pdht_table_put_records_dev (at one rank the bucketing is stable, so record
 * position = key index): mbits = CityHash64(key); among equal mbits the
 * highest index leaves its row; a new mbits that finds no free slot is
 * dropped under the put's rules (which new mbits lose is left to the
 * schedule, all keys of one mbits share the fate, a present mbits is never
 * dropped).  Counters, the put's: counts4[0] += entries created, [1] += keys
 * dropped, [3] += slots inspected, and [2] += 1: the call uses the per-slot
 * winner words and takes a batch number, so it counts among the 2^32 batches
 * (put, update, cswap, inserting accumulate, add, keyed put, and the keyed
 * update, add and cswap of pdht_hip_table_keys_rmw.h) a table takes
 * between two pdht_table_init_dev calls.
 * status (may be NULL), one uint8 per key: 0 stored / 1 superseded by a later
 * key of the batch with the same mbits / 2 dropped, table full.
 * mbits_out (may be NULL; 8-byte aligned): mbits_out[i] = CityHash64(key i),
 * for a later pdht_table_get_dev, pdht_table_cswap_dev or forged record.
 * workspace: pdht_table_put_keys_workspace_bytes(m) = 4*m bytes (device,
 * 4-byte aligned): the slots between the two kernels.  Its contents on entry
 * do not matter.
 * Two kernels with only the kernel boundary between them.
 * pdht_hip_last_kernel(), P = 16 when rowbytes is a multiple of 16, else 8:
 *   "k_table_claim_keys+k_table_write_keys<P>"
 * -- also for m == 0, which launches nothing and returns 0. */
size_t pdht_table_put_keys_workspace_bytes(size_t m);
int pdht_table_put_keys_dev(void *table, uint64_t capacity, size_t rowbytes,
                            const void *keys, size_t keysize, size_t key_slot,
                            const void *values, size_t elemsize, size_t value_stride,
                            size_t m, void *workspace, size_t workspace_bytes,
                            uint64_t *mbits_out, uint8_t *status,
                            pdht_hip_stream_t stream);

/* get_keys: status and values equal what pdht_bucket_records_dev(nranks = 1)
 * -> pdht_table_get_dev(head 8) -> pdht_get_resolve_dev(value_offset = slot)
 * leaves.  status (required), one uint8 per key:
 *   0  found: row i of values receives the elemsize bytes at row + slot
 *   2  no entry under CityHash64(key i)
 *   3  collision: the keysize bytes at the start of the row differ from key i
 * Rows of values whose status is not 0 keep their bytes.  Repeated keys are
 * allowed.  mbits_out (may be NULL; 8-byte aligned) as above.  The table is
 * not written: counts4 stays.
 * One kernel.  pdht_hip_last_kernel(), P = the widest of 16 / 8 / 4 / 1 that
 * divides rowbytes, slot, values, value_stride and elemsize:
 *   "k_table_get_keys<P>"
 * -- also for m == 0, which launches nothing and returns 0. */
int pdht_table_get_keys_dev(const void *table, uint64_t capacity, size_t rowbytes,
                            const void *keys, size_t keysize, size_t key_slot,
                            size_t m, void *values, size_t elemsize, size_t value_stride,
                            uint64_t *mbits_out, uint8_t *status,
                            pdht_hip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDHT_HIP_TABLE_KEYS_H_ */
