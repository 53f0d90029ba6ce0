/*
 * pdht_hip_table_iter.h -- enumerating the device-resident target table of
 * pdht_hip_table.h: its entries exported in slot order, as arrays or as put
 * records.  Part of the C-ABI of pdht_hip.h (which includes this header; ABI
 * revision 4, these entry points only add to it) and exported by the same
 * libraries.
 *
 * The reference's owner walks its local table entry by entry in storage order
 * (pdht_iterate / pdht_hasnext / pdht_getnext, libpdht/iter.c:24-91; the
 * Meraculous traversal starts from that walk, bench/Meraculous/
 * meraculous.c:105-108; pdht_print_active, libpdht/util.c:276, dumps the table
 * the same way).  Here the walk is one batch call: a stable stream compaction
 * of the live slots.  Exported as put records it also feeds
 * pdht_table_put_records_dev directly, so a table grows by
 *   rehash = pdht_table_export_dev (record form) -> pdht_table_put_records_dev
 * into a table of another capacity, with no second insertion kernel.
 *
 * Slots.  A table of `capacity` has the slots 0 .. capacity; slot `capacity`
 * is the private slot of mbits 0.  A slot is live when it holds an entry.  A
 * call looks at the slots [first_slot, first_slot + nslots), nslots >= 1 and
 * first_slot + nslots <= capacity + 1.
 *
 * Order.  Entry e is the e-th live slot of the range in ascending slot order.
 * So a table is paged by resuming at (slot of the last entry) + 1, and two
 * exports of an unchanged table -- or two replays of a captured graph -- agree
 * byte for byte.
 *
 * Outputs, for the entries e < max_entries:
 *   the uint64 at (char*)mbits_out + e*mbits_stride   the entry's mbits (0 for
 *                                  the private slot, not the mark that says it
 *                                  is present)
 *   the rowbytes bytes at (char*)rows_out + e*row_stride   its row
 *   the uint32 at (char*)slot_out + e*slot_stride     its slot index
 * Nothing else is written: no byte between rows, nothing at or beyond entry
 * max_entries.  rows_out and slot_out may each be NULL (that output is then
 * not produced and its stride not looked at).
 *   count2[0] = the live slots of the range
 *   count2[1] = min(count2[0], max_entries), the entries written
 * count2 is device memory, 8-byte aligned, never NULL; both words are written
 * by a kernel on every call.  max_entries = 0 is the count-only form: the
 * three outputs may be NULL and no row is touched.
 *
 * Alignment: mbits_out 8-byte aligned, mbits_stride a multiple of 8 and >= 8;
 * rows_out 8-byte aligned, row_stride a multiple of 8 and >= rowbytes;
 * slot_out 4-byte aligned, slot_stride a multiple of 4 and >= 4 (the index
 * rules of the row movers, pdht_hip_put.h).  The outputs must not overlap the
 * table or each other (undefined, not checked).
 *
 * The record form.  With R a record buffer of stride S >= 24 + rowbytes (R
 * 8-byte aligned, S a multiple of 8): mbits_out = R + 16, rows_out = R + 24,
 * slot_out = R + 12 and all three strides = S make the output a put-record
 * batch of count2[1] records.  Bytes +0 .. +11 of each record are left alone;
 * pdht_table_put_records_dev reads none of them (it reads the mbits at +16 and
 * the row at +24 only), nor the slot index at +12.
 *
 * Workspace: pdht_table_export_workspace_bytes(nslots) bytes of device memory,
 * 16-byte aligned; a function of nslots only (0 = refused: nslots 0 or beyond
 * 2^31 + 1).  Its contents on entry are never read.
 *
 * Every refusal happens before any device call, with a message in
 * pdht_hip_last_error(), the geometry checks of pdht_hip_table.h first.  The
 * call does not block, does not spin, keeps no host state and can be captured
 * into a graph.  The table is read with ordinary loads; the stream orders the
 * call behind earlier puts on it.
 *
 * Three launches, the kernel boundaries their only synchronisation
 * (pdht_hip_last_kernel() names them with the piece width of the row copy):
 *   "k_table_export_count+k_table_export_scan+k_table_export_write<16>"
 *       rowbytes, rows_out and row_stride all multiples of 16
 *   "k_table_export_count+k_table_export_scan+k_table_export_write<8>"
 *       any other rows_out.  The record form with S = 24 + rowbytes always
 *       lands here (rowbytes and S are never both multiples of 16), as does
 *       any record buffer that is 16-byte aligned (R + 24 is 8 mod 16)
 *   "k_table_export_count+k_table_export_scan+k_table_export_write<0>"
 *       max_entries > 0 and rows_out NULL: mbits and slot indices only
 *   "k_table_export_count+k_table_export_scan<0>"
 *       the count-only form (two launches)
 */
#ifndef PDHT_HIP_TABLE_ITER_H_
#define PDHT_HIP_TABLE_ITER_H_

#include "pdht_hip.h" /* pdht_hip_stream_t, the status codes */

#ifdef __cplusplus
extern "C" {
#endif

size_t pdht_table_export_workspace_bytes(uint64_t nslots);
int pdht_table_export_dev(const void *table, uint64_t capacity, size_t rowbytes,
                          uint64_t first_slot, uint64_t nslots,
                          void *mbits_out, size_t mbits_stride,
                          void *rows_out, size_t row_stride,
                          void *slot_out, size_t slot_stride,
                          uint64_t max_entries, uint64_t *count2,
                          void *workspace, size_t workspace_bytes,
                          pdht_hip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDHT_HIP_TABLE_ITER_H_ */
