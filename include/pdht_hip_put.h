/*
 * pdht_hip_put.h -- the payload half of destination bucketing: put records
 * that carry their values, and row gather / scatter in bucket order.  Part of
 * the C-ABI of pdht_hip.h (which includes this header; ABI revision 4, these
 * entry points only add to it) and exported by the same libraries.
 *
 * pdht_bucket_records_dev writes message_t + key.  A put sends more
 * (pdht_put, libmpipdht/putget.c:80-101): sizeof(message_t) +
 * PDHT_MAXKEYSIZE + dht->elemsize bytes, the value at msg->key +
 * PDHT_MAXKEYSIZE; the Meraculous loader ships whole list_t entries
 * (bench/Meraculous/buildUFXhashBinary.h:196-237); and get replies
 * {status, key, value} (libmpipdht/pdht.h:131-135) come back grouped by rank
 * and have to return to the caller's order.
 */
#ifndef PDHT_HIP_PUT_H_
#define PDHT_HIP_PUT_H_

#include "pdht_hip.h" /* pdht_hip_stream_t, the status codes */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- row movers (all pointers are device pointers) ----------------------- */
/* Rows of rowbytes bytes, row r of a buffer at byte r*stride; index_p is the
 * uint32 at (char*)index + p*index_stride:
 *   index_stride == 4               a dense index_out of pdht_bucket_batch_dev;
 *   index_stride == record stride,
 *   index = records + 12            the source index stored in wire records.
 * Bytes of dst outside [row*dst_stride, row*dst_stride + rowbytes) are never
 * written; row offsets are 64-bit.  m < 2^32, rowbytes >= 1, both strides >=
 * rowbytes, index_stride a multiple of 4 and >= 4, index 4-byte aligned.
 * index may lie in the buffer dst points into (as the put path's does), the
 * bytes themselves must not overlap; src and dst must not overlap.  Every
 * index must name a row the caller owns: nothing here knows the row count of
 * the indexed buffer.  Any alignment works; rows move in pieces of the
 * widest of 16 / 8 / 4 / 1 bytes that divides rowbytes, both strides and both
 * base addresses (pdht_hip_last_kernel(): "k_rows_gather<16>", ...). */
/* dst row p = src row index_p, for p < m.  Repeated indices are allowed. */
int pdht_gather_rows_dev(const void *src, size_t src_stride, size_t rowbytes,
                         const void *index, size_t index_stride, size_t m,
                         void *dst, size_t dst_stride, pdht_hip_stream_t stream);
/* dst row index_p = src row p.  The indices must be distinct. */
int pdht_scatter_rows_dev(const void *src, size_t src_stride, size_t rowbytes,
                          const void *index, size_t index_stride, size_t m,
                          void *dst, size_t dst_stride, pdht_hip_stream_t stream);

/* ---- put records ---------------------------------------------------------- */
/* pdht_bucket_records_dev with the value behind the key: a put's send buffer.
 * Record at bucketed position p, stride pdht_bucket_put_record_bytes(keysize,
 * key_slot, elemsize) = 24 + slot + elemsize rounded up to 8, where slot =
 * key_slot ? key_slot : keysize rounded up to 8:
 *   +0        the header, source index and mbits exactly as
 *             pdht_bucket_records_dev writes them (type, rank, ht_index,
 *             index, mbits)
 *   +24       key[keysize], zero-padded to slot
 *   +24+slot  value[index][elemsize], zero-padded to 8
 * values: row i at (char*)values + i*value_stride (value_stride >= elemsize).
 * key_slot = 32 (PDHT_MAXKEYSIZE) with elemsize % 8 == 0 is byte for byte the
 * sbuf of putget.c:80-98; key_slot = 0 is the compact form.  key_slot must
 * be 0 or a multiple of 8 that is >= keysize (the size query returns 0
 * otherwise).  Every byte of every record is defined on return.  records
 * (device, 8-byte aligned) holds n records; the workspace is sized by
 * pdht_bucket_records_workspace_bytes and must be 16-byte aligned,
 * bucket_offsets (8-byte aligned) as for pdht_bucket_batch_dev; a misaligned
 * one is refused before any launch.  Two kernels run on the stream, the bucketing kernel
 * and the value mover; pdht_hip_last_kernel() names both, e.g.
 * "k_bucket_scatter_staged<8B>+k_rows_gather<8>". */
size_t pdht_bucket_put_record_bytes(size_t keysize, size_t key_slot, size_t elemsize);
int pdht_bucket_put_records_dev(const void *keys, size_t keysize,
                                const void *values, size_t elemsize, size_t value_stride,
                                size_t n, uint32_t nranks, uint32_t msg_type,
                                uint32_t src_rank, uint32_t ht_index, size_t key_slot,
                                void *workspace, size_t workspace_bytes,
                                void *records, uint64_t *bucket_offsets,
                                pdht_hip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDHT_HIP_PUT_H_ */
