// pdht_table_iter.hip -- the target table's entries in slot order (include/pdht_hip_table_iter.h;
// kernels in table_iter.h): argument checks, launchers and the C ABI.  Every check runs before any
// device call.
#include "table_host.h"
#include "table_iter.h"
// the A/B hook points of the export (product/pdht_hooks_table.h: none taken)
#include "pdht_hooks_table.h"

namespace pdht {

// Store policy of the exported mbits, slot indices and rows (EXPERIMENTS.md §R10: plain stores; the
// record form's 4-, 8- and row-sized pieces of one record merge in L2, non-temporal ones take 1.4-2x)
constexpr bool kTableExportNt = false;

static thread_local char g_export_chain[96];

static u64 export_tiles(u64 nslots) { return (nslots + kExportTile - 1) / kExportTile; }

static size_t export_workspace_bytes(u64 nslots) {
  if (nslots == 0 || nslots > (1ull << 31) + 1) return 0;
  return hook_table_export_workspace((size_t)((export_tiles(nslots) * 4 + 15) & ~15ull), nslots);
}

static int table_export(const void *table, u64 capacity, size_t rowbytes, u64 first_slot, u64 nslots,
                        void *mbits_out, size_t mbits_stride, void *rows_out, size_t row_stride, void *slot_out,
                        size_t slot_stride, u64 max_entries, u64 *count2, void *workspace, size_t workspace_bytes,
                        hipStream_t st) {
  if (int rc = geom_check(table, capacity, rowbytes)) return rc;
  if (nslots == 0) return fail("table export: nslots must be >= 1%s", "");
  if (first_slot > capacity || nslots > capacity + 1 - first_slot)
    return fail("table export: first_slot + nslots must be <= capacity + 1%s", "");
  if (max_entries) {
    if (!mbits_out) return fail("table export: mbits_out must not be NULL when max_entries > 0%s", "");
    if ((uintptr_t)mbits_out & 7) return fail("table export: mbits_out must be 8-byte aligned%s", "");
    if (mbits_stride < 8 || (mbits_stride & 7))
      return fail("table export: mbits_stride must be a multiple of 8 and >= 8%s", "");
    if (rows_out) {
      if ((uintptr_t)rows_out & 7) return fail("table export: rows_out must be 8-byte aligned%s", "");
      if (row_stride < rowbytes || (row_stride & 7))
        return fail("table export: row_stride must be a multiple of 8 and >= rowbytes%s", "");
    }
    if (slot_out) {
      if ((uintptr_t)slot_out & 3) return fail("table export: slot_out must be 4-byte aligned%s", "");
      if (slot_stride < 4 || (slot_stride & 3))
        return fail("table export: slot_stride must be a multiple of 4 and >= 4%s", "");
    }
  }
  if (!count2) return fail("table export: count2 must not be NULL%s", "");
  if ((uintptr_t)count2 & 7) return fail("table export: count2 must be 8-byte aligned%s", "");
  if (!workspace) return fail("table export: workspace must not be NULL%s", "");
  if ((uintptr_t)workspace & 15) return fail("table export: workspace must be 16-byte aligned%s", "");
  const size_t need = export_workspace_bytes(nslots);
  if (workspace_bytes < need)
    return fail("table export: workspace too small (%s%lld bytes needed)", "", (long long)need);
  const bool rows = max_entries && rows_out;
  const bool p16 = rows && (rowbytes & 15) == 0 && (row_stride & 15) == 0 && ((uintptr_t)rows_out & 15) == 0;
  if (max_entries)
    snprintf(g_export_chain, sizeof g_export_chain, "k_table_export_count+k_table_export_scan+k_table_export_write<%d>",
             !rows ? 0 : p16 ? 16 : 8);
  else
    snprintf(g_export_chain, sizeof g_export_chain, "k_table_export_count+k_table_export_scan<0>");
  g_kernel = g_export_chain;
  int dev;
  if (int rc = current_device(&dev)) return rc;
  const TableGeom t = make_geom(table, capacity, rowbytes);
  ExportArgs a{};
  a.tags = t.tags;
  a.rows = t.rows;
  a.rowbytes = rowbytes;
  a.first = first_slot;
  a.nslots = nslots;
  a.ntiles = export_tiles(nslots);
  a.cap = t.cap;
  a.tiles = static_cast<u32 *>(workspace);
  a.count2 = count2;
  a.max_entries = max_entries;
  a.mbits_out = static_cast<uint8_t *>(mbits_out);
  a.mbits_stride = mbits_stride;
  a.rows_out = rows ? static_cast<uint8_t *>(rows_out) : nullptr;
  a.row_stride = row_stride;
  a.slot_out = max_entries ? static_cast<uint8_t *>(slot_out) : nullptr;
  a.slot_stride = slot_stride;
  a.np = (u32)(rowbytes / (p16 ? 16 : 8));
  a.gshift = group_shift(a.np);
  const unsigned grid = grid_for(a.ntiles, 8, dev);
  const bool nt = hook_table_export_nt(kTableExportNt);
  if (int rc = hook_table_export(a, grid, p16, nt, st); rc != kNoVariant) return rc;
  k_table_export_count<<<grid, kBlock, 0, st>>>(a);
  HIP_TRY(hipGetLastError());
  k_table_export_scan<<<1, kExportScanBlock, 0, st>>>(a);
  HIP_TRY(hipGetLastError());
  if (!max_entries) return 0;
  if (p16)
    nt ? k_table_export_write<16, true><<<grid, kBlock, 0, st>>>(a)
       : k_table_export_write<16, false><<<grid, kBlock, 0, st>>>(a);
  else
    nt ? k_table_export_write<8, true><<<grid, kBlock, 0, st>>>(a)
       : k_table_export_write<8, false><<<grid, kBlock, 0, st>>>(a);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace pdht

using namespace pdht;

PDHT_API size_t pdht_table_export_workspace_bytes(uint64_t nslots) { return export_workspace_bytes(nslots); }

PDHT_API int pdht_table_export_dev(const void *table, uint64_t capacity, size_t rowbytes, uint64_t first_slot,
                                   uint64_t nslots, void *mbits_out, size_t mbits_stride, void *rows_out,
                                   size_t row_stride, void *slot_out, size_t slot_stride, uint64_t max_entries,
                                   uint64_t *count2, void *workspace, size_t workspace_bytes, pdht_hip_stream_t s) {
  return table_export(table, capacity, rowbytes, first_slot, nslots, mbits_out, mbits_stride, rows_out, row_stride,
                      slot_out, slot_stride, max_entries, count2, workspace, workspace_bytes, ST(s));
}
