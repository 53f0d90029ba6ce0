// product/pdht_hooks_table.h -- the A/B hook points of the table export
// (pdht_table_iter.hip), PRODUCT build: none taken.  The tuning build's
// header of the same name holds the alternative the export was measured
// against (EXPERIMENTS.md §R10).
#pragma once

namespace pdht {

// bytes the export's workspace holds for a range of nslots
static inline size_t hook_table_export_workspace(size_t bytes, u64) { return bytes; }
// the three launches of an export (kNoVariant: the product's own)
static inline int hook_table_export(const ExportArgs &, unsigned, bool, bool, hipStream_t) { return kNoVariant; }

}  // namespace pdht
