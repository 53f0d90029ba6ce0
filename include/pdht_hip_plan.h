/*
 * pdht_hip_plan.h -- the launch plan and tile order of the default 64-B
 * kernel, for callers and tests that need to know which shape a batch takes
 * (pdht_hip_last_kernel() names the kernel, not the launch shape).  Part of
 * the C-ABI of pdht_hip.h (which includes this header; ABI revision 4, these
 * entry points only add to it) and exported by the same libraries.
 */
#ifndef PDHT_HIP_PLAN_H_
#define PDHT_HIP_PLAN_H_

#include "pdht_hip.h" /* the status codes */

#ifdef __cplusplus
extern "C" {
#endif

/* Launch plan of the default 64-B kernel (k_fixed_xpose64, 256 threads, two
 * tiles of prefetch per wave) over n packed, 16-B aligned 64-B keys on a chip
 * of `cus` CUs; host arithmetic only, no GPU is touched.  A tile is 64 keys;
 * W = waves = the waves the persistent grid keeps resident (3 workgroups of 4
 * per CU, fewer for a small batch); a round is 2 W consecutive tiles.
 *   round_blocked = 0: the persistent shape -- `grid` workgroups, workgroup b
 *     walks every round in slot b; a big batch goes out as `launches`
 *     consecutive launches of that shape (`grid` and `rounds` are the first
 *     one's);
 *   round_blocked = 1: ONE launch of `grid` workgroups, workgroup b serving
 *     rounds_per_wg rounds from round (b / (W/4)) * rounds_per_wg on, in slot
 *     b % (W/4).
 * In round r the wave w of a workgroup in slot s hashes tiles
 * (2 r + d) W + 4 s + w, d = 0, 1 (those below the batch's tile count).
 * rounds_per_wg < 0 asks for the library's own choice, 0 for the persistent
 * shape; with_hist != 0 plans a call that accumulates a histogram (always
 * persistent; up to 4M keys such a call takes a 1024-thread shape instead,
 * which this plan does not describe). */
typedef struct pdht_hip_xpose64_plan {
  uint64_t grid;          /* workgroups of the (first) launch */
  uint64_t rounds;        /* rounds the (first) launch spans */
  uint64_t launches;      /* consecutive launches the batch goes out as */
  uint32_t waves;         /* W */
  uint32_t rounds_per_wg; /* R; 0 in the persistent shape */
  uint32_t round_blocked;
  uint32_t reserved;
} pdht_hip_xpose64_plan;
int pdht_hip_xpose64_plan_for(size_t n, int cus, int rounds_per_wg, int with_hist,
                              pdht_hip_xpose64_plan *plan);
/* Tile numbers of workgroups [block0, block0 + nblocks) of the plan's (first)
 * launch, from the function the kernel itself indexes with:
 * tiles[((b * RW + r) * 2 + d) * 4 + w] for the workgroup's r-th round, RW =
 * rounds_per_wg (round-blocked) or rounds (persistent).  Entries at or above
 * the batch's tile count are tiles the kernel skips. */
int pdht_hip_xpose64_tiles(const pdht_hip_xpose64_plan *plan, uint64_t block0,
                           size_t nblocks, uint64_t *tiles);
#ifdef __cplusplus
}
#endif

#endif /* PDHT_HIP_PLAN_H_ */
