// mic_density.h — the score-density rule, one definition for host and device (mic_density.hip's kernel, mic_density_host,
// exe/cuCLARK --density, exe/evaluate_density).  CLARK's evaluate_density_confidence / evaluate_density_gamma steps show how many
// assignments a run has per confidence score and per gamma score: how a user picks --min-confidence and --min-gamma.  Here a read's
// result row {sum, idxBest, best, idxSecond, second, ...} goes into one cell of a 51 x 101 table, bins of width 0.01:
//   unassigned     idxBest == 0 or idxBest > n_targets (mic_abund.h's test: the CSV prints "NA"); no cell
//   confidence bin c = floor(100 best / (best + second)) clamped into 50 .. 100; best + second == 0: c = 100
//                  (bin 100 is exactly 1.0, bin 50 holds the ties; the clamp keeps a malformed row of caller-owned memory in the table)
//   gamma bin      den = norm - k + 1 (signed; norm = the CSV's Length column): den <= 0: g = 0, else g = min(100, floor(100 sum / den))
// Integer arithmetic only, 64-bit products (u32 counts: every product stays below 2^39).
// Counters, MIC_DENSITY_WORDS u64: [0] reads seen, [1] unassigned, [2 + (c - 50) * 101 + g] the joint cell.  The two marginal
// densities are sums over the table and are not stored.
// Bin edges are multiples of 0.01 and the filters of mic_abund.h are ">=": for thresholds conf, gamma of at most two decimals the
// reads mic_abund_bucket keeps are exactly the cells with c >= 100 conf and g >= 100 gamma - the report's cumulative columns
// (density_report.hpp) are survival counts of the filters, not estimates.
#ifndef MIC_DENSITY_H
#define MIC_DENSITY_H

#include <stdint.h>

#include "mi_clark.h"

#if defined(__HIPCC__)
#define MIC_DN_HD __host__ __device__
#else
#define MIC_DN_HD
#endif

#define MIC_DENSITY_CONF_LO 50
#define MIC_DENSITY_CONF_BINS 51
#define MIC_DENSITY_GAMMA_BINS 101
#define MIC_DENSITY_CELLS (MIC_DENSITY_CONF_BINS * MIC_DENSITY_GAMMA_BINS)
#define MIC_DENSITY_NONE 0xFFFFFFFFu       /* mic_density_cell: the read is unassigned */
#if MIC_DENSITY_WORDS != 2 + MIC_DENSITY_CELLS
#error "include/mi_clark.h: MIC_DENSITY_WORDS is 2 + 51 * 101"
#endif

MIC_DN_HD static inline uint32_t mic_density_conf_bin(uint32_t best, uint32_t second) {
  const uint64_t tot = (uint64_t)best + second;
  if (tot == 0) return 100u;
  const uint64_t c = (uint64_t)best * 100u / tot;
  return c < MIC_DENSITY_CONF_LO ? (uint32_t)MIC_DENSITY_CONF_LO : c > 100u ? 100u : (uint32_t)c;
}

MIC_DN_HD static inline uint32_t mic_density_gamma_bin(uint32_t sum, uint32_t norm, int k) {
  const int64_t den = (int64_t)norm - k + 1;
  if (den <= 0) return 0u;
  const uint64_t g = (uint64_t)sum * 100u / (uint64_t)den;
  return g > 100u ? 100u : (uint32_t)g;
}

// the read's cell, 0 .. MIC_DENSITY_CELLS - 1 (its counter is word 2 + cell), or MIC_DENSITY_NONE
MIC_DN_HD static inline uint32_t mic_density_cell(const uint32_t* res, uint32_t norm, int k, uint32_t n_targets) {
  const uint32_t sum = res[0], ib = res[1], best = res[2], second = res[4];
  if (ib == 0 || ib > n_targets) return MIC_DENSITY_NONE;
  return (mic_density_conf_bin(best, second) - MIC_DENSITY_CONF_LO) * MIC_DENSITY_GAMMA_BINS + mic_density_gamma_bin(sum, norm, k);
}

#endif
