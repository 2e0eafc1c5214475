// mic_abund.h — the abundance counting rule, one definition for host and device (mic_abund.hip's kernel, mic_abundance_host,
// exe/cuCLARK --abundance, exe/estimate_abundance).  CLARK's estimate_abundance step turns a result CSV into a profile: reads per
// target, with a confidence and a gamma filter.  Here a read's result row {sum, idxBest, best, idxSecond, second, ...} goes into
// one bucket of num_targets + 2:
//   0              unassigned (idxBest == 0: the CSV prints "NA")
//   1              assigned, but the filter drops it
//   idxBest + 1    counts for target idxBest - 1
// The filter is exact integer arithmetic on thresholds num / 10^d (mic_abund_parse: at most 9 fractional digits):
//   confidence best / (best + second) >= c   <=>  best * 10^d >= num * (best + second)
//   gamma      sum / (norm - k + 1)   >= g   <=>  num == 0, or norm - k + 1 > 0 and sum * 10^d >= num * (norm - k + 1)
// (norm = the CSV's Length column, the gamma denominator of mic_fmt_gamma.)  ">=": CLARK's defaults -c 0.5 -g 0 count every
// assigned read.  All products stay below 2^63 for u32 counts and d <= 9.
#ifndef MIC_ABUND_H
#define MIC_ABUND_H

#include <stdint.h>

#include "mi_clark.h"

#if defined(__HIPCC__)
#define MIC_AB_HD __host__ __device__
#else
#define MIC_AB_HD
#endif

#define MIC_ABUND_MAX_DIGITS 9

// a filter the rule can evaluate without overflow: denominators 10^0 .. 10^9, numerators at most the denominator
MIC_AB_HD static inline bool mic_abund_filter_ok(const mic_abund_filter& f) {
  uint64_t p = 1;
  bool cd = false, gd = false;
  for (int i = 0; i <= MIC_ABUND_MAX_DIGITS; ++i, p *= 10) { cd = cd || f.conf_den == p; gd = gd || f.gamma_den == p; }
  return cd && gd && f.conf_num <= f.conf_den && f.gamma_num <= f.gamma_den;
}

MIC_AB_HD static inline uint32_t mic_abund_bucket(const uint32_t* res, uint32_t norm, int k, uint32_t n_targets, const mic_abund_filter& f) {
  const uint32_t sum = res[0], ib = res[1], best = res[2], second = res[4];
  if (ib == 0 || ib > n_targets) return 0;       // (an index past the targets prints "NA" as well: mic_csv_line)
  const bool conf = (uint64_t)best * f.conf_den >= f.conf_num * ((uint64_t)best + second);
  const int64_t den = (int64_t)norm - k + 1;
  const bool gamma = f.gamma_num == 0 || (den > 0 && (uint64_t)sum * f.gamma_den >= f.gamma_num * (uint64_t)den);
  return conf && gamma ? ib + 1 : 1u;
}

// A threshold as the command lines take it: decimal digits with at most one '.', at least one digit, at most 9 after the point,
// value in [0, max_int].  No sign, no exponent, no blanks.  *num / *den = the exact value, *den = 10^(digits after the point).
static inline bool mic_abund_parse_text(const char* s, uint64_t max_int, uint64_t* num, uint64_t* den) {
  if (!s) return false;
  uint64_t n = 0, d = 1;
  int digits = 0, frac = -1;
  for (const char* p = s; *p; ++p) {
    if (*p == '.') { if (frac >= 0) return false; frac = 0; continue; }
    if (*p < '0' || *p > '9') return false;
    if (frac >= 0) { if (++frac > MIC_ABUND_MAX_DIGITS) return false; d *= 10; }
    if (n > (uint64_t)1 << 40) return false;        // far above any bound: stop before the value could wrap
    n = n * 10 + (uint64_t)(*p - '0');
    ++digits;
  }
  if (digits == 0 || n > max_int * d) return false;
  *num = n; *den = d;
  return true;
}

#endif
