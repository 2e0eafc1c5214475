// kmer_report.hpp — the k-mer report of exe/cuCLARK --kmer-report and mic_ksketch_format, and the estimator behind it (host only, no
// device; the sketches and their rule: csrc/mic_ksketch.h).  Plain CSV text:
//   Name,Reads,Kmers,DistinctKmers,Duplication
//   one line per target with Kmers > 0, in label order:
//     Reads          the reads --abundance gives the target under the run's --min-confidence / --min-gamma
//     Kmers          k-mer occurrences of the reads whose table label is the target (the hit counter)
//     DistinctKmers  llround of the estimate from the target's registers, at least 1
//     Duplication    Kmers / DistinctKmers, two decimals, rounded half up from integer arithmetic
// A target with many reads and a high duplication was hit in the same few k-mers over and over.
// format_coverage (below): the same lines with the target's k-mers in the table and the fraction of them the reads touched.
#ifndef MIC_KMER_REPORT_HPP
#define MIC_KMER_REPORT_HPP

#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "decimal_text.hpp"
#include "mic_ksketch.h"

namespace mic {
namespace ksketch {

// O. Ertl, "New cardinality estimation algorithms for HyperLogLog sketches" (2017), algorithm 6 with the helper series of
// algorithms 4 and 5: the improved raw estimator.  c[v] = how many of the m registers hold v, v = 0 .. q + 1.
inline double sigma(double x) {
  if (x == 1.0) return INFINITY;
  double y = 1.0, z = x, zp;
  do { x *= x; zp = z; z += x * y; y += y; } while (zp != z);
  return z;
}
inline double tau(double x) {
  if (x == 0.0 || x == 1.0) return 0.0;
  double y = 1.0, z = 1.0 - x, zp;
  do { x = sqrt(x); zp = z; y *= 0.5; z -= (1.0 - x) * (1.0 - x) * y; } while (zp != z);
  return z / 3.0;
}

// regs: the MIC_KSKETCH_REGS registers of one target (a value above q + 1 - no k-mer gives one - counts as q + 1)
inline double estimate(const uint8_t* regs) {
  const int q = MIC_KSKETCH_Q;
  const double m = (double)MIC_KSKETCH_REGS;
  uint32_t c[MIC_KSKETCH_Q + 2] = {};
  for (uint32_t i = 0; i < MIC_KSKETCH_REGS; ++i) ++c[regs[i] > q + 1 ? q + 1 : regs[i]];
  double z = m * tau(1.0 - (double)c[q + 1] / m);
  for (int v = q; v >= 1; --v) z = 0.5 * (z + (double)c[v]);
  z += m * sigma((double)c[0] / m);
  return m * m / (2.0 * M_LN2 * z);             // alpha_inf = 1 / (2 ln 2); all registers zero: z = inf, 0; all at q + 1: z = 0, inf
}

inline uint64_t distinct(const uint8_t* regs, uint64_t hits) {
  const double e = estimate(regs);
  if (!(e < 9.0e18)) return (uint64_t)INT64_MAX;            // (every register saturated: no finite estimate; no run of reads gets there)
  const long long v = llround(e);
  return v < 1 ? (hits ? 1u : 0u) : (uint64_t)v;
}

// names: n_targets strings; reads, hits: n_targets words; regs: n_targets * MIC_KSKETCH_REGS bytes
inline std::string format_report(const char* const* names, const uint64_t* reads, const uint8_t* regs, const uint64_t* hits, uint32_t n_targets) {
  std::string out = "Name,Reads,Kmers,DistinctKmers,Duplication\n";
  auto num = [](uint64_t v) { return std::to_string((unsigned long long)v); };
  for (uint32_t t = 0; t < n_targets; ++t) {
    if (!hits[t]) continue;
    const uint64_t d = distinct(regs + (size_t)t * MIC_KSKETCH_REGS, hits[t]);
    out += std::string(names[t]) + "," + num(reads[t]) + "," + num(hits[t]) + "," + num(d) + "," + decimal::ratio_text(hits[t], d, 2) + "\n";
  }
  return out;
}

// The coverage report of exe/cuCLARK --kmer-coverage and mic_kcoverage_format: the k-mer report's lines and two more columns,
//   Name,Reads,Kmers,DistinctKmers,Duplication,TargetKmers,Coverage
//     TargetKmers    the target's k-mers in the resident table (the census counts, csrc/mic_census.h)
//     Coverage       min(DistinctKmers, TargetKmers) / TargetKmers, six decimals, rounded half up from integer arithmetic (the clamp:
//                    a HyperLogLog estimate may exceed the true total by its error)
// target_kmers: n_targets words.  A target with hits and no k-mers in the table (no healthy table gives one): false, *bad = the target.
inline bool format_coverage(const char* const* names, const uint64_t* reads, const uint8_t* regs, const uint64_t* hits, const uint64_t* target_kmers,
                            uint32_t n_targets, std::string& out, uint32_t* bad = nullptr) {
  out = "Name,Reads,Kmers,DistinctKmers,Duplication,TargetKmers,Coverage\n";
  auto num = [](uint64_t v) { return std::to_string((unsigned long long)v); };
  for (uint32_t t = 0; t < n_targets; ++t) {
    if (!hits[t]) continue;
    if (!target_kmers[t]) { if (bad) *bad = t; return false; }
    const uint64_t d = distinct(regs + (size_t)t * MIC_KSKETCH_REGS, hits[t]);
    out += std::string(names[t]) + "," + num(reads[t]) + "," + num(hits[t]) + "," + num(d) + "," + decimal::ratio_text(hits[t], d, 2) + "," +
           num(target_kmers[t]) + "," + decimal::ratio_text(d < target_kmers[t] ? d : target_kmers[t], target_kmers[t], 6) + "\n";
  }
  return true;
}

}  // namespace ksketch
}  // namespace mic
#endif
