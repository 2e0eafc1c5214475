// density_report.hpp — the score-density report of exe/cuCLARK --density, exe/evaluate_density and mic_density_format (host only, no
// device; the counters and their rule: csrc/mic_density.h).  Plain CSV text, four blocks:
//   Reads,<n> / Unassigned,<n> / Assigned,<n>
//   Confidence,Reads,Cumulative     51 lines 0.50 .. 1.00: the assigned reads of the bin, and those of this bin and every bin above:
//                                   what --min-confidence <that value> keeps (the 0.50 line's Cumulative = Assigned)
//   Gamma,Reads,Cumulative          101 lines 0.00 .. 1.00, the same for --min-gamma
//   Confidence,Gamma,Reads          the non-zero joint cells in ascending order
// Assigned is the sum of the joint cells (= Reads - Unassigned for counters the rule produced).
#ifndef MIC_DENSITY_REPORT_HPP
#define MIC_DENSITY_REPORT_HPP

#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "mic_density.h"

namespace mic {
namespace density {

enum Which { kAll = 0, kConfidence = 1, kGamma = 2 };

inline std::string bin_text(uint32_t hundredths) {
  char b[16];
  snprintf(b, sizeof(b), "%u.%02u", hundredths / 100u, hundredths % 100u);
  return b;
}

// counts: MIC_DENSITY_WORDS words
inline std::string format_report(const uint64_t* counts, Which which = kAll) {
  const uint64_t* cell = counts + 2;
  std::vector<uint64_t> conf(MIC_DENSITY_CONF_BINS, 0), gamma(MIC_DENSITY_GAMMA_BINS, 0);
  uint64_t assigned = 0;
  for (uint32_t c = 0; c < MIC_DENSITY_CONF_BINS; ++c)
    for (uint32_t g = 0; g < MIC_DENSITY_GAMMA_BINS; ++g) {
      const uint64_t v = cell[c * MIC_DENSITY_GAMMA_BINS + g];
      conf[c] += v; gamma[g] += v; assigned += v;
    }
  std::string out;
  auto num = [](uint64_t v) { return std::to_string((unsigned long long)v); };
  out += "Reads," + num(counts[0]) + "\nUnassigned," + num(counts[1]) + "\nAssigned," + num(assigned) + "\n";
  auto marginal = [&](const char* head, const std::vector<uint64_t>& m, uint32_t lo) {
    out += head;
    uint64_t cum = assigned;
    for (size_t i = 0; i < m.size(); ++i) {
      out += bin_text(lo + (uint32_t)i) + "," + num(m[i]) + "," + num(cum) + "\n";
      cum -= m[i];
    }
  };
  if (which == kAll || which == kConfidence) marginal("Confidence,Reads,Cumulative\n", conf, MIC_DENSITY_CONF_LO);
  if (which == kAll || which == kGamma) marginal("Gamma,Reads,Cumulative\n", gamma, 0);
  if (which == kAll) {
    out += "Confidence,Gamma,Reads\n";
    for (uint32_t c = 0; c < MIC_DENSITY_CONF_BINS; ++c)
      for (uint32_t g = 0; g < MIC_DENSITY_GAMMA_BINS; ++g) {
        const uint64_t v = cell[c * MIC_DENSITY_GAMMA_BINS + g];
        if (v) out += bin_text(MIC_DENSITY_CONF_LO + c) + "," + bin_text(g) + "," + num(v) + "\n";
      }
  }
  return out;
}

}  // namespace density
}  // namespace mic
#endif
