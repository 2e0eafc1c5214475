// evaluate_density.cpp — exe/evaluate_density: CLARK's evaluate_density_confidence / evaluate_density_gamma steps, the score densities
// of one or more result CSVs, on the CPU.
//   evaluate_density -F <result.csv> [<result.csv> ...] [--confidence | --gamma]
// Plain and --extended result CSVs are read alike (result_csv.hpp: their last seven columns are the same); several files are summed.
// The report (density_report.hpp; the rule: mic_density.h) goes to stdout - with --confidence or --gamma only the totals and that
// marginal.  It is the report exe/cuCLARK --density counts on the device, and needs no -k:
//   unassigned  1st_assignment "NA" with score1 0: what the CSV prints for idxBest == 0, the device's test (a target whose label is
//               literally "NA" is told apart by its score: an assigned read has score1 > 0);
//   confidence  binned exactly from score1 and score2 (mic_density_conf_bin);
//   gamma       binned from the printed Gamma text read as a decimal: floor(100 text) clamped into 0 .. 100; "-0", "-nan", "inf" and
//               anything else that is no number go to bin 0 (the rule's bin for norm - k + 1 <= 0, the only rows that print them).
// Why text and exact binning agree: "%g" prints sum / den rounded to six significant digits.  Bin edges j / 100 print exactly, so
// rounding never moves a value below its bin's lower edge, and it reaches the upper edge (j + 1) / 100 only when
// 0 < (j + 1) den - 100 sum <= 5e-5 den (half a unit of the sixth digit, for values in [0.1, 1); smaller values have finer digits,
// values of 1 and more are in bin 100 either way).  The left side is a positive integer, so this needs den >= 20 000: reads of fewer
// than 20 000 k-mers are binned identically by this tool and by the device.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "density_report.hpp"
#include "mic_density.h"
#include "result_csv.hpp"

namespace {

[[noreturn]] void usage_exit(const char* msg) {
  if (msg && *msg) std::cerr << msg << std::endl;
  std::cerr << "Usage: evaluate_density -F <result.csv> [<result.csv> ...] [--confidence | --gamma]" << std::endl;
  exit(1);
}

}  // namespace

int main(int argc, char** argv) {
  std::vector<std::string> files;
  mic::density::Which which = mic::density::kAll;
  for (int i = 1; i < argc; ++i) {
    const std::string v = argv[i];
    if (v == "-F") {
      while (i + 1 < argc && argv[i + 1][0] != '-') files.push_back(argv[++i]);
      if (files.empty()) usage_exit("Please specify the result file(s).");
    } else if (v == "--confidence" || v == "--gamma") {
      const mic::density::Which w = v == "--gamma" ? mic::density::kGamma : mic::density::kConfidence;
      if (which != mic::density::kAll && which != w) usage_exit("--confidence and --gamma exclude each other: without either, both densities are written.");
      which = w;
    } else if (v == "--help" || v == "-h") {
      usage_exit("");
    } else {
      usage_exit(("Failed to recognize option: " + v).c_str());
    }
  }
  if (files.empty()) usage_exit("Please specify the result file(s) with -F.");
  std::vector<uint64_t> counts(MIC_DENSITY_WORDS, 0);
  for (const std::string& path : files) {
    std::ifstream in(path);
    if (!in) { std::cerr << "Failed to open the result file: " << path << std::endl; return 1; }
    std::string line;
    size_t ln = 0;
    while (std::getline(in, line)) {
      ++ln;
      if (!line.empty() && line.back() == '\r') line.pop_back();
      if (line.empty()) continue;
      if (ln == 1 && line.compare(0, 10, "Object_ID,") == 0) continue;       // header
      std::string fld[7];
      size_t end = 0;
      uint64_t s1 = 0, s2 = 0;
      if (!mic::csv::last_seven(line, fld, &end) || !mic::csv::parse_u32(fld[3], s1) || !mic::csv::parse_u32(fld[5], s2)) {
        std::cerr << "Failed to read line " << ln << " of " << path << ": not a result line of CLARK's format." << std::endl;
        return 1;
      }
      ++counts[0];
      if (fld[2] == "NA" && s1 == 0) { ++counts[1]; continue; }     // (a target labelled "NA" has a score: see the header comment)
      const uint32_t c = mic_density_conf_bin((uint32_t)s1, (uint32_t)s2);
      const uint32_t g = mic::decimal::floor_hundredths(fld[1], MIC_DENSITY_GAMMA_BINS - 1);
      ++counts[2 + (c - MIC_DENSITY_CONF_LO) * MIC_DENSITY_GAMMA_BINS + g];
    }
  }
  const std::string report = mic::density::format_report(counts.data(), which);
  if (fwrite(report.data(), 1, report.size(), stdout) != report.size() || fflush(stdout) != 0) { std::cerr << "Failed to write the report." << std::endl; return 1; }
  return 0;
}
