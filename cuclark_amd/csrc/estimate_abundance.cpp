// estimate_abundance.cpp — exe/estimate_abundance: CLARK's third step, the abundance profile of one or more result CSVs, on the CPU.
//   estimate_abundance -F <result.csv> [<result.csv> ...] [-D <database directory>] [-c <conf>] [-g <gamma>] [-a <min %>] [--highconfidence]
// Plain and --extended result CSVs are read alike (their last seven columns are the same: Length, Gamma, 1st_assignment, score1,
// 2nd_assignment, score2, confidence); several files are summed.  A read counts for its 1st_assignment when it passes the filter of
// mic_abund.h: the confidence is decided exactly from score1 and score2, the gamma from the printed Gamma text, compared as a
// decimal.  The table (abundance_table.hpp) goes to stdout; names and lineages come from <-D>/../taxonomy, the layout set_targets.sh
// makes, as for exe/cuCLARK --abundance.
//   estimate_abundance -F <extended.csv> ... --rank-report <file> [--lineage <tsv> | -D <database directory>]
// also writes the rank roll-up report (rank_report.hpp; the rule: mic_rollup.h) into <file>: every read's per-target counts - an
// --extended result CSV carries them, a plain one is refused - are summed along the lineage and the read is counted at the lowest
// level whose confidence passes -c (gamma as above).  The lineage comes from --lineage, else from <-D>/../taxonomy.
//   estimate_abundance -F <result.csv> ... --kraken-report <file> [--lineage <tsv> | -D <database directory>] [--kraken-target-rank <name>]
// also writes Kraken's sample report (kraken_report.hpp) of the same counts into <file>: the cross-check of exe/cuCLARK
// --kraken-report.  Plain result CSVs will do.  With --lineage the targets are the file's labels; with neither the report is flat.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "abundance_table.hpp"
#include "mic_abund.h"
#include "mic_rollup.h"
#include "kraken_report.hpp"
#include "rank_report.hpp"
#include "result_csv.hpp"

namespace {

[[noreturn]] void usage_exit(const char* msg) {
  if (msg && *msg) std::cerr << msg << std::endl;
  std::cerr << "Usage: estimate_abundance -F <result.csv> [<result.csv> ...] [-D <database directory>] [-c <min confidence in [0,1]>]"
               " [-g <min gamma in [0,1]>] [-a <min abundance in [0,100]>] [--highconfidence]"
               " [--rank-report <file> [--lineage <tsv>]] [--kraken-report <file> [--lineage <tsv>] [--kraken-target-rank <name>]]" << std::endl;
  exit(1);
}

}  // namespace

int main(int argc, char** argv) {
  std::vector<std::string> files;
  std::string db, rank_report, lineage_file, kraken_report, kraken_rank = "species";
  mic_abund_filter f = {5, 10, 0, 1};
  uint64_t a_num = 0, a_den = 1;
  for (int i = 1; i < argc; ++i) {
    const std::string v = argv[i];
    auto value = [&](const char* what) -> const char* {
      if (++i >= argc) usage_exit((std::string("Please specify ") + what + ".").c_str());
      return argv[i];
    };
    if (v == "-F") {
      while (i + 1 < argc && argv[i + 1][0] != '-') files.push_back(argv[++i]);
      if (files.empty()) usage_exit("Please specify the result file(s).");
    } else if (v == "-D") {
      db = value("the database directory");
    } else if (v == "-c") {
      const char* t = value("the minimum confidence");
      if (!mic_abund_parse_text(t, 1, &f.conf_num, &f.conf_den)) usage_exit((std::string("The minimum confidence should be a decimal number in [0,1] (at most 9 decimals): ") + t).c_str());
    } else if (v == "-g") {
      const char* t = value("the minimum gamma");
      if (!mic_abund_parse_text(t, 1, &f.gamma_num, &f.gamma_den)) usage_exit((std::string("The minimum gamma should be a decimal number in [0,1] (at most 9 decimals): ") + t).c_str());
    } else if (v == "-a") {
      const char* t = value("the minimum abundance");
      if (!mic_abund_parse_text(t, 100, &a_num, &a_den)) usage_exit((std::string("The minimum abundance should be a decimal number in [0,100] (at most 9 decimals): ") + t).c_str());
    } else if (v == "--rank-report") {
      rank_report = value("the file of the rank report");
    } else if (v == "--kraken-report") {
      kraken_report = value("the file of the Kraken report");
    } else if (v == "--kraken-target-rank") {
      kraken_rank = value("the rank of the targets");
    } else if (v == "--lineage") {
      lineage_file = value("the lineage file");
    } else if (v == "--highconfidence") {
      f.conf_num = 75; f.conf_den = 100; f.gamma_num = 3; f.gamma_den = 100;
    } else if (v == "--help" || v == "-h") {
      usage_exit("");
    } else {
      usage_exit(("Failed to recognize option: " + v).c_str());
    }
  }
  if (files.empty()) usage_exit("Please specify the result file(s) with -F.");
  if (rank_report.empty() && kraken_report.empty() && !lineage_file.empty()) usage_exit("--lineage goes with --rank-report <file>.");
  if (!rank_report.empty() && lineage_file.empty() && db.empty()) usage_exit("--rank-report needs a lineage: --lineage <tsv>, or -D <database directory> with ../taxonomy next to it.");
  if (!db.empty() && db.back() != '/') db.push_back('/');
  // --rank-report: the lineage over the labels of the first file's header, the counters, the per-read scratch
  const bool ranks = !rank_report.empty();
  const std::string tail = ",Length,Gamma,1st_assignment,score1,2nd_assignment,score2,confidence";
  std::vector<std::string> ru_labels;
  mic::rank::Lineage lin;
  std::vector<uint64_t> ru_counts, ru_tot;
  std::vector<uint32_t> ru_off, ru_tg, ru_cn, ru_touched;

  std::map<std::string, uint64_t> per_label;
  uint64_t unassigned = 0, filtered = 0;
  for (const std::string& path : files) {
    std::ifstream in(path);
    if (!in) { std::cerr << "Failed to open the result file: " << path << std::endl; return 1; }
    std::string line;
    size_t ln = 0;
    while (std::getline(in, line)) {
      ++ln;
      if (!line.empty() && line.back() == '\r') line.pop_back();
      if (line.empty()) continue;
      if (ln == 1 && line.compare(0, 10, "Object_ID,") == 0) {                // header
        if (ranks) {
          std::vector<std::string> labs;
          if (line.size() > 9 + tail.size() && line.compare(line.size() - tail.size(), tail.size(), tail) == 0) {
            const std::string mid = line.substr(10, line.size() - tail.size() - 10);
            for (size_t a = 0;;) { const size_t b = mid.find(',', a); labs.push_back(mid.substr(a, b == std::string::npos ? b : b - a)); if (b == std::string::npos) break; a = b + 1; }
          }
          if (labs.empty()) { std::cerr << "--rank-report needs the per-target counts of an --extended result file; " << path << " is not one." << std::endl; return 1; }
          if (ru_labels.empty()) {
            ru_labels = labs;
            std::string err;
            bool ok;
            if (!lineage_file.empty()) ok = mic::rank::lineage_from_file(lineage_file, ru_labels, lin, err);
            else {
              mic::abund::Taxonomy t;
              if (!mic::rank::load_taxonomy(db + "../taxonomy", t)) { std::cerr << "--rank-report: no taxonomy (nodes.dmp) in " << db << "../taxonomy and no --lineage <tsv>." << std::endl; return 1; }
              ok = mic::rank::lineage_from_taxonomy(ru_labels, t, lin, err);
            }
            if (!ok) { std::cerr << err << std::endl; return 1; }
            ru_counts.assign(lin.n_counters(), 0);
            ru_off.assign(8, 0);
            for (uint32_t l = 1; l <= lin.n_levels; ++l) ru_off[l] = ru_off[l - 1] + (uint32_t)lin.groups[l - 1].size();
            ru_tot.assign(ru_labels.size(), 0); ru_touched.assign(ru_labels.size(), 0);
          } else if (labs != ru_labels) { std::cerr << "--rank-report: " << path << " has other targets than " << files[0] << "." << std::endl; return 1; }
        }
        continue;
      }
      if (ranks && ru_labels.empty()) { std::cerr << "--rank-report needs the header line of an --extended result file; " << path << " has none." << std::endl; return 1; }
      // the last seven fields (the object name may hold commas)
      std::string fld[7];
      size_t end = 0;
      bool ok = mic::csv::last_seven(line, fld, &end);
      uint64_t s1 = 0, s2 = 0;
      if (!ok || !mic::csv::parse_u32(fld[3], s1) || !mic::csv::parse_u32(fld[5], s2)) {
        std::cerr << "Failed to read line " << ln << " of " << path << ": not a result line of CLARK's format." << std::endl;
        return 1;
      }
      const std::string& first = fld[2];
      const bool gamma = mic::decimal::at_least(fld[1], f.gamma_num, f.gamma_den);
      if (ranks) {      // the T count columns in front of the last seven
        ru_tg.clear(); ru_cn.clear();
        for (size_t t = ru_labels.size(); t-- > 0 && ok;) {
          const size_t c = end == 0 ? std::string::npos : line.rfind(',', end - 1);
          uint64_t v = 0;
          if (c == std::string::npos || !mic::csv::parse_u32(line.substr(c + 1, end - c - 1), v)) { ok = false; break; }
          if (v) { ru_tg.push_back((uint32_t)t); ru_cn.push_back((uint32_t)v); }
          end = c;
        }
        if (!ok) { std::cerr << "Failed to read line " << ln << " of " << path << ": not a line of an --extended result file with " << ru_labels.size() << " targets." << std::endl; return 1; }
        std::reverse(ru_tg.begin(), ru_tg.end()); std::reverse(ru_cn.begin(), ru_cn.end());
        uint32_t row[MIC_ROLLUP_WORDS];
        ++ru_counts[mic_rollup_read_host(ru_tg.data(), ru_cn.data(), ru_tg.size(), (uint32_t)ru_labels.size(), lin.n_levels, lin.group_of.data(), ru_off.data(),
                                         0, 0, f, gamma ? 1 : 0, 0, ru_tot.data(), ru_touched.data(), row, nullptr)];
      }
      if (first == "NA") { ++unassigned; continue; }
      const bool conf = s1 * f.conf_den >= f.conf_num * (s1 + s2);
      if (conf && gamma) ++per_label[first];
      else ++filtered;
    }
  }
  std::vector<std::string> labels;
  std::vector<uint64_t> counts = {unassigned, filtered};
  for (const auto& kv : per_label) { labels.push_back(kv.first); counts.push_back(kv.second); }
  mic::abund::Taxonomy tax;
  if (!db.empty()) mic::abund::load_taxonomy(db + "../taxonomy", tax);
  if (ranks) {
    if (ru_labels.empty()) { std::cerr << "--rank-report: no result line was read." << std::endl; return 1; }
    const std::string report = mic::rank::format_report(ru_counts, lin);
    FILE* out = fopen(rank_report.c_str(), "wb");
    if (!out || fwrite(report.data(), 1, report.size(), out) != report.size() || fclose(out) != 0) { std::cerr << "Failed to write the rank report: " << rank_report << std::endl; return 1; }
  }
  if (!kraken_report.empty()) {
    // the targets: the lineage file's labels when there is one (it names every target), else the labels that were counted
    std::vector<std::string> kr_labels = labels;
    std::string err;
    if (!lineage_file.empty() && !mic::kraken::lineage_labels(lineage_file, kr_labels, err)) { std::cerr << err << std::endl; return 1; }
    std::vector<uint64_t> kr_counts(kr_labels.size() + 2, 0);
    kr_counts[0] = unassigned; kr_counts[1] = filtered;
    for (const auto& kv : per_label) {
      const auto at = std::find(kr_labels.begin(), kr_labels.end(), kv.first);
      if (at == kr_labels.end()) { std::cerr << "--kraken-report: " << kv.first << " is not a label of " << lineage_file << "." << std::endl; return 1; }
      kr_counts[2 + (size_t)(at - kr_labels.begin())] += kv.second;
    }
    mic::rank::Lineage kl;
    if (!mic::kraken::report_lineage(lineage_file, db.empty() ? std::string() : db + "../taxonomy", kr_labels, kl, err)) { std::cerr << err << std::endl; return 1; }
    const std::string report = mic::kraken::format_report(kr_counts, kl, kraken_rank);
    FILE* out = fopen(kraken_report.c_str(), "wb");
    if (!out || fwrite(report.data(), 1, report.size(), out) != report.size() || fclose(out) != 0) { std::cerr << "Failed to write the Kraken report: " << kraken_report << std::endl; return 1; }
  }
  const std::string table = mic::abund::format_table(counts, labels, &tax, a_num, a_den);
  if (fwrite(table.data(), 1, table.size(), stdout) != table.size() || fflush(stdout) != 0) { std::cerr << "Failed to write the table." << std::endl; return 1; }
  return 0;
}
