// split_reads.cpp — exe/split_reads: the classified and the unclassified reads of a result CSV written out as two files, on the CPU.
//   split_reads -F <result.csv> -O <reads.fa|fq> [--classified-out <file>] [--unclassified-out <file>] [-c <conf>] [-g <gamma>] [--highconfidence]
// The cross-check of exe/cuCLARK --classified-out / --unclassified-out: the CSV and the file's records (mic_index_reads) are walked
// in step - row i belongs to record i, a differing name is an error that names the row.  Plain and --extended result CSVs are read
// alike (result_csv.hpp).  A record is classified by exe/estimate_abundance's comparisons: 1st_assignment is not NA, the confidence
// passes exactly from score1 and score2, the gamma from the printed Gamma text compared as a decimal.  The bytes are cut by
// mic_split.h's host partition: every record from its header line to the next record's, unchanged.  Plain C++: the indexer is
// mic_host.cpp's, compiled into the tool; no device library is loaded.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "mi_clark.h"
#include "mic_abund.h"
#include "mic_split.h"
#include "result_csv.hpp"

namespace {

[[noreturn]] void usage_exit(const char* msg) {
  if (msg && *msg) std::cerr << msg << std::endl;
  std::cerr << "Usage: split_reads -F <result.csv> -O <reads.fa|fq> [--classified-out <file>] [--unclassified-out <file>]"
               " [-c <min confidence in [0,1]>] [-g <min gamma in [0,1]>] [--highconfidence]" << std::endl;
  exit(1);
}

bool write_file(const std::string& path, const uint8_t* p, size_t n) {
  FILE* out = fopen(path.c_str(), "wb");
  if (!out) return false;
  const bool ok = fwrite(p, 1, n, out) == n;
  return fclose(out) == 0 && ok;
}

}  // namespace

int main(int argc, char** argv) {
  std::string csv, reads, out_c, out_u;
  mic_abund_filter f = {5, 10, 0, 1};
  for (int i = 1; i < argc; ++i) {
    const std::string v = argv[i];
    auto value = [&](const char* what) -> const char* {
      if (++i >= argc) usage_exit((std::string("Please specify ") + what + ".").c_str());
      return argv[i];
    };
    if (v == "-F") csv = value("the result file");
    else if (v == "-O") reads = value("the file of the reads");
    else if (v == "--classified-out") out_c = value("the file of the classified reads");
    else if (v == "--unclassified-out") out_u = value("the file of the unclassified reads");
    else if (v == "-c") {
      const char* t = value("the minimum confidence");
      if (!mic_abund_parse_text(t, 1, &f.conf_num, &f.conf_den)) usage_exit((std::string("The minimum confidence should be a decimal number in [0,1] (at most 9 decimals): ") + t).c_str());
    } else if (v == "-g") {
      const char* t = value("the minimum gamma");
      if (!mic_abund_parse_text(t, 1, &f.gamma_num, &f.gamma_den)) usage_exit((std::string("The minimum gamma should be a decimal number in [0,1] (at most 9 decimals): ") + t).c_str());
    } else if (v == "--highconfidence") {
      f.conf_num = 75; f.conf_den = 100; f.gamma_num = 3; f.gamma_den = 100;
    } else if (v == "--help" || v == "-h") {
      usage_exit("");
    } else {
      usage_exit(("Failed to recognize option: " + v).c_str());
    }
  }
  if (csv.empty()) usage_exit("Please specify the result file with -F.");
  if (reads.empty()) usage_exit("Please specify the file of the reads with -O.");
  if (out_c.empty() && out_u.empty()) usage_exit("Please specify --classified-out <file>, --unclassified-out <file> or both.");
  if (out_c == out_u) usage_exit("--classified-out and --unclassified-out name the same file.");

  std::vector<uint8_t> text;
  {
    std::ifstream in(reads, std::ios::binary);
    if (!in) { std::cerr << "Failed to open the file of the reads: " << reads << std::endl; return 1; }
    text.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
  }
  std::vector<uint64_t> name_s, name_e, start;
  long n = 0;
  if (!text.empty()) {
    std::vector<uint64_t> ss(1), se(1), ln(1);
    name_s.resize(1); name_e.resize(1);
    n = mic_index_reads(text.data(), text.size(), 1, name_s.data(), name_e.data(), ss.data(), se.data(), ln.data());
    if (n < 0) { std::cerr << "The file of the reads is neither FASTA nor FASTQ: " << reads << std::endl; return 1; }
    name_s.resize(n); name_e.resize(n); ss.resize(n); se.resize(n); ln.resize(n);
    n = mic_index_reads(text.data(), text.size(), (size_t)n, name_s.data(), name_e.data(), ss.data(), se.data(), ln.data());
    start.resize(n);
    for (long r = 0; r < n; ++r) start[r] = name_s[r] - 1;
  }
  std::vector<char> classified((size_t)n, 0);            // the class of every record, from its row
  std::ifstream in(csv);
  if (!in) { std::cerr << "Failed to open the result file: " << csv << std::endl; return 1; }
  std::string line;
  size_t ln = 0;
  long row = 0;
  while (std::getline(in, line)) {
    ++ln;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) continue;
    if (ln == 1 && line.compare(0, 10, "Object_ID,") == 0) continue;
    std::string fld[7];
    size_t end = 0;
    uint64_t s1 = 0, s2 = 0;
    if (!mic::csv::last_seven(line, fld, &end) || !mic::csv::parse_u32(fld[3], s1) || !mic::csv::parse_u32(fld[5], s2)) {
      std::cerr << "Failed to read line " << ln << " of " << csv << ": not a result line of CLARK's format." << std::endl;
      return 1;
    }
    if (row >= n) { std::cerr << "Row " << row + 1 << " of " << csv << " has no record: " << reads << " holds " << n << "." << std::endl; return 1; }
    size_t nl = (size_t)(name_e[row] - name_s[row]);
    if (nl >= 40) nl = 39;                    // (the CSV prints at most 39 characters of a name: mic_csv_line)
    if (line.size() <= nl || line[nl] != ',' || memcmp(line.data(), text.data() + name_s[row], nl) != 0) {
      std::cerr << "Row " << row + 1 << " of " << csv << " is not record " << row + 1 << " of " << reads << ": the names differ ("
                << line.substr(0, line.find(',')) << " / " << std::string((const char*)text.data() + name_s[row], nl) << ")." << std::endl;
      return 1;
    }
    const bool cls = fld[2] != "NA" && s1 * f.conf_den >= f.conf_num * (s1 + s2) && mic::decimal::at_least(fld[1], f.gamma_num, f.gamma_den);
    classified[(size_t)row] = cls ? 1 : 0;
    ++row;
  }
  if (row != n) { std::cerr << csv << " has " << row << " rows, " << reads << " holds " << n << " records." << std::endl; return 1; }
  std::vector<uint8_t> out(text.size() + 1);
  uint64_t tot[4] = {0, 0, 0, 0};
  const int which = (out_c.empty() ? 0 : MIC_SPLIT_CLASSIFIED) | (out_u.empty() ? 0 : MIC_SPLIT_UNCLASSIFIED);
  if (!mic_split_partition_host(text.data(), text.size(), start.data(), (size_t)n, which, [&](size_t r) { return classified[r] != 0; }, out.data(), tot)) {
    std::cerr << "Failed to split " << reads << ": its records do not tile the file." << std::endl;
    return 1;
  }
  if (!out_c.empty() && !write_file(out_c, out.data(), tot[0])) { std::cerr << "Failed to write the classified reads: " << out_c << std::endl; return 1; }
  if (!out_u.empty() && !write_file(out_u, out.data() + tot[0], tot[1])) { std::cerr << "Failed to write the unclassified reads: " << out_u << std::endl; return 1; }
  std::cerr << tot[2] << " classified, " << tot[3] << " unclassified" << std::endl;
  return 0;
}
