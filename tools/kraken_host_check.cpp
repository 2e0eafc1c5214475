// kraken_host_check.cpp — mic_kraken_format (csrc/mic_host.cpp, the rule: csrc/mic_kraken.h) and the Kraken report's formatter
// (csrc/kraken_report.hpp) driven as a stand-alone program, so that they can be built with -fsanitize=address,undefined and run on
// the CPU (tests/test_kraken_out.py does), the way tools/hitmap_host_check.cpp is:
//   g++ -std=c++17 -fopenmp -fsanitize=address,undefined -static-libasan -static-libubsan -Iinclude -Icuclark_amd/csrc -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
//       tools/kraken_host_check.cpp cuclark_amd/csrc/mic_host.cpp -lpthread
//   kraken_host_check <cases.bin> <out.bin>
// cases.bin: u32 n_targets, per target {u32 len, the name}; u32 n_cases, per case {u32 k, u64 filter[4], u32 n_reads, per read {u32 name_len,
// the name, u32 result[8], u32 norm, u32 n_words, u32 words[n_words]}}; u32 n_reports, per report {u32 len, the targets' rank, u32 len, the
// lineage file's path (empty: flat), u64 counts[n_targets + 2]}.  Every array is copied into an allocation of exactly its size.
// out.bin: per case and then per report {u64 text bytes, the text}.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "kraken_report.hpp"
#include "mi_clark.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool put(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
static bool get_str(FILE* f, std::string& s) {
  uint32_t len;
  if (!get(f, &len, 4)) return false;
  s.resize(len);
  return get(f, len ? &s[0] : nullptr, len);
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <cases.bin> <out.bin>\n", argv[0]); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
  uint32_t nt = 0, n_cases = 0, n_reports = 0;
  if (!get(in, &nt, 4)) { fprintf(stderr, "short header\n"); return 2; }
  std::vector<std::string> tnames(nt);
  for (uint32_t t = 0; t < nt; ++t) if (!get_str(in, tnames[t])) return 2;
  std::vector<const char*> tn(nt);
  for (uint32_t t = 0; t < nt; ++t) tn[t] = tnames[t].c_str();
  if (!get(in, &n_cases, 4)) return 2;
  for (uint32_t c = 0; c < n_cases; ++c) {
    uint32_t k, n_reads;
    uint64_t fl[4];
    if (!get(in, &k, 4) || !get(in, fl, 32) || !get(in, &n_reads, 4)) return 2;
    const mic_abund_filter f = {fl[0], fl[1], fl[2], fl[3]};
    std::vector<std::string> names(n_reads);
    std::vector<uint32_t> res((size_t)n_reads * 8), norm(n_reads), offsets(n_reads + 1, 0), words;
    for (uint32_t r = 0; r < n_reads; ++r) {
      uint32_t nw;
      if (!get_str(in, names[r]) || !get(in, &res[(size_t)r * 8], 32) || !get(in, &norm[r], 4) || !get(in, &nw, 4)) return 2;
      std::vector<uint32_t> w(nw);
      if (!get(in, w.data(), (size_t)nw * 4)) return 2;
      words.insert(words.end(), w.begin(), w.end());
      offsets[r + 1] = (uint32_t)words.size();
    }
    std::vector<uint32_t> exact(words);      // (an allocation of exactly the words' size)
    exact.shrink_to_fit();
    std::vector<const char*> rn(n_reads);
    for (uint32_t r = 0; r < n_reads; ++r) rn[r] = names[r].c_str();
    const uint32_t* wp = exact.empty() ? nullptr : exact.data();
    const long len = mic_kraken_format(rn.data(), n_reads, res.data(), norm.data(), (int)k, nt, &f, offsets.data(), wp, tn.data(), nullptr, 0);
    if (len < 0) { fprintf(stderr, "case %u: mic_kraken_format returned %ld\n", c, len); return 1; }
    std::vector<char> text((size_t)len + 1);
    if (mic_kraken_format(rn.data(), n_reads, res.data(), norm.data(), (int)k, nt, &f, offsets.data(), wp, tn.data(), text.data(), text.size()) != len) {
      fprintf(stderr, "case %u: two text lengths\n", c);
      return 1;
    }
    if (len > 0) {    // a buffer that is too small is left alone
      std::vector<char> small((size_t)len, 0x5A);
      if (mic_kraken_format(rn.data(), n_reads, res.data(), norm.data(), (int)k, nt, &f, offsets.data(), wp, tn.data(), small.data(), small.size()) != len || small[0] != 0x5A) {
        fprintf(stderr, "case %u: a short text buffer was written\n", c);
        return 1;
      }
    }
    const uint64_t tb = (uint64_t)len;
    if (!put(out, &tb, 8) || !put(out, text.data(), (size_t)len)) { fprintf(stderr, "cannot write\n"); return 2; }
  }
  if (!get(in, &n_reports, 4)) return 2;
  for (uint32_t c = 0; c < n_reports; ++c) {
    std::string rank, path, err;
    std::vector<uint64_t> counts((size_t)nt + 2);
    if (!get_str(in, rank) || !get_str(in, path) || !get(in, counts.data(), counts.size() * 8)) return 2;
    mic::rank::Lineage lin;
    if (!mic::kraken::report_lineage(path, "", tnames, lin, err)) { fprintf(stderr, "report %u: %s\n", c, err.c_str()); return 1; }
    const std::string text = mic::kraken::format_report(counts, lin, rank);
    const uint64_t tb = text.size();
    if (!put(out, &tb, 8) || !put(out, text.data(), text.size())) { fprintf(stderr, "cannot write\n"); return 2; }
  }
  // what the rule refuses must be refused without a read past the arrays
  {
    const mic_abund_filter ok = {5, 10, 0, 1}, bad = {5, 7, 0, 1};
    const uint32_t desc[2] = {3, 1}, up[2] = {0, 1}, res[8] = {0, 0, 0, 0, 0, 0, 0, 0}, w[1] = {1};
    const char* nm[1] = {"r"};
    if (mic_kraken_format(nm, 1, res, nullptr, 31, nt, &ok, desc, w, tn.data(), nullptr, 0) != MIC_E_INVALID) { fprintf(stderr, "descending offsets were accepted\n"); return 1; }
    if (mic_kraken_format(nullptr, 1, res, nullptr, 31, nt, &ok, up, w, tn.data(), nullptr, 0) != MIC_E_INVALID) { fprintf(stderr, "null names were accepted\n"); return 1; }
    if (mic_kraken_format(nm, 1, nullptr, nullptr, 31, nt, &ok, up, w, tn.data(), nullptr, 0) != MIC_E_INVALID) { fprintf(stderr, "null results were accepted\n"); return 1; }
    if (mic_kraken_format(nm, 1, res, nullptr, 31, nt, nullptr, up, w, tn.data(), nullptr, 0) != MIC_E_INVALID) { fprintf(stderr, "a null filter was accepted\n"); return 1; }
    if (mic_kraken_format(nm, 1, res, nullptr, 31, nt, &bad, up, w, tn.data(), nullptr, 0) != MIC_E_INVALID) { fprintf(stderr, "a filter over 7 was accepted\n"); return 1; }
    if (mic_kraken_format(nm, 1, res, nullptr, 31, nt, &ok, up, nullptr, tn.data(), nullptr, 0) != MIC_E_INVALID) { fprintf(stderr, "null words were accepted\n"); return 1; }
    if (mic_kraken_format(nullptr, 0, nullptr, nullptr, 31, nt, &ok, nullptr, nullptr, tn.data(), nullptr, 0) != 0) { fprintf(stderr, "no reads have text\n"); return 1; }
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("%u cases, %u reports\n", n_cases, n_reports);
  return 0;
}
