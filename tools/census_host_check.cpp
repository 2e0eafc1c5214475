// census_host_check.cpp — mic_db_census_host and mic_kcoverage_format (csrc/mic_host.cpp; the rule: csrc/mic_census.h, the report:
// csrc/kmer_report.hpp) driven as a stand-alone program, so that they can be built with -fsanitize=address,undefined and run on the
// CPU (tests/test_kmer_coverage.py does):
//   g++ -std=c++17 -fopenmp -fsanitize=address,undefined -static-libasan -static-libubsan -Iinclude -Icuclark_amd/csrc -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
//       tools/census_host_check.cpp cuclark_amd/csrc/mic_host.cpp -lpthread      (mic_host.cpp calls nothing of the HIP runtime)
//   census_host_check <cases.bin> <out.bin>
// cases.bin: per case {u64 htsize, u64 n_elems, i32 k, i32 key_bytes, u32 n_targets, u32 sampling}, u8 sizes[htsize], keys[n_elems]
// of key_bytes each, u16 labels[n_elems].  Every array is copied into an allocation of exactly its size (a read or write past it is the
// sanitizer's to find).  out.bin: per case u64 counts[n_targets], u64 stats[8], u64 length of a coverage report, the report (every
// target with as many hits as it has k-mers and all registers zero: one distinct k-mer each).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "mi_clark.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool put(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <cases.bin> <out.bin>\n", argv[0]); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
  size_t cases = 0;
  for (;;) {
    uint64_t htsize, n_el; int32_t k, kb; uint32_t nt, sampling;
    if (fread(&htsize, 8, 1, in) != 1) break;
    if (!get(in, &n_el, 8) || !get(in, &k, 4) || !get(in, &kb, 4) || !get(in, &nt, 4) || !get(in, &sampling, 4)) { fprintf(stderr, "short case header\n"); return 2; }
    std::vector<uint8_t> sizes(htsize), keys(n_el * (size_t)kb);
    std::vector<uint16_t> labels(n_el);
    if (!get(in, sizes.data(), htsize) || !get(in, keys.data(), keys.size()) || !get(in, labels.data(), n_el * 2)) { fprintf(stderr, "short case\n"); return 2; }
    std::vector<uint64_t> counts(nt, 0);
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int rc = mic_db_census_host(sizes.data(), htsize, n_el ? keys.data() : nullptr, kb, n_el ? labels.data() : nullptr, sampling, k, nt,
                                      nt ? counts.data() : nullptr, stats);
    if (rc != MIC_OK) { fprintf(stderr, "case %zu: mic_db_census_host returned %d\n", cases, rc); return 1; }
    std::vector<std::string> names(nt);
    std::vector<const char*> nm(nt);
    for (uint32_t t = 0; t < nt; ++t) { names[t] = "target_" + std::to_string(t + 1); nm[t] = names[t].c_str(); }
    const std::vector<uint8_t> regs((size_t)nt * MIC_KSKETCH_REGS, 0);
    const long len = mic_kcoverage_format(nm.data(), counts.data(), regs.data(), counts.data(), counts.data(), nt, nullptr, 0);
    if (len < 0) { fprintf(stderr, "case %zu: mic_kcoverage_format returned %ld\n", cases, len); return 1; }
    std::vector<char> text((size_t)len + 1);          // exactly the size the call asked for
    if (mic_kcoverage_format(nm.data(), counts.data(), regs.data(), counts.data(), counts.data(), nt, text.data(), text.size()) != len) { fprintf(stderr, "case %zu: two lengths\n", cases); return 1; }
    std::vector<char> small((size_t)len, 0x5A);       // a buffer one byte short is left alone
    if (mic_kcoverage_format(nm.data(), counts.data(), regs.data(), counts.data(), counts.data(), nt, small.data(), small.size()) != len || small[0] != 0x5A) {
      fprintf(stderr, "case %zu: a short buffer was written\n", cases);
      return 1;
    }
    const uint64_t len64 = (uint64_t)len;
    if (!put(out, counts.data(), (size_t)nt * 8) || !put(out, stats, 64) || !put(out, &len64, 8) || !put(out, text.data(), (size_t)len)) { fprintf(stderr, "cannot write\n"); return 2; }
    ++cases;
  }
  // what the functions refuse must be refused without a read past the arrays
  {
    const uint8_t sz[2] = {1, 0};
    const uint32_t ky[1] = {7};
    const uint16_t lb[1] = {0};
    uint64_t counts[1] = {0}, stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (mic_db_census_host(sz, 2, ky, 4, lb, 1, 33, 1, counts, stats) != MIC_E_INVALID) { fprintf(stderr, "k = 33 was accepted\n"); return 1; }
    if (mic_db_census_host(sz, 2, ky, 3, lb, 1, 31, 1, counts, stats) != MIC_E_INVALID) { fprintf(stderr, "3-byte keys were accepted\n"); return 1; }
    if (mic_db_census_host(sz, 2, nullptr, 4, lb, 1, 31, 1, counts, stats) != MIC_E_INVALID) { fprintf(stderr, "null keys were accepted\n"); return 1; }
    if (mic_db_census_host(sz, 2, ky, 4, lb, 1, 31, 1, counts, nullptr) != MIC_E_INVALID) { fprintf(stderr, "null stats were accepted\n"); return 1; }
    // hits on a target without k-mers in the table: no report
    const char* nm[1] = {"t"};
    const std::vector<uint8_t> regs(MIC_KSKETCH_REGS, 0);
    const uint64_t hits[1] = {3}, none[1] = {0};
    if (mic_kcoverage_format(nm, hits, regs.data(), hits, none, 1, nullptr, 0) != MIC_E_INVALID) { fprintf(stderr, "hits without k-mers in the table were reported\n"); return 1; }
    if (mic_kcoverage_format(nm, hits, regs.data(), hits, nullptr, 1, nullptr, 0) != MIC_E_INVALID) { fprintf(stderr, "null target k-mers were accepted\n"); return 1; }
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("%zu cases\n", cases);
  return 0;
}
