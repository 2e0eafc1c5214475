// ksketch_host_check.cpp — mic_ksketch_add_host, mic_ksketch_estimate and mic_ksketch_format (csrc/mic_host.cpp; the rule:
// csrc/mic_ksketch.h, the estimator and the report: csrc/kmer_report.hpp) driven as a stand-alone program, so that they can be built
// with -fsanitize=address,undefined and run on the CPU (tests/test_kmer_report.py does):
//   g++ -std=c++17 -fopenmp -fsanitize=address,undefined -static-libasan -static-libubsan -Iinclude -Icuclark_amd/csrc -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
//       tools/ksketch_host_check.cpp cuclark_amd/csrc/mic_host.cpp -lpthread      (mic_host.cpp calls nothing of the HIP runtime)
//   ksketch_host_check <cases.bin> <out.bin>
// cases.bin: per case {u64 n, i32 k, u32 n_targets}, u64 kmers[n], u32 labels[n], u64 reads[n_targets].
// Every array is copied into an allocation of exactly its size (a read or write past it is the sanitizer's to find).  out.bin: per
// case u64 hits[n_targets], the n_targets * 16384 register bytes, f64 estimate[n_targets], u64 length of the report, the report.
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
    uint64_t n; int32_t k; uint32_t nt;
    if (fread(&n, 8, 1, in) != 1) break;
    if (!get(in, &k, 4) || !get(in, &nt, 4)) { fprintf(stderr, "short case header\n"); return 2; }
    std::vector<uint64_t> kmers(n), reads(nt);
    std::vector<uint32_t> labels(n);
    if (!get(in, kmers.data(), n * 8) || !get(in, labels.data(), n * 4) || !get(in, reads.data(), (size_t)nt * 8)) { fprintf(stderr, "short case\n"); return 2; }
    std::vector<uint8_t> regs((size_t)nt * MIC_KSKETCH_REGS, 0);
    std::vector<uint64_t> hits(nt, 0);
    // in two halves: a sketch is added to, the halves merge into what one call gives
    const size_t half = n / 2;
    int rc = mic_ksketch_add_host(kmers.data(), labels.data(), half, k, nt, regs.data(), hits.data());
    if (rc == MIC_OK) rc = mic_ksketch_add_host(kmers.data() + half, labels.data() + half, n - half, k, nt, regs.data(), hits.data());
    if (rc != MIC_OK) { fprintf(stderr, "case %zu: mic_ksketch_add_host returned %d\n", cases, rc); return 1; }
    std::vector<double> est(nt);
    for (uint32_t t = 0; t < nt; ++t) est[t] = mic_ksketch_estimate(regs.data() + (size_t)t * MIC_KSKETCH_REGS);
    std::vector<std::string> names(nt);
    std::vector<const char*> nm(nt);
    for (uint32_t t = 0; t < nt; ++t) { names[t] = "target_" + std::to_string(t + 1); nm[t] = names[t].c_str(); }
    const long len = mic_ksketch_format(nm.data(), reads.data(), regs.data(), hits.data(), nt, nullptr, 0);
    if (len < 0) { fprintf(stderr, "case %zu: mic_ksketch_format returned %ld\n", cases, len); return 1; }
    std::vector<char> text((size_t)len + 1);          // exactly the size the call asked for
    if (mic_ksketch_format(nm.data(), reads.data(), regs.data(), hits.data(), nt, text.data(), text.size()) != len) { fprintf(stderr, "case %zu: two lengths\n", cases); return 1; }
    if (len > 0) {                                    // a buffer one byte short is left alone
      std::vector<char> small((size_t)len, 0x5A);
      if (mic_ksketch_format(nm.data(), reads.data(), regs.data(), hits.data(), nt, small.data(), small.size()) != len || small[0] != 0x5A) {
        fprintf(stderr, "case %zu: a short buffer was written\n", cases);
        return 1;
      }
    }
    const uint64_t len64 = (uint64_t)len;
    if (!put(out, hits.data(), (size_t)nt * 8) || !put(out, regs.data(), regs.size()) || !put(out, est.data(), (size_t)nt * 8) || !put(out, &len64, 8) ||
        !put(out, text.data(), (size_t)len)) { fprintf(stderr, "cannot write\n"); return 2; }
    ++cases;
  }
  // what the rule refuses must be refused without a read past the arrays
  {
    const uint64_t km[1] = {1ull << 62};              // no 27-mer
    const uint32_t lb[1] = {1};
    std::vector<uint8_t> regs(MIC_KSKETCH_REGS, 0);
    uint64_t hits[1] = {0};
    if (mic_ksketch_add_host(km, lb, 1, 27, 1, regs.data(), hits) != MIC_E_INVALID) { fprintf(stderr, "a value that is no k-mer was accepted\n"); return 1; }
    if (mic_ksketch_add_host(km, lb, 1, 33, 1, regs.data(), hits) != MIC_E_INVALID) { fprintf(stderr, "k = 33 was accepted\n"); return 1; }
    if (mic_ksketch_add_host(km, lb, 1, 32, 1, nullptr, hits) != MIC_E_INVALID) { fprintf(stderr, "null registers were accepted\n"); return 1; }
    if (mic_ksketch_estimate(nullptr) >= 0) { fprintf(stderr, "null registers were estimated\n"); return 1; }
    if (mic_ksketch_format(nullptr, hits, regs.data(), hits, 1, nullptr, 0) != MIC_E_INVALID) { fprintf(stderr, "null names were accepted\n"); return 1; }
    // a label past the targets and label 0 add nothing
    const uint64_t k2[2] = {5, 6};
    const uint32_t l2[2] = {0, 2};
    if (mic_ksketch_add_host(k2, l2, 2, 31, 1, regs.data(), hits) != MIC_OK || hits[0] != 0) { fprintf(stderr, "a label outside the targets was counted\n"); return 1; }
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("%zu cases\n", cases);
  return 0;
}
