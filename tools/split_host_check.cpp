// split_host_check.cpp — mic_split_host (csrc/mic_host.cpp, the rule: csrc/mic_split.h) driven as a stand-alone program, so that it
// can be built with -fsanitize=address,undefined and run on the CPU (tests/test_split_reads.py does):
//   g++ -std=c++17 -fopenmp -fsanitize=address,undefined -static-libasan -static-libubsan -Iinclude -Icuclark_amd/csrc -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
//       tools/split_host_check.cpp cuclark_amd/csrc/mic_host.cpp -lpthread      (mic_host.cpp calls nothing of the HIP runtime)
//   split_host_check <cases.bin> <out.bin>
// cases.bin: per case {u64 nb, u64 n, i32 k, u32 n_targets, u64 filter[4]}, the text, u64 starts[n], u32 rows[8 n], u32 norms[n].
// Every array is copied into an allocation of exactly its size (a read or write past it is the sanitizer's to find), the output
// buffer is nb + 1 bytes of 0xA5.  out.bin: per case and which = 1, 2, 3: u64 totals[4], then the nb + 1 bytes of the buffer.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mi_clark.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <cases.bin> <out.bin>\n", argv[0]); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
  size_t cases = 0;
  for (;;) {
    uint64_t nb, n, filt[4]; int32_t k; uint32_t nt;
    if (fread(&nb, 8, 1, in) != 1) break;
    if (!get(in, &n, 8) || !get(in, &k, 4) || !get(in, &nt, 4) || !get(in, filt, 32)) { fprintf(stderr, "short case header\n"); return 2; }
    std::vector<uint8_t> text(nb);
    std::vector<uint64_t> starts(n);
    std::vector<uint32_t> rows(n * MIC_RESULT_WORDS), norms(n);
    if (!get(in, text.data(), nb) || !get(in, starts.data(), n * 8) || !get(in, rows.data(), n * MIC_RESULT_WORDS * 4) || !get(in, norms.data(), n * 4)) {
      fprintf(stderr, "short case\n");
      return 2;
    }
    const mic_abund_filter f = {filt[0], filt[1], filt[2], filt[3]};
    for (int which = 1; which <= 3; ++which) {
      std::vector<uint8_t> buf(nb + 1, 0xA5);
      uint64_t tot[4] = {0, 0, 0, 0};
      const int rc = mic_split_host(text.data(), nb, starts.data(), n, rows.data(), norms.data(), k, nt, &f, which, buf.data(), tot);
      if (rc != MIC_OK) { fprintf(stderr, "case %zu, which %d: mic_split_host returned %d\n", cases, which, rc); return 1; }
      if (fwrite(tot, 8, 4, out) != 4 || fwrite(buf.data(), 1, buf.size(), out) != buf.size()) { fprintf(stderr, "cannot write\n"); return 2; }
    }
    ++cases;
  }
  // what the rule refuses must be refused without a read past the arrays
  {
    const uint8_t t[4] = {'>', 'a', '\n', 'A'};
    const uint64_t bad[2] = {0, 9};
    const uint32_t rows[2 * MIC_RESULT_WORDS] = {0};
    uint8_t buf[5];
    uint64_t tot[4];
    const mic_abund_filter f = {5, 10, 0, 1};
    if (mic_split_host(t, 4, bad, 2, rows, nullptr, 31, 6, &f, 3, buf, tot) != MIC_E_INVALID) { fprintf(stderr, "a start past the text was accepted\n"); return 1; }
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("%zu cases\n", cases);
  return 0;
}
