// hitmap_host_check.cpp — mic_hitmap_runs_host and mic_hitmap_format (csrc/mic_host.cpp, the rule: csrc/mic_hitmap.h) driven as a
// stand-alone program, so that they can be built with -fsanitize=address,undefined and run on the CPU (tests/test_hit_maps.py does):
//   g++ -std=c++17 -fopenmp -fsanitize=address,undefined -static-libasan -static-libubsan -Iinclude -Icuclark_amd/csrc -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
//       tools/hitmap_host_check.cpp cuclark_amd/csrc/mic_host.cpp -lpthread      (mic_host.cpp calls nothing of the HIP runtime)
//   hitmap_host_check <cases.bin> <out.bin>
// cases.bin: u32 n_targets, then per target {u32 len, the name}; then per case {u32 n_reads}, per read {u32 name_len, the name, u32 n_parts,
// u32 part_nk[n_parts], u32 labels[sum of part_nk]}.  Every array is copied into an allocation of exactly its size (a read or write past
// it is the sanitizer's to find).  out.bin: per case {u32 n_words, u32 offsets[n_reads + 1], u32 words[n_words], u64 text bytes, the text}.
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
  uint32_t nt = 0;
  if (!get(in, &nt, 4)) { fprintf(stderr, "short header\n"); return 2; }
  std::vector<std::string> tnames(nt);
  for (uint32_t t = 0; t < nt; ++t) {
    uint32_t len;
    if (!get(in, &len, 4)) return 2;
    tnames[t].resize(len);
    if (!get(in, &tnames[t][0], len)) return 2;
  }
  std::vector<const char*> tn(nt);
  for (uint32_t t = 0; t < nt; ++t) tn[t] = tnames[t].c_str();
  size_t cases = 0;
  for (;;) {
    uint32_t n_reads;
    if (fread(&n_reads, 4, 1, in) != 1) break;
    std::vector<std::string> names(n_reads);
    std::vector<uint32_t> offsets(n_reads + 1, 0), words;
    for (uint32_t r = 0; r < n_reads; ++r) {
      uint32_t nl, np;
      if (!get(in, &nl, 4)) return 2;
      names[r].resize(nl);
      if (!get(in, &names[r][0], nl) || !get(in, &np, 4)) return 2;
      std::vector<uint32_t> nk(np);
      if (!get(in, nk.data(), (size_t)np * 4)) return 2;
      size_t total = 0;
      for (uint32_t p = 0; p < np; ++p) total += nk[p];
      std::vector<uint32_t> labels(total);
      if (!get(in, labels.data(), total * 4)) return 2;
      const long n = mic_hitmap_runs_host(labels.data(), nk.data(), np, nt, nullptr, 0);
      if (n < 0) { fprintf(stderr, "case %zu, read %u: mic_hitmap_runs_host returned %ld\n", cases, r, n); return 1; }
      std::vector<uint32_t> w((size_t)n);
      if (mic_hitmap_runs_host(labels.data(), nk.data(), np, nt, w.data(), w.size()) != n) { fprintf(stderr, "case %zu: two lengths\n", cases); return 1; }
      if (n > 0) {    // a buffer one word short: the length is still given, nothing is written behind the buffer
        std::vector<uint32_t> small((size_t)n - 1);
        if (mic_hitmap_runs_host(labels.data(), nk.data(), np, nt, small.data(), small.size()) != n) { fprintf(stderr, "case %zu: short buffer\n", cases); return 1; }
      }
      words.insert(words.end(), w.begin(), w.end());
      offsets[r + 1] = (uint32_t)words.size();
    }
    std::vector<const char*> rn(n_reads);
    for (uint32_t r = 0; r < n_reads; ++r) rn[r] = names[r].c_str();
    const long len = mic_hitmap_format(rn.data(), n_reads, offsets.data(), words.data(), tn.data(), nt, nullptr, 0);
    if (len < 0) { fprintf(stderr, "case %zu: mic_hitmap_format returned %ld\n", cases, len); return 1; }
    std::vector<char> text((size_t)len + 1);
    if (mic_hitmap_format(rn.data(), n_reads, offsets.data(), words.data(), tn.data(), nt, text.data(), text.size()) != len) { fprintf(stderr, "case %zu: two text lengths\n", cases); return 1; }
    if (len > 0) {    // a buffer that is too small is left alone
      std::vector<char> small((size_t)len, 0x5A);
      if (mic_hitmap_format(rn.data(), n_reads, offsets.data(), words.data(), tn.data(), nt, small.data(), small.size()) != len || small[0] != 0x5A) {
        fprintf(stderr, "case %zu: a short text buffer was written\n", cases);
        return 1;
      }
    }
    const uint32_t nw = (uint32_t)words.size();
    const uint64_t tb = (uint64_t)len;
    if (!put(out, &nw, 4) || !put(out, offsets.data(), offsets.size() * 4) || !put(out, words.data(), words.size() * 4) || !put(out, &tb, 8) ||
        !put(out, text.data(), (size_t)len)) { fprintf(stderr, "cannot write\n"); return 2; }
    ++cases;
  }
  // what the rule refuses must be refused without a read past the arrays
  {
    const uint32_t big[1] = {65536};
    const uint32_t lab[1] = {1};
    if (mic_hitmap_runs_host(lab, big, 1, 4, nullptr, 0) != MIC_E_INVALID) { fprintf(stderr, "a part of 65 536 positions was accepted\n"); return 1; }
    if (mic_hitmap_runs_host(lab, nullptr, 1, 4, nullptr, 0) != MIC_E_INVALID) { fprintf(stderr, "null part lengths were accepted\n"); return 1; }
    const uint32_t desc[2] = {3, 1};
    const char* nm[1] = {"r"};
    if (mic_hitmap_format(nm, 1, desc, lab, tn.data(), nt, nullptr, 0) != MIC_E_INVALID) { fprintf(stderr, "descending offsets were accepted\n"); return 1; }
    if (mic_hitmap_format(nullptr, 1, desc, lab, tn.data(), nt, nullptr, 0) != MIC_E_INVALID) { fprintf(stderr, "null names were accepted\n"); return 1; }
    if (mic_hitmap_runs_host(nullptr, nullptr, 0, 4, nullptr, 0) != 0) { fprintf(stderr, "a read without parts has words\n"); return 1; }
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("%zu cases\n", cases);
  return 0;
}
