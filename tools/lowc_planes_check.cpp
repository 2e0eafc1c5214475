// The lane logic of lowc_kernel (mic_ingest.hip) on the CPU, against the host form of the rule: for random runs with planted
// tracts, run ends and line ends, every base's window is cut out of three 128-bit masks (run end, low and high code bit) exactly as
// a lane does it, counted with mic_lowc_T_planes, and compared with mic_lowc_run's sliding histogram.  No device.
//   g++ -O2 -std=c++17 -I cuclark_amd/csrc tools/lowc_planes_check.cpp -o check && ./check      (exit 0, prints the totals)
#include "mic_lowc.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

// what one lane computes for logical position q of a sequence whose logical codes are c[0 .. n) (4 = ends the run)
static bool lane_masked(const std::vector<uint8_t>& c, size_t q, uint32_t level) {
  uint32_t we = 0, w0 = 0, w1 = 0;               // bit i: position q - 16 + i; outside the sequence: a run end
  for (int i = 0; i < 32; ++i) {
    const long p = (long)q - MIC_LOWC_HALF + i;
    const uint32_t v = (p < 0 || p >= (long)c.size()) ? 4u : c[(size_t)p];
    we |= (uint32_t)(v > 3u) << i; w0 |= (v & 1u) << i; w1 |= ((v >> 1) & 1u) << i;
  }
  if ((we >> 16) & 1u) return false;
  const uint32_t below = we & 0xFFFFu, above = we >> 17;
  const uint32_t lo = below ? 32u - (uint32_t)__builtin_clz(below) : 0u;
  const uint32_t hi = above ? 16u + (uint32_t)__builtin_ffs((int)above) : 32u;
  if (hi - lo < 4u) return false;
  const uint32_t l = hi - lo - 2u;
  return mic_lowc_over(mic_lowc_T_planes(w0, w1, lo, l), l, level);
}

int main() {
  srand(5);
  long bad = 0, masked = 0, total = 0;
  const uint32_t levels[5] = {1, 20, 21, 58, 149};
  for (int t = 0; t < 4000; ++t) {
    const int L = (t % 7 == 0) ? rand() % 3000 : rand() % 300;
    std::string s;
    for (int i = 0; i < L; ++i) s.push_back("ACGTacgu"[rand() % 8]);
    for (int r = 0; r < 1 + rand() % 4 && L > 0; ++r) {
      const int n = 5 + rand() % 70, p = rand() % L, ul = 1 + rand() % 6;
      std::string u;
      for (int i = 0; i < ul; ++i) u.push_back("ACGT"[rand() % 4]);
      for (int i = 0; i < n && p + i < L; ++i) s[p + i] = u[i % ul];
    }
    for (int r = 0; r < rand() % 4 && L > 0; ++r) s[rand() % L] = "N\rx-"[rand() % 4];
    const uint32_t level = levels[rand() % 5];
    std::vector<uint8_t> c(s.size());
    for (size_t i = 0; i < s.size(); ++i) c[i] = (uint8_t)mic_lowc_code((uint8_t)s[i]);
    std::vector<uint8_t> want(s.size() + 1, 0);
    for (size_t a = 0; a < c.size();) {
      if (c[a] > 3) { ++a; continue; }
      size_t b = a;
      while (b < c.size() && c[b] <= 3) ++b;
      mic_lowc_run(c.data() + a, b - a, level, want.data() + a);
      a = b;
    }
    for (size_t q = 0; q < c.size(); ++q) {
      ++total; masked += want[q];
      if ((bool)want[q] != lane_masked(c, q, level) && bad++ < 5) printf("mismatch: trial %d position %zu level %u\n", t, q, level);
    }
  }
  printf("bases %ld masked %ld mismatches %ld\n", total, masked, bad);
  return bad != 0 || masked == 0;
}
