// mic_lowc.h — the low-complexity mask, one definition for host and device (mic_ingest.hip's lowc_kernel and pack_kernel<*, true>,
// mic_text_mask_low_complexity).  Integer arithmetic only.
// A RUN is a maximal sequence of nucleotide bytes (ACGTU, either case) of a record's sequence - what the packer calls a part, before
// its length >= k test: '\n' is transparent (wrapped FASTA lines join), every other byte ends the run ('\r', 'N', a base already masked
// by --min-base-quality: runs are taken AFTER the quality mask).  A run has n nucleotides x[0..n) in the packer's 2-bit code (U = T)
// and triplets t[j] = 16 x[j] + 4 x[j+1] + x[j+2], j in [0, n-2).
//   window of base i:  [lo, hi), lo = max(0, i-16), hi = min(n, i+16)       (width 32, centred, clipped to the run)
//   l = hi - lo - 2 triplets t[lo .. lo+l);  c_v = occurrences of the value v among them;  T = sum_v c_v (c_v - 1) / 2  (<= 435)
//   base i is MASKED  <=>  l >= 2  and  10 T > level (l - 1)                 (level in [1,149]; 0 = off; 150 could mask nothing:
//                                                                             a full window of one letter has 10 T = 4350 = 150 * 29)
// A masked base is to the packer what an 'N' is: it ends the run it stands in and belongs to no k-mer.  Nothing else moves: Length
// column, names and gamma's denominator are unchanged, and record_kernel's container bound holds (still one byte between two parts).
// This is DUST's score (Morgulis et al. 2006: sum c(c-1)/2 over (l-1), threshold level/10) on a FIXED centred window of about k
// nucleotides.  It is NOT symmetric DUST's perfect intervals: the report of dustmasker or another tool differs at tract edges.
// The rule is NOT idempotent: a fragment left between two masked stretches is a new, shorter run with other windows.  It is
// therefore applied exactly once, to the original text (after the quality mask), and no device text that can be classified again
// (a MIC_INGEST_RESIDENT slot) is rewritten by it: the device keeps a bitmap beside the text.
#ifndef MIC_LOWC_H
#define MIC_LOWC_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MIC_LC_HD __host__ __device__
#else
#define MIC_LC_HD
#endif

#define MIC_LOWC_MAX_LEVEL 149u
#define MIC_LOWC_HALF 16          /* window = [i - 16, i + 16) */

// the packer's 2-bit code of a nucleotide byte (A=3 C=2 G=1 T/U=0), or 4 for any other byte
MIC_LC_HD static inline uint32_t mic_lowc_code(uint32_t b) {
  const uint32_t u = b & 0xDFu;
  return (u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'U') ? ((0x4Bu >> (2 * ((u >> 1) & 3u))) & 3u) : 4u;
}

// the mask condition
MIC_LC_HD static inline bool mic_lowc_over(uint32_t T, uint32_t l, uint32_t level) { return l >= 2 && 10u * T > level * (l - 1u); }

// T of one window given as bit planes: bit i of c0 / c1 = low / high code bit of window position i (0..31), the window's triplets are
// those at positions [lo, lo + l), l <= 30 (bits outside [lo, lo + l + 2) are ignored).  Pairs of equal triplets are counted per
// distance d: position j and j + d both inside, all three codes equal.
MIC_LC_HD static inline uint32_t mic_lowc_T_planes(uint32_t c0, uint32_t c1, uint32_t lo, uint32_t l) {
  if (l < 2) return 0;
  const uint32_t m0 = ((1u << l) - 1u) << lo;              // l <= 30, lo + l <= 30
  uint32_t T = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t d = 1; d < 30; ++d) {
    const uint32_t eq = ~((c0 ^ (c0 >> d)) | (c1 ^ (c1 >> d)));           // code j == code j + d
    const uint32_t e3 = eq & (eq >> 1) & (eq >> 2) & m0 & (m0 >> d);      // triplet j == triplet j + d, both in the window
#if defined(__HIP_DEVICE_COMPILE__)
    T += __popc(e3);
#else
    T += (uint32_t)__builtin_popcount(e3);
#endif
  }
  return T;
}

// one run on the host, linear in n: code[0..n) the run's 2-bit codes, out[i] = 1 for every masked base (out holds n bytes).
// The triplet histogram slides: a triplet that leaves takes c - 1 pairs with it, one that enters adds c.
static inline void mic_lowc_run(const uint8_t* code, size_t n, uint32_t level, uint8_t* out) {
  memset(out, 0, n);
  if (n < 4 || level == 0) return;
  uint8_t cnt[64];
  memset(cnt, 0, sizeof cnt);
  size_t a = 0, b = 0;              // triplets [a, b) are in the histogram
  uint32_t T = 0;
  for (size_t i = 0; i < n; ++i) {
    const size_t lo = i > MIC_LOWC_HALF ? i - MIC_LOWC_HALF : 0, hi = i + MIC_LOWC_HALF < n ? i + MIC_LOWC_HALF : n;
    const size_t tb = hi - 2;       // triplets [lo, hi - 2)   (hi >= 4 here)
    for (; b < tb; ++b) T += cnt[16 * code[b] + 4 * code[b + 1] + code[b + 2]]++;
    for (; a < lo; ++a) T -= --cnt[16 * code[a] + 4 * code[a + 1] + code[a + 2]];
    if (mic_lowc_over(T, (uint32_t)(tb - lo), level)) out[i] = 1;
  }
}

#endif
