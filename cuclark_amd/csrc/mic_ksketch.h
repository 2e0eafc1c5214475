// mic_ksketch.h — the k-mer sketch rule, one definition for host and device (mic_kernels.hip's ksketch_kernel, mic_ksketch_add_host,
// exe/cuCLARK --kmer-report).  How many DIFFERENT k-mers of a target did the reads touch: a target with thousands of reads over a
// few dozen distinct k-mers is a low-complexity or contamination artefact, one with a tenth of the reads over tens of thousands of
// distinct k-mers is present (KrakenUniq's false-positive control).  Per target t:
//   hits[t]       u64: k-mer occurrences of the reads whose table label is t (what the query kernels sum into a result row)
//   regs[t][M]    u8, M = 2^14: a HyperLogLog sketch (p = 14) of the canonical k-mers among them
// For every such occurrence, c = the canonical k-mer (the smaller of the k-mer and its reverse complement, as 2-bit values):
//   h    = fmix64(c ^ 0x9E3779B97F4A7C15)      MurmurHash3's 64-bit finalizer
//   idx  = h >> 50                             the top 14 bits
//   w    = h << 14                             the other 50, left-aligned
//   rank = w ? clz64(w) + 1 : 51               1 .. 51
//   regs[t][idx] = max(regs[t][idx], rank);  hits[t] += 1
// Which occurrences count is the query's rule: per read part, none from a part shorter than k, none across an 'N' (masked bases
// included: they are packed as 'N'), a palindromic k-mer (even k) once per occurrence.  The rule does not look at confidence or gamma.
// Registers merge by element-wise max, hits by sum: batches, engines and calls combine in any order with the same result.
// The estimator (host only) is Ertl's improved raw estimator (O. Ertl, "New cardinality estimation algorithms for HyperLogLog
// sketches", 2017, algorithm 6): no bias tables, no switch between ranges.
#ifndef MIC_KSKETCH_H
#define MIC_KSKETCH_H

#include <stdint.h>

#include "mi_clark.h"

#if defined(__HIPCC__)
#define MIC_KS_HD __host__ __device__
#else
#define MIC_KS_HD
#endif

#define MIC_KSKETCH_P 14
#define MIC_KSKETCH_Q (64 - MIC_KSKETCH_P)              /* hash bits behind the index; ranks are 1 .. Q + 1 */
#define MIC_KSKETCH_SEED 0x9E3779B97F4A7C15ull
#if MIC_KSKETCH_REGS != (1 << MIC_KSKETCH_P)
#error "include/mi_clark.h: MIC_KSKETCH_REGS is 2^14"
#endif

MIC_KS_HD static inline uint64_t mic_ksketch_fmix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// c = the canonical k-mer
MIC_KS_HD static inline uint64_t mic_ksketch_hash(uint64_t c) { return mic_ksketch_fmix64(c ^ MIC_KSKETCH_SEED); }
MIC_KS_HD static inline uint32_t mic_ksketch_index(uint64_t h) { return (uint32_t)(h >> MIC_KSKETCH_Q); }
MIC_KS_HD static inline uint32_t mic_ksketch_rank(uint64_t h) {
  const uint64_t w = h << MIC_KSKETCH_P;
  return w ? (uint32_t)__builtin_clzll(w) + 1u : (uint32_t)MIC_KSKETCH_Q + 1u;
}

// the canonical form of a k-mer value (2 bits per nucleotide, T G C A = 0 1 2 3 as the packer writes them, first nucleotide in the high bits), 1 <= k <= 32:
// the same value as canonical() of mic_device.h, written without device builtins for the host
MIC_KS_HD static inline uint64_t mic_ksketch_canonical(uint64_t kmer, int k) {
  uint64_t x = ~kmer;                                                     // complement, then reverse the 32 pairs
  x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
  x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
  x = ((x >> 8) & 0x00FF00FF00FF00FFull) | ((x & 0x00FF00FF00FF00FFull) << 8);
  x = ((x >> 16) & 0x0000FFFF0000FFFFull) | ((x & 0x0000FFFF0000FFFFull) << 16);
  x = (x >> 32) | (x << 32);
  const uint64_t rc = x >> (64 - 2 * k);
  return kmer < rc ? kmer : rc;
}

#endif
