// mic_census.h — the table census rule, one definition for host and device (mic_kernels.hip's census_kernel, mic_db_census_host,
// exe/cuCLARK --kmer-coverage).  How many k-mers of each target does the resident table hold: the denominator of KrakenUniq's
// coverage (distinct k-mers the reads touched / the target's k-mers in the database), and at the same time a check that every k-mer of
// the database comes back from the built table under its own label.
// Input: the images a table is loaded from (.sz / .ky / .lb: bucket sizes, keys, 0-based labels), a bucket range [s0, s1), `sampling`
// and rank_base (the non-empty buckets in front of s0).  The elements are those the table builders enumerate:
//   bucket   kept when non-empty and (sampling <= 1 or its rank among the non-empty buckets, counted from 1, is a multiple of sampling)
//   entry    reachable by the reference's linear scan (CuClarkDB.cu:1291-1307): its key is above every key in front of it and not
//            above the bucket's last key (in a well-formed bucket - keys ascending - that is every entry)
//   c        = key * htsize + bucket
// For each element, with l = the table's answer to a read that is exactly this k-mer (probe_any at position 0) and `mine` = this
// engine answers for it:
//   c > revcomp(c, k)            stats[2] += 1      not canonical (malformed databases only): no query can ask for it
//   !mine                        stats[1] += 1      another part or shard answers for it
//   l == file label + 1          stats[0] += 1;  l <= num_targets: counts[l - 1] += 1;  else stats[4] += 1 (in no counts entry)
//   otherwise                    stats[3] += 1      lost: not found, or found under another label
// counts is u64[num_targets], stats u64[8] with stats[5 .. 7] left 0.  All additions commute: tiles, waves, parts and calls combine in
// any order.  A healthy whole table shows stats[3] == 0, stats[0] == its number of k-mers, sum(counts) == stats[0] - stats[4]; every
// k-mer is `mine` on exactly one part of a parted table, so the parts' counts sum to the whole table's.
// The host form has no table to probe: every canonical element counts under its file label - what a healthy whole table returns.
#ifndef MIC_CENSUS_H
#define MIC_CENSUS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define MIC_CS_HD __host__ __device__
#else
#define MIC_CS_HD
#endif

#define MIC_CENSUS_STATS 8
#define MIC_CENSUS_FOUND 0          /* found under their own label */
#define MIC_CENSUS_ELSEWHERE 1      /* another part or shard answers */
#define MIC_CENSUS_NONCANONICAL 2
#define MIC_CENSUS_LOST 3
#define MIC_CENSUS_BEYOND 4         /* found, label at or above num_targets */
#define MIC_CENSUS_LDS_TARGETS 8192 /* up to here the kernel counts in a per-block histogram (32 KiB of u32) */

// reverse complement of a k-mer value (2 bits per nucleotide, complement = 3 - code, first nucleotide in the high bits), 1 <= k <= 32;
// bits above 2k do not count.  The same value as revcomp_bits() of mic_device.h, written without device builtins.
MIC_CS_HD static inline uint64_t mic_census_revcomp(uint64_t c, int k) {
  uint64_t x = ~c;
  x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
  x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
  x = ((x >> 8) & 0x00FF00FF00FF00FFull) | ((x & 0x00FF00FF00FF00FFull) << 8);
  x = ((x >> 16) & 0x0000FFFF0000FFFFull) | ((x & 0x0000FFFF0000FFFFull) << 16);
  x = (x >> 32) | (x << 32);
  return x >> (64 - 2 * k);
}
MIC_CS_HD static inline bool mic_census_is_canonical(uint64_t c, int k) { return !(c > mic_census_revcomp(c, k)); }

// the reference scan over one bucket: begin with the bucket's last key, then feed the keys in file order; true = this entry is reachable
struct MicCensusScan { uint64_t last, run; bool first; };
MIC_CS_HD static inline MicCensusScan mic_census_scan(uint64_t last_key) { MicCensusScan s; s.last = last_key; s.run = 0; s.first = true; return s; }
MIC_CS_HD static inline bool mic_census_reach(MicCensusScan& s, uint64_t kv) {
  const bool rising = s.first || kv > s.run;
  const bool reach = rising && kv <= s.last;
  if (rising) { s.run = kv; s.first = false; }
  return reach;
}

// the stats field of a canonical element: l = the table's answer (label + 1, 0 = not found), file_label 0-based
MIC_CS_HD static inline int mic_census_field(uint32_t l, bool mine, uint32_t file_label) {
  return !mine ? MIC_CENSUS_ELSEWHERE : l == file_label + 1u ? MIC_CENSUS_FOUND : MIC_CENSUS_LOST;
}

#endif
