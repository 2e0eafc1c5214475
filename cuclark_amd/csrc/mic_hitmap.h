// mic_hitmap.h — the hit-map rule, one definition for host and device (mic_kernels.hip's hitmap_kernel, mic_ingest.hip's text kernels,
// mic_hitmap_runs_host, mic_hitmap_format, exe/cuCLARK --hit-maps).  WHERE along a read the hits fall: a chimeric read shows as target
// A for 90 k-mers, nothing for k - 1 k-mers, then target B; a conserved-gene false positive as a short island of hits in an empty read.
// Read r is its packed parts exactly as the packer wrote them (reads_pointer, containers): maximal nucleotide runs of at least k
// nucleotides, a run longer than MIC_MAX_PART as the packer's overlapping sub-parts (their k-mer positions do not overlap).
//   part p, plen nucleotides     nk = plen - k + 1 k-mer positions; position i has label L[i] = the 1-based label the table gives the
//                                k-mer at i, or 0: the k-mer is in no target, the label is above n_targets, or this engine does not
//                                answer for the k-mer (probe_any's `mine`)
//   run                          a maximal stretch of equal labels inside ONE part (never across a part boundary, equal labels or not)
//   map of a read                32-bit words: per part, in order, one word (label << 16) | len per run, 1 <= len <= 65535 (nk <=
//                                MIC_MAX_PART, at most 65 535 targets); between two consecutive parts one separator word 0 (a run's
//                                len is never 0: unambiguous); a read without parts has an empty map
//   batch                        offsets u32[n_reads + 1] (exclusive prefix sums of words per read) + words
// Per read: the sum of len over words with label != 0 is the query kernels' total (result word 0), per target the count of the read's
// sparse row, over all words the sum of nk over the parts.  A sub-part cut shows as a separator and a label run that crosses it as two
// runs: the packed form cannot tell a cut from an 'N', and nothing here guesses.
// The text, one line per read in input order behind the header line MIC_HITMAP_HEADER:
//   <name>,<map>\n     <name>: what the result CSV prints in its first column (the same cut, at most 39 bytes);  <map>: tokens joined
//                      by single spaces - a run is <target>:<len> (<target>: the target's name as the CSV's assignment columns print
//                      it, 0 for label 0; <len>: plain decimal), a separator is | ; an empty map gives <name>,\n
#ifndef MIC_HITMAP_H
#define MIC_HITMAP_H

#include <stdint.h>

#include "mi_clark.h"

#if defined(__HIPCC__)
#define MIC_HM_HD __host__ __device__
#else
#define MIC_HM_HD
#endif

#define MIC_HITMAP_SEP 0u
#define MIC_HITMAP_NAME_MAX 39u         /* the CSV's cap on a read's name (OBJECTNAMEMAX - 1) */

// the label a position contributes: m = what the probe gave (0: none), mine = this engine answers for the k-mer
MIC_HM_HD static inline uint32_t mic_hitmap_label(uint32_t m, bool mine, uint32_t n_targets) { return (m && mine && m <= n_targets) ? m : 0u; }
MIC_HM_HD static inline uint32_t mic_hitmap_word(uint32_t label, uint32_t len) { return (label << 16) | len; }
MIC_HM_HD static inline uint32_t mic_hitmap_word_label(uint32_t w) { return w >> 16; }
MIC_HM_HD static inline uint32_t mic_hitmap_word_len(uint32_t w) { return w & 0xFFFFu; }

#endif
