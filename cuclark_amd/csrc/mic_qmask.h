// mic_qmask.h — the base-quality mask, one definition for host and device (mic_ingest.hip's pack_kernel<true>, mic_text.hip's
// pair_merge_kernel<true>, mic_fastq_mask_quality, the command line's host merge of paired files).
// A four-line FASTQ record has a sequence line S and a quality line U, both the bytes of the line without its '\n' (a '\r'
// belongs to the line).  With the threshold byte c0 = offset + Q (mic_ingest_set_min_quality; 0 = off):
//   S[i] is MASKED  <=>  i >= len(U)  or  U[i] < c0        (unsigned bytes; surplus quality characters are ignored)
// and a masked byte is to the packer what the byte 'N' is: it ends the ACGTU run it stands in and belongs to no k-mer.  Nothing
// else moves: the Length column counts the bytes of S, names and the gamma denominator are unchanged.
#ifndef MIC_QMASK_H
#define MIC_QMASK_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MIC_QM_HD __host__ __device__
#else
#define MIC_QM_HD
#endif

// is byte i of a sequence line masked by the quality line [qual, qual + qlen)?  (c0 != 0)
MIC_QM_HD static inline bool mic_qmask_masked(const uint8_t* qual, uint32_t qlen, uint32_t i, uint32_t c0) {
  return i >= qlen || (uint32_t)qual[i] < c0;
}

// one sequence line in place (host): seq[0, n) against qual[0, m)
static inline void mic_qmask_line(uint8_t* seq, size_t n, const uint8_t* qual, size_t m, uint32_t c0) {
  const size_t both = n < m ? n : m;
  for (size_t i = 0; i < both; ++i) if ((uint32_t)qual[i] < c0) seq[i] = 'N';
  for (size_t i = both; i < n; ++i) seq[i] = 'N';
}

#endif
