// mic_kraken.h — the Kraken per-read line, one definition for host and device (mic_ingest.hip's kraken_len_kernel / kraken_fmt_kernel,
// mic_kraken_format, exe/cuCLARK --kraken-out).  The tools behind a k-mer classifier (Pavian, Krona's ktImportTaxonomy, KrakenTools,
// Bracken, MultiQC) read Kraken's per-read file; everything a line needs is what a batch already has: the result row, the CSV's Length
// column, the name cut, the class rule of mic_split.h and the hit-map words of mic_hitmap.h.  One line per read, in input order, no
// header line:
//   <class>\t<name>\t<taxid>\t<length>\t<map>\n
//   <class>   C iff mic_split_classified(result row, norm, k, n_targets, filter) - bucket >= 2 of mic_abund_bucket, the predicate of
//             --classified-out; else U (no hit, an index above the targets, dropped by --min-confidence / --min-gamma)
//   <name>    what the hit-map text prints: the CSV's first column, a name of 40 bytes or more as its first 39
//   <taxid>   on a C line the name of target idxBest - 1 as the CSV's 1st_assignment prints it, on a U line 0.  The target's LABEL
//             (a taxid for a database made with set_targets.sh), not an LCA: resolving at a higher rank stays with --rank-report
//   <length>  norm in plain decimal: the CSV's Length column (merged pairs: the length minus one; ONE number, not Kraken's a|b - the
//             merged text does not keep the mates' own lengths)
//   <map>     the read's hit-map words, tokens joined by single blanks: a run <target>:<len> exactly as the hit-map text prints it
//             (0:<len> for label 0, NA for a label above n_targets), a separator word |:| (the packed form cannot tell an N from
//             the mate joint: every separator prints that way); an empty map prints 0:0, so that the field always has a token
// mic_kraken_line below writes a line byte by byte into any sink; the sink that only counts gives the line's length, so that the
// length pass and the format pass cannot disagree.
#ifndef MIC_KRAKEN_H
#define MIC_KRAKEN_H

#include <stdint.h>

#include "mic_fmt.h"
#include "mic_hitmap.h"
#include "mic_split.h"

// put(char): takes the line's next byte; target(l, put): puts the name of target l - 1 (1 <= l <= n_targets)
template <typename Put, typename Target>
MIC_HM_HD static inline void mic_kraken_line(Put& put, const uint8_t* name, uint32_t name_len, const uint32_t* res, uint32_t norm, int k,
                                             uint32_t n_targets, const mic_abund_filter& f, const uint32_t* words, uint32_t n_words,
                                             Target& target) {
  const bool cls = mic_split_classified(res, norm, k, n_targets, f);
  char tmp[16];
  put(cls ? 'C' : 'U'); put('\t');
  const uint32_t nl = name_len >= 40 ? MIC_HITMAP_NAME_MAX : name_len;
  for (uint32_t i = 0; i < nl; ++i) put((char)name[i]);
  put('\t');
  if (cls) target(res[1], put); else put('0');
  put('\t');
  { const int n = mic_fmt_u32(norm, tmp); for (int i = 0; i < n; ++i) put(tmp[i]); }
  put('\t');
  if (n_words == 0) { put('0'); put(':'); put('0'); }
  for (uint32_t i = 0; i < n_words; ++i) {
    const uint32_t w = words[i], l = mic_hitmap_word_label(w);
    if (i) put(' ');
    if (w == MIC_HITMAP_SEP) { put('|'); put(':'); put('|'); continue; }
    if (l == 0) put('0');
    else if (l > n_targets) { put('N'); put('A'); }
    else target(l, put);
    put(':');
    const int n = mic_fmt_u32(mic_hitmap_word_len(w), tmp);
    for (int j = 0; j < n; ++j) put(tmp[j]);
  }
  put('\n');
}

#endif
