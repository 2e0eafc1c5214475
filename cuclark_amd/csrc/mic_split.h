// mic_split.h — the read-splitting rule, one definition for host and device (mic_split.hip's kernels, mic_split_host,
// exe/split_reads).  A classified text is handed back as two texts: the records that were assigned and the records that were not.
//   records  Record r of a text of nb bytes is the bytes [start[r], start[r + 1]) - from the first byte of its header line up to the
//            first byte of the next record's header line; the last record runs to nb.  The records tile the text: start[0] = 0,
//            starts ascend, nothing lies between two records.  (Device: the slot's record index; host: mic_index_reads, name_s - 1.)
//   classes  Record r is CLASSIFIED iff mic_abund_bucket(result_r, norm_r, k, n_targets, filter) >= 2: it counts for a target under
//            the abundance filter (mic_abund.h).  It is UNCLASSIFIED otherwise: bucket 0 (no hit) or 1 (dropped by the filter).
//   output   Each class's records in input order, byte for byte.  Every record but the last ends where a header line begins, so
//            behind a '\n'; when the text's last byte is not '\n' (an unterminated last line) the last record gets one '\n'
//            appended - the only byte ever added.  Both classes go into ONE buffer of nb + 1 bytes: classified records at [0, a),
//            unclassified records at [a, a + b), a + b = nb or nb + 1.
#ifndef MIC_SPLIT_H
#define MIC_SPLIT_H

#include <stdint.h>

#include "mic_abund.h"

MIC_AB_HD static inline bool mic_split_classified(const uint32_t* res, uint32_t norm, int k, uint32_t n_targets, const mic_abund_filter& f) {
  return mic_abund_bucket(res, norm, k, n_targets, f) >= 2;
}

// bytes of the text that record r holds: [*s, *e), both clipped to nb and e >= s whatever the index says
MIC_AB_HD static inline void mic_split_extent(uint64_t start, uint64_t next, bool last, uint64_t nb, uint64_t* s, uint64_t* e) {
  uint64_t a = start < nb ? start : nb;
  uint64_t b = last ? nb : (next < nb ? next : nb);
  if (b < a) b = a;
  *s = a; *e = b;
}

// 1 when the text's last record gets a '\n' appended
MIC_AB_HD static inline uint32_t mic_split_appends(const uint8_t* text, uint64_t nb) { return nb && text[nb - 1] != '\n' ? 1u : 0u; }

static inline bool mic_split_which_ok(int which) { return which >= 1 && which <= 3; }

#include <string.h>
// The partition on the CPU for any class predicate is_classified(r) (mic_split_host: the rule on result rows; exe/split_reads: the
// classes read from a CSV): classified records to out[0, a), unclassified to out[a, a + b), totals = {a, b, classified records,
// unclassified records}.  Two passes over the records: the totals (where the unclassified records begin), then the copy.  False,
// nothing written, when the starts do not tile the text (start[0] = 0, ascending, below nb).
template <typename IsClassified>
static inline bool mic_split_partition_host(const uint8_t* text, size_t nb, const uint64_t* start, size_t n, int which, IsClassified is_classified,
                                            uint8_t* out, uint64_t totals[4]) {
  if (n && (nb == 0 || start[0] != 0)) return false;
  for (size_t r = 0; r < n; ++r)
    if (start[r] >= nb || (r && start[r] <= start[r - 1])) return false;
  const uint32_t add = n ? mic_split_appends(text, nb) : 0u;
  uint64_t a = 0, b = 0, na = 0, nu = 0;
  for (int pass = 0; pass < 2; ++pass) {
    uint64_t oa = 0, ob = a;
    for (size_t r = 0; r < n; ++r) {
      const bool last = r + 1 == n;
      uint64_t s, e;
      mic_split_extent(start[r], last ? nb : start[r + 1], last, nb, &s, &e);
      const uint64_t len = e - s + (last ? add : 0u);
      const bool cls = is_classified(r);
      if (pass == 0) { if (cls) { a += len; ++na; } else { b += len; ++nu; } continue; }
      uint64_t& o = cls ? oa : ob;
      if (which & (cls ? 1 : 2)) {
        memcpy(out + o, text + s, e - s);
        if (last && add) out[o + (e - s)] = '\n';
      }
      o += len;
    }
  }
  totals[0] = a; totals[1] = b; totals[2] = na; totals[3] = nu;
  return true;
}

#endif
