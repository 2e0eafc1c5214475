// mic_rollup.h — the rank roll-up rule, one definition for host and device (mic_rollup.hip's kernels, mic_rollup_host,
// exe/estimate_abundance --rank-report).  A read's per-target counts are summed along a lineage of L levels above the targets
// (group_of[l][t], l = 1 .. L; level 0 is the targets themselves), best / second-best are taken again at every level by the rule of
// result_rows_kernel (groups scanned in ascending id: strictly greater replaces best, else strictly greater replaces second), and
// the read is assigned at the LOWEST level that passes the two tests of mic_abund_bucket:
//   confidence  best * conf_den >= conf_num * (best + second)        (per level)
//   gamma       the test of mic_abund.h on sum, norm and k           (the same at every level)
// Roll-up row, MIC_ROLLUP_WORDS u32: {sum, idxBest, best, idxSecond, second, level, flags, nGroupsHit}; indices are group + 1,
// 0 = none; words 1-4 and 7 are the resolved level's (level 0's when no level passes: level = MIC_ROLLUP_UNRESOLVED).
// sum == 0: all words zero.  A row that is not available: level = MIC_ROLLUP_PENDING, flags = MIC_FLAG_ROW_OVERFLOW, nothing counted.
// Counters, u64 [2 + T + G_1 + .. + G_L]: [0] no hit, [1] unresolved, [2 + off_l + g] assigned to group g of level l.
//
// "Ascending scan" is restated as two maxima of the key (count << 16) | (0xFFFF - id) (dense_finish_kernel's): the largest key is
// the largest count with the lowest id, the largest of the rest is what the scan leaves as second (equal counts: the lower id).
#ifndef MIC_ROLLUP_H
#define MIC_ROLLUP_H

#include <stdint.h>

#include "mi_clark.h"
#include "mic_abund.h"

struct MicRollupLevel { uint32_t ib, best, is, second; };

MIC_AB_HD static inline unsigned long long mic_rollup_key(unsigned long long count, uint32_t id) {
  return count ? (count << 16) | (0xFFFFu - id) : 0ull;
}
MIC_AB_HD static inline void mic_rollup_key_push(unsigned long long key, unsigned long long& best, unsigned long long& second) {
  if (key > best) { second = best; best = key; } else if (key > second) second = key;
}
MIC_AB_HD static inline MicRollupLevel mic_rollup_level_of(unsigned long long best, unsigned long long second) {
  MicRollupLevel r;
  r.ib = best ? 0x10000u - (uint32_t)(best & 0xFFFF) : 0u; r.best = (uint32_t)(best >> 16);
  r.is = second ? 0x10000u - (uint32_t)(second & 0xFFFF) : 0u; r.second = (uint32_t)(second >> 16);
  return r;
}

MIC_AB_HD static inline bool mic_rollup_gamma_ok(uint32_t sum, uint32_t norm, int k, const mic_abund_filter& f) {
  const int64_t den = (int64_t)norm - k + 1;
  return f.gamma_num == 0 || (den > 0 && (uint64_t)sum * f.gamma_den >= f.gamma_num * (uint64_t)den);
}
MIC_AB_HD static inline bool mic_rollup_conf_ok(const MicRollupLevel& r, const mic_abund_filter& f) {
  return r.best != 0 && (uint64_t)r.best * f.conf_den >= f.conf_num * ((uint64_t)r.best + r.second);
}

// The resolution, level by level (ascending l, so that neither side keeps an array of levels): start with the read's sum, push
// every level's result with the number of groups hit there and the level's counter offset (off_l = T + G_1 + .. + G_(l-1), off_0 = 0),
// then finish: writes the roll-up row and returns the read's counter.
struct MicRollupState { uint32_t level, nhit, counter; bool gamma; MicRollupLevel at; };
MIC_AB_HD static inline void mic_rollup_begin(MicRollupState& s, uint32_t sum, uint32_t norm, int k, const mic_abund_filter& f) {
  s.level = MIC_ROLLUP_UNRESOLVED; s.nhit = 0; s.counter = 1; s.gamma = mic_rollup_gamma_ok(sum, norm, k, f);
  s.at.ib = s.at.best = s.at.is = s.at.second = 0;
}
MIC_AB_HD static inline void mic_rollup_push(MicRollupState& s, uint32_t l, const MicRollupLevel& lv, uint32_t nhit, uint32_t off_l,
                                             const mic_abund_filter& f) {
  const bool take = s.level == MIC_ROLLUP_UNRESOLVED && s.gamma && mic_rollup_conf_ok(lv, f);
  if (take) { s.level = l; s.counter = 2u + off_l + (lv.ib - 1); }
  if (take || l == 0) { s.at = lv; s.nhit = nhit; }
}
MIC_AB_HD static inline uint32_t mic_rollup_finish(const MicRollupState& s, uint32_t sum, uint32_t flags, uint32_t* out) {
  if (sum == 0) { for (int i = 0; i < MIC_ROLLUP_WORDS; ++i) out[i] = 0; return 0; }
  out[0] = sum; out[1] = s.at.ib; out[2] = s.at.best; out[3] = s.at.is; out[4] = s.at.second;
  out[5] = s.level; out[6] = flags; out[7] = s.nhit;
  return s.counter;
}

// One read on the host from its (target, count) pairs (counts > 0, targets < T): the per-level sums in tot[] (zero on entry and on
// return, as long as the largest level) with touched[] as the list of groups met (as long as n), levels (optional) and the roll-up
// row (out, MIC_ROLLUP_WORDS) written; returns the read's counter.  gamma_forced < 0: the gamma test is the rule's on norm and k;
// 0 / 1: decided by the caller (exe/estimate_abundance reads it off the CSV's Gamma column).
static inline uint32_t mic_rollup_read_host(const uint32_t* tg, const uint32_t* cn, size_t n, uint32_t T, uint32_t L, const uint16_t* group_of,
                                            const uint32_t* off, uint32_t norm, int k, const mic_abund_filter& f, int gamma_forced,
                                            uint32_t flags, uint64_t* tot, uint32_t* touched, uint32_t* out, uint32_t* lev) {
  uint32_t sum = 0;
  for (size_t i = 0; i < n; ++i) sum += cn[i];
  MicRollupState st;
  mic_rollup_begin(st, sum, norm, k, f);
  if (gamma_forced >= 0) st.gamma = gamma_forced != 0;
  for (uint32_t l = 0; l <= L; ++l) {
    const uint16_t* g = l ? group_of + (size_t)(l - 1) * T : nullptr;
    uint32_t nt = 0;
    for (size_t i = 0; i < n; ++i) {
      const uint32_t id = g ? g[tg[i]] : tg[i];
      if (!tot[id]) touched[nt++] = id;
      tot[id] += cn[i];
    }
    unsigned long long best = 0, second = 0;
    for (uint32_t i = 0; i < nt; ++i) { mic_rollup_key_push(mic_rollup_key(tot[touched[i]], touched[i]), best, second); tot[touched[i]] = 0; }
    const MicRollupLevel lv = mic_rollup_level_of(best, second);
    mic_rollup_push(st, l, lv, nt, off[l], f);
    if (lev) { lev[4 * l] = lv.ib; lev[4 * l + 1] = lv.best; lev[4 * l + 2] = lv.is; lev[4 * l + 3] = lv.second; }
  }
  return mic_rollup_finish(st, sum, flags, out);
}

// The two conditions on a lineage (group_of[(l - 1) * T + t], l = 1 .. L): ids numbered by first appearance in ascending target
// order, and every level a coarsening of the one below.  0 when it holds; else the offending target in *bad_t, its level in *bad_l
// and 1 (numbering) or 2 (coarsening) as the return value; -1 for a bad shape.
static inline int mic_rollup_check_lineage(uint32_t T, uint32_t L, const uint16_t* group_of, uint32_t* bad_t, uint32_t* bad_l) {
  if (T == 0 || T > 65535 || L == 0 || L > MIC_ROLLUP_MAX_LEVELS || !group_of) return -1;
  for (uint32_t l = 1; l <= L; ++l) {
    const uint16_t* g = group_of + (size_t)(l - 1) * T;
    uint32_t next = 0;
    for (uint32_t t = 0; t < T; ++t) {
      if (g[t] > next) { if (bad_t) *bad_t = t; if (bad_l) *bad_l = l; return 1; }
      if (g[t] == next) ++next;
    }
  }
  // coarsening: the group at level l is a function of the group at level l - 1 (level 0: always, a target is its own group)
  for (uint32_t l = 2; l <= L; ++l) {
    const uint16_t* lo = group_of + (size_t)(l - 2) * T;
    const uint16_t* hi = lo + T;
    uint32_t n_lo = 0;
    for (uint32_t t = 0; t < T; ++t) if (lo[t] >= n_lo) n_lo = lo[t] + 1u;
    uint16_t* par = new uint16_t[n_lo];
    uint8_t* seen = new uint8_t[n_lo]();
    int rc = 0;
    for (uint32_t t = 0; t < T && !rc; ++t) {
      if (!seen[lo[t]]) { seen[lo[t]] = 1; par[lo[t]] = hi[t]; }
      else if (par[lo[t]] != hi[t]) { if (bad_t) *bad_t = t; if (bad_l) *bad_l = l; rc = 2; }
    }
    delete[] par; delete[] seen;
    if (rc) return rc;
  }
  return 0;
}

#endif
