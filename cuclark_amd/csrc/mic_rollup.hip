// mic_rollup.hip — rank roll-up on the device (include/mi_clark.h: mic_rollup_*; the rule: mic_rollup.h).
//
// Rows form (rollup_kernel).  One thread per read loads the row's first two words.  Rows of 0 or 1 entries - nearly all reads of a
// sample - are finished there: with one target hit every level's best is that count and its group a table lookup, so the read costs
// its row read and the 32-byte write.  Wider rows are then taken up by the wave: rows of up to 16 entries by the 16 lanes of the
// owner's quarter of the wave (four reads at a time), longer ones by all 64 lanes; entry j sits in lane j, its group at level l
// comes from group_of (at most 7 x 128 KB, L2-resident), every lane sums the counts of the lanes that share its group in one loop of
// lane broadcasts over the row's entries, the lowest lane of a group speaks for it, and best / second-best are two key-max
// reductions (dense_finish_kernel's key).  No loop per distinct group.  Counters: abund_kernel's ballot-aggregated 64-bit atomics.
//
// Dense form (rollup_dense_kernel): one block per listed read.  A level is a coarsening of the one below, so the targets sorted by
// their group (a permutation and segment starts per level, built by mic_rollup_set) make every group a contiguous segment: one
// thread per group sums its segment, no scatter, then the block's keys are reduced as in dense_finish_kernel.
#include "mi_clark.h"
#include "mic_internal.h"
#include "mic_abund.h"
#include "mic_rollup.h"

#include <string.h>

#include <vector>

namespace {

struct RollupArgs {
  const uint32_t* rows; const uint32_t* norm; const uint16_t* gof;
  uint32_t* rollup; uint32_t* levels; unsigned long long* counts; const uint32_t* status;
  uint32_t row_words, norm_sub, n, n_targets, n_levels;
  int k;
  uint32_t off[8];
  mic_abund_filter f;
};

constexpr uint32_t kNoBucket = 0xFFFFFFFFu;

template <int W>
__device__ inline uint32_t group_add(uint32_t v) {
#pragma unroll
  for (int d = W / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, W);
  return v;
}
template <int W>
__device__ inline unsigned long long group_max(unsigned long long v) {
#pragma unroll
  for (int d = W / 2; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d, W);
    v = o > v ? o : v;
  }
  return v;
}
// the bits of a wave ballot that belong to this lane's group of W lanes
template <int W>
__device__ inline uint64_t group_ballot(bool p, int lane) {
  const uint64_t m = __builtin_amdgcn_ballot_w64(p);
  return W == 64 ? m : (m >> (lane & ~(W - 1))) & ((1ull << (W & 63)) - 1);
}

__device__ inline void store_level(uint32_t* levels, size_t r, uint32_t n_levels, uint32_t l, const MicRollupLevel& lv) {
  *(uint4*)(levels + (r * (n_levels + 1) + l) * 4) = make_uint4(lv.ib, lv.best, lv.is, lv.second);
}

// W lanes (sub = 0 .. W - 1) hold read r's row of n entries, n <= W and n <= row_words - 1; n_loop >= n is wave-uniform.  Lanes of an
// inactive group run along (the shuffles need them) and touch no memory.  Returns the read's counter to every lane of the group.
template <int W>
__device__ inline uint32_t rollup_wide(const RollupArgs& a, bool active, size_t r, uint32_t n, uint32_t n_loop, uint32_t nm, int lane) {
  const int sub = lane & (W - 1);
  uint32_t e = 0;
  if (active && (uint32_t)sub < n) e = a.rows[r * a.row_words + 1 + sub];
  const uint32_t tgt = e & 0xFFFF;
  const uint32_t c = tgt < a.n_targets ? e >> 16 : 0u;        // (a target past the table's: ignored, as mic_abund_bucket prints "NA")
  const bool has = c != 0;
  const uint32_t sum = group_add<W>(c);
  MicRollupState st;
  mic_rollup_begin(st, sum, nm, a.k, a.f);
  {
    const unsigned long long key = mic_rollup_key(c, tgt);
    const unsigned long long best = group_max<W>(key);
    const unsigned long long second = group_max<W>(key == best ? 0ull : key);
    const MicRollupLevel lv = mic_rollup_level_of(best, second);
    const uint32_t nhit = (uint32_t)__builtin_popcountll(group_ballot<W>(has, lane));
    mic_rollup_push(st, 0, lv, nhit, 0, a.f);
    if (a.levels && active && sub == 0) store_level(a.levels, r, a.n_levels, 0, lv);
  }
#pragma unroll
  for (uint32_t l = 1; l <= MIC_ROLLUP_MAX_LEVELS; ++l) {
    if (l > a.n_levels) break;
    const uint32_t g = has ? a.gof[(size_t)(l - 1) * a.n_targets + tgt] : 0xFFFFFFFFu;
    uint32_t tot = 0;
    bool leader = has;
    for (uint32_t i = 0; i < n_loop; ++i) {
      const uint32_t gi = __shfl(g, (int)i, W), ci = __shfl(c, (int)i, W);
      const bool same = gi == g;
      tot += same ? ci : 0u;
      leader = leader && !(same && (int)i < sub);
    }
    const unsigned long long key = leader ? mic_rollup_key(tot, g) : 0ull;
    const unsigned long long best = group_max<W>(key);
    const unsigned long long second = group_max<W>(key == best ? 0ull : key);
    const MicRollupLevel lv = mic_rollup_level_of(best, second);
    const uint32_t nhit = (uint32_t)__builtin_popcountll(group_ballot<W>(leader, lane));
    mic_rollup_push(st, l, lv, nhit, a.off[l], a.f);
    if (a.levels && active && sub == 0) store_level(a.levels, r, a.n_levels, l, lv);
  }
  uint32_t out[MIC_ROLLUP_WORDS];
  const uint32_t bucket = mic_rollup_finish(st, sum, 0, out);
  if (active && sub == 0) {
    uint4* o = (uint4*)(a.rollup + r * MIC_ROLLUP_WORDS);
    o[0] = make_uint4(out[0], out[1], out[2], out[3]);
    o[1] = make_uint4(out[4], out[5], out[6], out[7]);
  }
  return bucket;
}

__global__ void __launch_bounds__(256) rollup_kernel(const RollupArgs a) {
  if (a.status && *a.status) return;              // the batch goes back to the host path, which counts it there
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t r_wave = r - lane;
  const bool valid = r < a.n;
  uint32_t n_ent = 0, first = 0, nm = 0, bucket = kNoBucket;
  if (valid) {
    const uint32_t* row = a.rows + (size_t)r * a.row_words;
    n_ent = row[0];
    if (a.norm) nm = a.norm[r] - a.norm_sub;
    if (n_ent >= 1 && n_ent <= a.row_words - 1) first = row[1];
  }
  const bool pending = valid && n_ent > a.row_words - 1;       // MIC_ROW_INVALID (or a count no row of this width can hold)
  const bool wide = valid && !pending && n_ent >= 2;
  if (valid && !wide) {
    uint4* o = (uint4*)(a.rollup + (size_t)r * MIC_ROLLUP_WORDS);
    const uint32_t tgt = first & 0xFFFF;
    const uint32_t c = (!pending && n_ent == 1 && tgt < a.n_targets) ? first >> 16 : 0u;
    if (pending) {
      o[0] = make_uint4(0, 0, 0, 0);
      o[1] = make_uint4(0, MIC_ROLLUP_PENDING, MIC_FLAG_ROW_OVERFLOW, 0);
    } else if (c == 0) {
      o[0] = make_uint4(0, 0, 0, 0); o[1] = make_uint4(0, 0, 0, 0);
      bucket = 0;
    } else {
      // one target hit: second is 0 at every level, so the confidence test holds at level 0 and only gamma decides
      const bool ok = mic_rollup_gamma_ok(c, nm, a.k, a.f);
      o[0] = make_uint4(c, tgt + 1, c, 0);
      o[1] = make_uint4(0, ok ? 0u : MIC_ROLLUP_UNRESOLVED, 0, 1);
      bucket = ok ? 2u + tgt : 1u;
    }
    if (a.levels) {
      MicRollupLevel lv; lv.ib = c ? tgt + 1 : 0u; lv.best = c; lv.is = 0; lv.second = 0;
      store_level(a.levels, r, a.n_levels, 0, lv);
      for (uint32_t l = 1; l <= a.n_levels; ++l) {
        lv.ib = c ? a.gof[(size_t)(l - 1) * a.n_targets + tgt] + 1u : 0u;
        store_level(a.levels, r, a.n_levels, l, lv);
      }
    }
  }
  // rows of 2 .. 16 entries: the owner's quarter of the wave takes them one after another, four quarters at a time
  uint32_t mine = (uint32_t)group_ballot<16>(wide && n_ent <= 16, lane);
  while (__builtin_amdgcn_ballot_w64(mine != 0)) {
    const bool active = mine != 0;
    const int owner = (lane & 48) + (active ? __builtin_ctz(mine) : 0);
    mine &= mine - 1;
    const uint32_t n_o = active ? (uint32_t)__shfl((int)n_ent, owner) : 0u;
    const uint32_t nm_o = (uint32_t)__shfl((int)nm, owner);
    uint32_t n_loop = n_o;
    n_loop = max(n_loop, (uint32_t)__shfl_xor((int)n_loop, 16));
    n_loop = max(n_loop, (uint32_t)__shfl_xor((int)n_loop, 32));
    n_loop = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_loop);
    const uint32_t b = rollup_wide<16>(a, active, (size_t)r_wave + owner, n_o, n_loop, nm_o, lane);
    if (active && lane == owner) bucket = b;
  }
  // longer rows (only when the engine's rows are wider than 16 words): the whole wave
  uint64_t m64 = __builtin_amdgcn_ballot_w64(wide && n_ent > 16);
  while (m64) {
    const int owner = __builtin_ctzll(m64);
    m64 &= m64 - 1;
    const uint32_t n_o = (uint32_t)__builtin_amdgcn_readlane((int)n_ent, owner);
    const uint32_t nm_o = (uint32_t)__builtin_amdgcn_readlane((int)nm, owner);
    const uint32_t b = rollup_wide<64>(a, true, (size_t)r_wave + owner, n_o, n_o, nm_o, lane);
    if (lane == owner) bucket = b;
  }
  if (!a.counts) return;
  uint64_t mm = __builtin_amdgcn_ballot_w64(bucket != kNoBucket);
  while (mm) {
    const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bucket, __builtin_ctzll(mm));
    const uint64_t same = __builtin_amdgcn_ballot_w64(bucket == b0);
    mm &= ~same;
    if (lane == __builtin_ctzll(same)) atomicAdd(&a.counts[b0], (unsigned long long)__builtin_popcountll(same));
  }
}

struct DenseArgs {
  const uint32_t* dense; const uint32_t* ids; const uint32_t* norm; const uint16_t* perm; const uint32_t* seg;
  uint32_t* rollup; uint32_t* levels; unsigned long long* counts;
  uint32_t n_targets, n_levels;
  int k;
  uint32_t n_groups[8], off[8], seg_off[8];
  mic_abund_filter f;
};

__global__ void __launch_bounds__(256) rollup_dense_kernel(const DenseArgs a) {
  const uint32_t r = a.ids ? a.ids[blockIdx.x] : blockIdx.x;
  const uint32_t* cnt = a.dense + (size_t)blockIdx.x * a.n_targets;
  __shared__ unsigned long long s_best[256], s_second[256];
  __shared__ uint32_t s_sum[256], s_n[256];
  MicRollupState st;
  uint32_t sum_all = 0;
  for (uint32_t l = 0; l <= a.n_levels; ++l) {
    const uint16_t* perm = l ? a.perm + (size_t)(l - 1) * a.n_targets : nullptr;
    const uint32_t* seg = l ? a.seg + a.seg_off[l] : nullptr;
    unsigned long long best = 0, second = 0; uint32_t sum = 0, nz = 0;
    for (uint32_t g = threadIdx.x; g < a.n_groups[l]; g += 256) {
      unsigned long long tot = 0;
      if (l == 0) tot = cnt[g];
      else for (uint32_t i = seg[g]; i < seg[g + 1]; ++i) tot += cnt[perm[i]];
      if (!tot) continue;
      mic_rollup_key_push(mic_rollup_key(tot, g), best, second);
      sum += (uint32_t)tot; ++nz;
    }
    s_best[threadIdx.x] = best; s_second[threadIdx.x] = second; s_sum[threadIdx.x] = sum; s_n[threadIdx.x] = nz;
    __syncthreads();
    if (threadIdx.x == 0) {
      best = 0; second = 0; sum = 0; nz = 0;
      for (int i = 0; i < 256; ++i) {
        mic_rollup_key_push(s_best[i], best, second);
        mic_rollup_key_push(s_second[i], best, second);
        sum += s_sum[i]; nz += s_n[i];
      }
      const MicRollupLevel lv = mic_rollup_level_of(best, second);
      if (l == 0) { sum_all = sum; mic_rollup_begin(st, sum, a.norm ? a.norm[r] : 0u, a.k, a.f); }
      mic_rollup_push(st, l, lv, nz, a.off[l], a.f);
      if (a.levels) store_level(a.levels, r, a.n_levels, l, lv);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    uint32_t out[MIC_ROLLUP_WORDS];
    const uint32_t bucket = mic_rollup_finish(st, sum_all, MIC_FLAG_DENSE_PATH, out);
    uint4* o = (uint4*)(a.rollup + (size_t)r * MIC_ROLLUP_WORDS);
    o[0] = make_uint4(out[0], out[1], out[2], out[3]);
    o[1] = make_uint4(out[4], out[5], out[6], out[7]);
    if (a.counts) atomicAdd(&a.counts[bucket], 1ull);
  }
}

}  // namespace

hipError_t mic_launch_rollup(const MicRollup& ru, const uint32_t* rows, uint32_t row_words, const uint32_t* norm, uint32_t norm_sub, size_t n,
                             int k, uint32_t n_targets, const mic_abund_filter& f, uint32_t* rollup, uint32_t* levels,
                             unsigned long long* counts, const uint32_t* status, hipStream_t s) {
  if (n == 0) return hipSuccess;
  RollupArgs a;
  a.rows = rows; a.norm = norm; a.gof = ru.d_group_of; a.rollup = rollup; a.levels = levels; a.counts = counts; a.status = status;
  a.row_words = row_words; a.norm_sub = norm_sub; a.n = (uint32_t)n; a.n_targets = n_targets; a.n_levels = ru.n_levels; a.k = k;
  for (int l = 0; l < 8; ++l) a.off[l] = ru.off[l];
  a.f = f;
  rollup_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(a);
  return hipGetLastError();
}

namespace {

const char* kFilterMsg = "roll-up filter: denominators must be 10^0 .. 10^9 and numerators at most them";

int engine_ctx(mic_engine* e, int* dev, int* k, uint32_t* nt) {
  MicTable t; int sc, ncu;
  return mic_engine_table(e, &t, &sc, &ncu, dev, k, nt);
}

int check_lineage(uint32_t T, uint32_t L, const uint16_t* group_of) {
  uint32_t bt = 0, bl = 0;
  const int c = mic_rollup_check_lineage(T, L, group_of, &bt, &bl);
  if (c < 0) return mic_set_error(MIC_E_INVALID, "a lineage has 1 .. %d levels over 1 .. 65535 targets", MIC_ROLLUP_MAX_LEVELS);
  if (c == 1) return mic_set_error(MIC_E_INVALID, "lineage level %u: the group of target %u is not numbered by first appearance", bl, bt);
  if (c == 2) return mic_set_error(MIC_E_INVALID, "lineage level %u is not a coarsening of level %u: target %u leaves the group its level-%u group belongs to", bl, bl - 1, bt, bl - 1);
  return MIC_OK;
}

}  // namespace

extern "C" {

int mic_rollup_check(uint32_t n_targets, uint32_t n_levels, const uint16_t* group_of) {
  return check_lineage(n_targets, n_levels, group_of);
}

int mic_rollup_set(mic_engine* e, uint32_t n_levels, const uint16_t* group_of) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  int dev, k; uint32_t T;
  int rc = engine_ctx(e, &dev, &k, &T);
  if (rc) return rc;
  MicRollup& ru = *mic_engine_rollup(e);
  if (ru.on) return mic_set_error(MIC_E_STATE, "roll-up counting is started on this engine: stop it before the lineage changes");
  if (n_levels && (rc = check_lineage(T, n_levels, group_of))) return rc;
  MIC_TRY(hipSetDevice(dev));
  MIC_TRY(hipDeviceSynchronize());
  if (ru.d_block) { MIC_TRY(hipFree(ru.d_block)); }
  if (ru.d_counts) { MIC_TRY(hipFree(ru.d_counts)); }
  ru = MicRollup();
  if (n_levels == 0) return MIC_OK;
  // per level: the targets sorted by group (stable), and where each group's segment starts
  std::vector<uint16_t> perm((size_t)n_levels * T);
  std::vector<uint32_t> seg;
  uint32_t n_groups[8] = {T}, seg_off[8] = {0};
  for (uint32_t l = 1; l <= n_levels; ++l) {
    const uint16_t* g = group_of + (size_t)(l - 1) * T;
    uint32_t G = 0;
    for (uint32_t t = 0; t < T; ++t) if (g[t] >= G) G = g[t] + 1u;
    n_groups[l] = G; seg_off[l] = (uint32_t)seg.size();
    std::vector<uint32_t> start(G + 1, 0);
    for (uint32_t t = 0; t < T; ++t) ++start[g[t] + 1];
    for (uint32_t i = 0; i < G; ++i) start[i + 1] += start[i];
    seg.insert(seg.end(), start.begin(), start.end());
    for (uint32_t t = 0; t < T; ++t) perm[(size_t)(l - 1) * T + start[g[t]]++] = (uint16_t)t;
  }
  const size_t b_gof = ((size_t)n_levels * T * 2 + 255) & ~(size_t)255, b_seg = seg.size() * 4;
  char* d = nullptr;
  MIC_TRY(hipMalloc(&d, 2 * b_gof + b_seg));
  hipError_t he = hipMemcpy(d, group_of, (size_t)n_levels * T * 2, hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(d + b_gof, perm.data(), perm.size() * 2, hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(d + 2 * b_gof, seg.data(), b_seg, hipMemcpyHostToDevice);
  if (he != hipSuccess) { hipFree(d); return mic_set_error(MIC_E_HIP, "uploading the lineage: %s", hipGetErrorString(he)); }
  ru.d_block = d; ru.d_group_of = (const uint16_t*)d; ru.d_perm = (const uint16_t*)(d + b_gof); ru.d_seg = (const uint32_t*)(d + 2 * b_gof);
  ru.n_levels = n_levels;
  uint32_t off = 0;
  for (uint32_t l = 0; l <= n_levels; ++l) { ru.n_groups[l] = n_groups[l]; ru.seg_off[l] = seg_off[l]; ru.off[l] = off; off += n_groups[l]; }
  ru.n_counters = 2 + off;
  return MIC_OK;
}

int mic_rollup_layout(const mic_engine* e, uint32_t* n_groups, uint64_t* n_counters) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  const MicRollup& ru = *mic_engine_rollup((mic_engine*)e);
  if (!ru.n_levels) return mic_set_error(MIC_E_STATE, "no lineage is set on this engine (mic_rollup_set)");
  if (n_groups) for (uint32_t l = 0; l <= ru.n_levels; ++l) n_groups[l] = ru.n_groups[l];
  if (n_counters) *n_counters = ru.n_counters;
  return (int)ru.n_levels;
}

int mic_rollup_device(mic_engine* e, const uint32_t* d_rows, const uint32_t* d_norm, size_t n_reads, const mic_abund_filter* filter,
                      uint32_t* d_rollup, uint32_t* d_levels, uint64_t* d_counts, void* stream) {
  if (!e || !filter || (n_reads && (!d_rows || !d_rollup))) return mic_set_error(MIC_E_INVALID, "null argument");
  if (!mic_abund_filter_ok(*filter)) return mic_set_error(MIC_E_INVALID, "%s", kFilterMsg);
  if (!d_norm && filter->gamma_num) return mic_set_error(MIC_E_INVALID, "a gamma threshold needs the reads' lengths (d_norm)");
  if (n_reads > 0xFFFFFF00ull) return mic_set_error(MIC_E_INVALID, "at most 2^32 - 256 reads per call");
  int dev, k; uint32_t nt;
  int rc = engine_ctx(e, &dev, &k, &nt);
  if (rc) return rc;
  const MicRollup& ru = *mic_engine_rollup(e);
  if (!ru.n_levels) return mic_set_error(MIC_E_STATE, "no lineage is set on this engine (mic_rollup_set)");
  MIC_TRY(hipSetDevice(dev));
  hipStream_t s = stream ? (hipStream_t)stream : mic_engine_stream(e);
  MIC_TRY(mic_launch_rollup(ru, d_rows, mic_engine_row_words(e), d_norm, 0, n_reads, k, nt, *filter, d_rollup, d_levels,
                         (unsigned long long*)d_counts, nullptr, s));
  return MIC_OK;
}

int mic_rollup_dense_device(mic_engine* e, const uint32_t* d_dense, const uint32_t* d_ids, size_t n_ids, const uint32_t* d_norm,
                            const mic_abund_filter* filter, uint32_t* d_rollup, uint32_t* d_levels, uint64_t* d_counts, void* stream) {
  if (!e || !filter || (n_ids && (!d_dense || !d_rollup))) return mic_set_error(MIC_E_INVALID, "null argument");
  if (!mic_abund_filter_ok(*filter)) return mic_set_error(MIC_E_INVALID, "%s", kFilterMsg);
  if (!d_norm && filter->gamma_num) return mic_set_error(MIC_E_INVALID, "a gamma threshold needs the reads' lengths (d_norm)");
  if (n_ids > 0x7FFFFFFFull) return mic_set_error(MIC_E_INVALID, "at most 2^31 - 1 reads per call");
  int dev, k; uint32_t nt;
  int rc = engine_ctx(e, &dev, &k, &nt);
  if (rc) return rc;
  const MicRollup& ru = *mic_engine_rollup(e);
  if (!ru.n_levels) return mic_set_error(MIC_E_STATE, "no lineage is set on this engine (mic_rollup_set)");
  if (n_ids == 0) return MIC_OK;
  MIC_TRY(hipSetDevice(dev));
  DenseArgs a;
  a.dense = d_dense; a.ids = d_ids; a.norm = d_norm; a.perm = ru.d_perm; a.seg = ru.d_seg; a.rollup = d_rollup; a.levels = d_levels;
  a.counts = (unsigned long long*)d_counts; a.n_targets = nt; a.n_levels = ru.n_levels; a.k = k;
  for (int l = 0; l < 8; ++l) { a.n_groups[l] = ru.n_groups[l]; a.off[l] = ru.off[l]; a.seg_off[l] = ru.seg_off[l]; }
  a.f = *filter;
  rollup_dense_kernel<<<(unsigned)n_ids, 256, 0, stream ? (hipStream_t)stream : mic_engine_stream(e)>>>(a);
  MIC_TRY(hipGetLastError());
  return MIC_OK;
}

int mic_rollup_start(mic_engine* e, const mic_abund_filter* filter) {
  if (!e || !filter) return mic_set_error(MIC_E_INVALID, "null argument");
  if (!mic_abund_filter_ok(*filter)) return mic_set_error(MIC_E_INVALID, "%s", kFilterMsg);
  int dev, k; uint32_t nt;
  int rc = engine_ctx(e, &dev, &k, &nt);
  if (rc) return rc;
  MicRollup& ru = *mic_engine_rollup(e);
  if (!ru.n_levels) return mic_set_error(MIC_E_STATE, "no lineage is set on this engine (mic_rollup_set)");
  MIC_TRY(hipSetDevice(dev));
  if (!ru.d_counts) MIC_TRY(hipMalloc(&ru.d_counts, (size_t)ru.n_counters * 8));
  MIC_TRY(hipDeviceSynchronize());             // (work still queued with the last run's counting)
  MIC_TRY(hipMemset(ru.d_counts, 0, (size_t)ru.n_counters * 8));
  ru.filter = *filter;
  ru.on = true;
  return MIC_OK;
}

int mic_rollup_fetch(mic_engine* e, uint64_t* counts, size_t n) {
  if (!e || !counts) return mic_set_error(MIC_E_INVALID, "null argument");
  MicRollup& ru = *mic_engine_rollup(e);
  if (!ru.d_counts) return mic_set_error(MIC_E_STATE, "roll-up counting was not started on this engine");
  if (n != ru.n_counters) return mic_set_error(MIC_E_INVALID, "the engine has %u roll-up counters (mic_rollup_layout), not %zu", ru.n_counters, n);
  int dev, k; uint32_t nt;
  int rc = engine_ctx(e, &dev, &k, &nt);
  if (rc) return rc;
  MIC_TRY(hipSetDevice(dev));
  MIC_TRY(hipDeviceSynchronize());
  MIC_TRY(hipMemcpy(counts, ru.d_counts, n * 8, hipMemcpyDeviceToHost));
  return MIC_OK;
}

int mic_rollup_stop(mic_engine* e) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  mic_engine_rollup(e)->on = false;
  return MIC_OK;
}

}  // extern "C"
