// mic_density.hip — score densities counted on the device (include/mi_clark.h: mic_density_*; the rule: mic_density.h).
//
// One kernel, a capped grid of 256-thread blocks striding over the batch's reads.  A block keeps a private u32[5151] histogram of the
// joint table in LDS (20.6 KB: seven blocks fit a CU's 160 KiB), zeroes it, adds one to the cell of every assigned read with an LDS
// atomic whose result is not used (ds_add_u32), and at the end adds only its non-zero cells to the global u64 counters.  The reads
// seen and the unassigned ones are counted from ballots, a wave's total at a time, and leave the block as one global atomic each.
// All adds are exact and commute: the counters do not depend on the order of waves, blocks, slots, engines or batches.
//
// A real sample piles most reads into a few cells (every single-target read sits in the c = 100 row), so the lanes of a wave often
// hit ONE LDS address, which the LDS then serves a lane at a time.  The wave therefore pre-aggregates the cell of its first
// assigned lane (kAggLeader): one ballot finds the lanes that share it, the first of them adds their number, the other lanes add
// one each as before.  This choice is NOT measured yet ("NOT measured"): it rests on the argument there.  The two
// alternatives stay compiled so that the measurement can be made, picked with MIC_DENSITY_AGG (measuring only): 0 = one add per
// lane, 2 = abund_kernel's ballot loop over all distinct cells; tests/test_density_gpu.py runs all three forms.
#include "mi_clark.h"
#include "mic_internal.h"
#include "mic_density.h"

#include <stdlib.h>

namespace {

constexpr uint32_t kReadsPerBlock = 1024;       // below this many reads per block the grid shrinks instead: every block pays a zero and a flush of the table

enum { kAggNone = 0, kAggLeader = 1, kAggAll = 2 };

template <int AGG>
__global__ void __launch_bounds__(256) density_kernel(const uint32_t* __restrict__ results, const uint32_t* __restrict__ norm, uint32_t norm_sub,
                                                      uint32_t n, int k, uint32_t n_targets, unsigned long long* __restrict__ counts,
                                                      const uint32_t* __restrict__ status) {
  if (status && *status) return;                  // the batch goes back to the host path, which counts it there
  __shared__ uint32_t hist[MIC_DENSITY_CELLS];
  __shared__ uint32_t tot[2];                     // the block's reads seen, unassigned
  for (uint32_t i = threadIdx.x; i < MIC_DENSITY_CELLS; i += 256) hist[i] = 0;
  if (threadIdx.x < 2) tot[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  uint32_t w_seen = 0, w_un = 0;                  // wave-uniform
  // 64-bit read index: the stride may carry it past 2^32 for n near 2^32 - 1; base is uniform in the wave, so its lanes stay together
  for (uint64_t base = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n; base += (uint64_t)gridDim.x * 256) {
    const uint64_t r = base + lane;
    const bool valid = r < n;
    uint32_t cell = MIC_DENSITY_NONE;
    if (valid) cell = mic_density_cell(results + r * MIC_RESULT_WORDS, norm ? norm[r] - norm_sub : 0u, k, n_targets);
    const bool hit = cell != MIC_DENSITY_NONE;    // (mic_density_cell: below MIC_DENSITY_CELLS then, whatever the row holds)
    const uint64_t vm = __builtin_amdgcn_ballot_w64(valid), hm = __builtin_amdgcn_ballot_w64(hit);
    w_seen += (uint32_t)__builtin_popcountll(vm);
    w_un += (uint32_t)__builtin_popcountll(vm & ~hm);
    if (AGG == kAggLeader) {
      if (hm) {
        const int first = __builtin_ctzll(hm);
        const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)cell, first);
        const uint64_t same = __builtin_amdgcn_ballot_w64(hit && cell == c0);
        if (lane == first) atomicAdd(&hist[c0], (uint32_t)__builtin_popcountll(same));
        else if (hit && cell != c0) atomicAdd(&hist[cell], 1u);
      }
    } else if (AGG == kAggAll) {
      uint64_t mm = hm;
      while (mm) {
        const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)cell, __builtin_ctzll(mm));
        const uint64_t same = __builtin_amdgcn_ballot_w64(hit && cell == c0);
        mm &= ~same;
        if (lane == __builtin_ctzll(same)) atomicAdd(&hist[c0], (uint32_t)__builtin_popcountll(same));
      }
    } else if (hit) {
      atomicAdd(&hist[cell], 1u);
    }
  }
  if (lane == 0) { atomicAdd(&tot[0], w_seen); atomicAdd(&tot[1], w_un); }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < MIC_DENSITY_CELLS; i += 256) {
    const uint32_t v = hist[i];
    if (v) atomicAdd(&counts[2 + i], (unsigned long long)v);
  }
  if (threadIdx.x < 2 && tot[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)tot[threadIdx.x]);
}

}  // namespace

hipError_t mic_launch_density(const uint32_t* results, const uint32_t* norm, uint32_t norm_sub, size_t n, int k, uint32_t n_targets,
                              int n_cu, unsigned long long* counts, const uint32_t* status, hipStream_t s) {
  if (n == 0) return hipSuccess;
  // a block's u32 cells hold its share of at most 2^32 - 1 reads; two blocks per CU at the most
  const size_t cap = (size_t)(n_cu > 0 ? n_cu : 256) * 2;
  size_t blocks = (n + kReadsPerBlock - 1) / kReadsPerBlock;
  if (blocks > cap) blocks = cap;
  // measuring only: exactly "0" or "2" picks an alternative, anything else is the default
  static const int agg = [] {
    const char* v = getenv("MIC_DENSITY_AGG");
    return v && v[0] == '0' && !v[1] ? (int)kAggNone : v && v[0] == '2' && !v[1] ? (int)kAggAll : (int)kAggLeader;
  }();
  auto* kern = agg == kAggNone ? density_kernel<kAggNone> : agg == kAggAll ? density_kernel<kAggAll> : density_kernel<kAggLeader>;
  kern<<<(unsigned)blocks, 256, 0, s>>>(results, norm, norm_sub, (uint32_t)n, k, n_targets, counts, status);
  return hipGetLastError();
}

extern "C" {

int mic_density_start(mic_engine* e) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  MicTable t; int sc, ncu, dev, k; uint32_t nt;
  int rc = mic_engine_table(e, &t, &sc, &ncu, &dev, &k, &nt);
  if (rc) return rc;
  MIC_TRY(hipSetDevice(dev));
  MicDensity& d = *mic_engine_density(e);
  if (!d.d_counts) MIC_TRY(hipMalloc(&d.d_counts, (size_t)MIC_DENSITY_WORDS * 8));
  MIC_TRY(hipDeviceSynchronize());             // (work still queued with the last run's counting)
  MIC_TRY(hipMemset(d.d_counts, 0, (size_t)MIC_DENSITY_WORDS * 8));
  d.on = true;
  return MIC_OK;
}

int mic_density_fetch(mic_engine* e, uint64_t* counts, size_t n) {
  if (!e || !counts) return mic_set_error(MIC_E_INVALID, "null argument");
  MicDensity& d = *mic_engine_density(e);
  if (!d.d_counts) return mic_set_error(MIC_E_STATE, "density counting was not started on this engine");
  if (n != MIC_DENSITY_WORDS) return mic_set_error(MIC_E_INVALID, "the density has %d counters (MIC_DENSITY_WORDS), not %zu", MIC_DENSITY_WORDS, n);
  MicTable t; int sc, ncu, dev, k; uint32_t nt;
  int rc = mic_engine_table(e, &t, &sc, &ncu, &dev, &k, &nt);
  if (rc) return rc;
  MIC_TRY(hipSetDevice(dev));
  MIC_TRY(hipDeviceSynchronize());
  MIC_TRY(hipMemcpy(counts, d.d_counts, n * 8, hipMemcpyDeviceToHost));
  return MIC_OK;
}

int mic_density_stop(mic_engine* e) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  mic_engine_density(e)->on = false;
  return MIC_OK;
}

int mic_density_device(mic_engine* e, const uint32_t* d_results, const uint32_t* d_norm, size_t n_reads, uint64_t* d_counts, void* stream) {
  if (!e || (n_reads && (!d_results || !d_counts))) return mic_set_error(MIC_E_INVALID, "null argument");
  if (n_reads > 0xFFFFFFFFull) return mic_set_error(MIC_E_INVALID, "at most 2^32 - 1 reads per call");
  MicTable t; int sc, ncu, dev, k; uint32_t nt;
  int rc = mic_engine_table(e, &t, &sc, &ncu, &dev, &k, &nt);
  if (rc) return rc;
  MIC_TRY(hipSetDevice(dev));
  hipStream_t s = stream ? (hipStream_t)stream : mic_engine_stream(e);
  MIC_TRY(mic_launch_density(d_results, d_norm, 0, n_reads, k, nt, ncu, (unsigned long long*)d_counts, nullptr, s));
  return MIC_OK;
}

}  // extern "C"
