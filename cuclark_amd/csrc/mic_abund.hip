// mic_abund.hip — abundance counting on the device (include/mi_clark.h: mic_abundance_*; the rule: mic_abund.h).
//
// One thread per read computes the read's bucket; the wave then adds its reads bucket by bucket: a ballot loop over the distinct
// buckets of the wave (as tally_counts sums per label, mic_kernels.hip), one 64-bit global atomicAdd per bucket per wave.  The
// adds are exact and commute, so the counters do not depend on the order of waves, slots or batches.  Most reads of a sample
// fall into a few buckets, so a wave issues a handful of atomics instead of 64.
#include "mi_clark.h"
#include "mic_internal.h"
#include "mic_abund.h"

#include <string.h>

namespace {

__global__ void __launch_bounds__(256) abund_kernel(const uint32_t* __restrict__ results, const uint32_t* __restrict__ norm, uint32_t norm_sub,
                                                    uint32_t n, int k, uint32_t n_targets, mic_abund_filter f,
                                                    unsigned long long* __restrict__ counts, const uint32_t* __restrict__ status) {
  if (status && *status) return;                  // the batch goes back to the host path, which counts it there
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool valid = r < n;
  uint32_t b = 0;
  if (valid) b = mic_abund_bucket(results + (size_t)r * MIC_RESULT_WORDS, norm ? norm[r] - norm_sub : 0u, k, n_targets, f);
  uint64_t mm = __builtin_amdgcn_ballot_w64(valid);
  while (mm) {
    const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)b, __builtin_ctzll(mm));
    const uint64_t same = __builtin_amdgcn_ballot_w64(valid && b == b0);
    mm &= ~same;
    if (lane == __builtin_ctzll(same)) atomicAdd(&counts[b0], (unsigned long long)__builtin_popcountll(same));
  }
}

mic_abund_filter filter_of(const MicAbund& a) {
  mic_abund_filter f;
  f.conf_num = a.conf_num; f.conf_den = a.conf_den; f.gamma_num = a.gamma_num; f.gamma_den = a.gamma_den;
  return f;
}

}  // namespace

hipError_t mic_launch_abund(const uint32_t* results, const uint32_t* norm, uint32_t norm_sub, size_t n, int k, uint32_t n_targets,
                            const MicAbund& a, unsigned long long* counts, const uint32_t* status, hipStream_t s) {
  if (n == 0) return hipSuccess;
  abund_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(results, norm, norm_sub, (uint32_t)n, k, n_targets, filter_of(a), counts, status);
  return hipGetLastError();
}

extern "C" {

int mic_abundance_start(mic_engine* e, const mic_abund_filter* filter) {
  if (!e || !filter) return mic_set_error(MIC_E_INVALID, "null argument");
  if (!mic_abund_filter_ok(*filter)) return mic_set_error(MIC_E_INVALID, "abundance filter: denominators must be 10^0 .. 10^9 and numerators at most them");
  MicTable t; int sc, ncu, dev, k; uint32_t nt;
  int rc = mic_engine_table(e, &t, &sc, &ncu, &dev, &k, &nt);
  if (rc) return rc;
  MIC_TRY(hipSetDevice(dev));
  MicAbund& a = *mic_engine_abund(e);
  if (!a.d_counts || a.n_words != nt + 2) {
    if (a.d_counts) { MIC_TRY(hipDeviceSynchronize()); MIC_TRY(hipFree(a.d_counts)); a.d_counts = nullptr; }
    MIC_TRY(hipMalloc(&a.d_counts, (size_t)(nt + 2) * 8));
    a.n_words = nt + 2;
  }
  MIC_TRY(hipDeviceSynchronize());             // (work still queued with the last run's counting)
  MIC_TRY(hipMemset(a.d_counts, 0, (size_t)a.n_words * 8));
  a.conf_num = filter->conf_num; a.conf_den = filter->conf_den; a.gamma_num = filter->gamma_num; a.gamma_den = filter->gamma_den;
  a.on = true;
  return MIC_OK;
}

int mic_abundance_fetch(mic_engine* e, uint64_t* counts, size_t n) {
  if (!e || !counts) return mic_set_error(MIC_E_INVALID, "null argument");
  MicAbund& a = *mic_engine_abund(e);
  if (!a.d_counts) return mic_set_error(MIC_E_STATE, "abundance counting was not started on this engine");
  if (n != a.n_words) return mic_set_error(MIC_E_INVALID, "the engine has %u counters (num_targets + 2), not %zu", a.n_words, n);
  MicTable t; int sc, ncu, dev, k; uint32_t nt;
  int rc = mic_engine_table(e, &t, &sc, &ncu, &dev, &k, &nt);
  if (rc) return rc;
  MIC_TRY(hipSetDevice(dev));
  MIC_TRY(hipDeviceSynchronize());
  MIC_TRY(hipMemcpy(counts, a.d_counts, n * 8, hipMemcpyDeviceToHost));
  return MIC_OK;
}

int mic_abundance_stop(mic_engine* e) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  mic_engine_abund(e)->on = false;
  return MIC_OK;
}

int mic_abundance_device(mic_engine* e, const uint32_t* d_results, const uint32_t* d_norm, size_t n_reads, const mic_abund_filter* filter,
                         uint64_t* d_counts, void* stream) {
  if (!e || !filter || (n_reads && (!d_results || !d_counts))) return mic_set_error(MIC_E_INVALID, "null argument");
  if (!mic_abund_filter_ok(*filter)) return mic_set_error(MIC_E_INVALID, "abundance filter: denominators must be 10^0 .. 10^9 and numerators at most them");
  if (!d_norm && filter->gamma_num) return mic_set_error(MIC_E_INVALID, "a gamma threshold needs the reads' lengths (d_norm)");
  if (n_reads > 0xFFFFFFFFull) return mic_set_error(MIC_E_INVALID, "at most 2^32 - 1 reads per call");
  MicTable t; int sc, ncu, dev, k; uint32_t nt;
  int rc = mic_engine_table(e, &t, &sc, &ncu, &dev, &k, &nt);
  if (rc) return rc;
  MIC_TRY(hipSetDevice(dev));
  MicAbund a;
  a.conf_num = filter->conf_num; a.conf_den = filter->conf_den; a.gamma_num = filter->gamma_num; a.gamma_den = filter->gamma_den;
  hipStream_t s = stream ? (hipStream_t)stream : mic_engine_stream(e);
  MIC_TRY(mic_launch_abund(d_results, d_norm, 0, n_reads, k, nt, a, (unsigned long long*)d_counts, nullptr, s));
  return MIC_OK;
}

}  // extern "C"
