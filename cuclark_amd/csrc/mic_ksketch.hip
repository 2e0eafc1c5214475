// mic_ksketch.hip — k-mer sketches: distinct k-mers hit per target (include/mi_clark.h: mic_ksketch_*; the rule: mic_ksketch.h).
// The kernel and its launcher live in mic_kernels.hip, next to the probes they use (probe_any and what it calls); this file is the
// engine state and the C ABI around them.  An engine's sketches are ONE device allocation, num_targets * MIC_KSKETCH_REGS register
// bytes followed by num_targets u64 hit counters, made at mic_ksketch_start and freed with the engine: nothing is allocated or
// launched for an engine that never starts them.
#include "mi_clark.h"
#include "mic_internal.h"
#include "mic_ksketch.h"

extern "C" {

int mic_ksketch_start(mic_engine* e) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  MicTable t; int sc, ncu, dev, k; uint32_t nt;
  int rc = mic_engine_table(e, &t, &sc, &ncu, &dev, &k, &nt);
  if (rc) return rc;
  if (nt == 0) return mic_set_error(MIC_E_STATE, "the engine has no targets");
  MIC_TRY(hipSetDevice(dev));
  MicKsketch& ks = *mic_engine_ksketch(e);
  const size_t reg_bytes = (size_t)nt * MIC_KSKETCH_REGS, bytes = reg_bytes + (size_t)nt * 8;
  if (ks.d_regs && ks.n_targets != nt) {          // (the engine's number of targets is fixed at creation: not reached)
    MIC_TRY(hipDeviceSynchronize());
    MIC_TRY(hipFree(ks.d_regs));
    ks.d_regs = nullptr; ks.d_hits = nullptr;
  }
  if (!ks.d_regs) {
    void* d = nullptr;
    MIC_TRY(hipMalloc(&d, bytes));
    ks.d_regs = (uint8_t*)d;
    ks.d_hits = (unsigned long long*)((uint8_t*)d + reg_bytes);      // (reg_bytes is a multiple of 16 KiB: aligned)
    ks.n_targets = nt;
  }
  MIC_TRY(hipDeviceSynchronize());             // (work still queued with the last run's sketching)
  MIC_TRY(hipMemset(ks.d_regs, 0, bytes));
  ks.on = true;
  return MIC_OK;
}

int mic_ksketch_fetch(mic_engine* e, uint8_t* regs, size_t n_regs, uint64_t* hits, size_t n_hits) {
  if (!e || !regs || !hits) return mic_set_error(MIC_E_INVALID, "null argument");
  MicKsketch& ks = *mic_engine_ksketch(e);
  if (!ks.d_regs) return mic_set_error(MIC_E_STATE, "k-mer sketches were not started on this engine");
  if (n_regs != (size_t)ks.n_targets * MIC_KSKETCH_REGS || n_hits != ks.n_targets)
    return mic_set_error(MIC_E_INVALID, "the sketches have %zu registers and %u hit counters, not %zu and %zu", (size_t)ks.n_targets * MIC_KSKETCH_REGS,
                         ks.n_targets, n_regs, n_hits);
  MicTable t; int sc, ncu, dev, k; uint32_t nt;
  int rc = mic_engine_table(e, &t, &sc, &ncu, &dev, &k, &nt);
  if (rc) return rc;
  MIC_TRY(hipSetDevice(dev));
  MIC_TRY(hipDeviceSynchronize());
  MIC_TRY(hipMemcpy(regs, ks.d_regs, n_regs, hipMemcpyDeviceToHost));
  MIC_TRY(hipMemcpy(hits, ks.d_hits, n_hits * 8, hipMemcpyDeviceToHost));
  return MIC_OK;
}

int mic_ksketch_stop(mic_engine* e) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  mic_engine_ksketch(e)->on = false;
  return MIC_OK;
}

int mic_ksketch_device(mic_engine* e, const uint32_t* d_reads_pointer, const uint16_t* d_containers, size_t n_reads, const uint32_t* d_results,
                       uint8_t* d_regs, uint64_t* d_hits, void* stream) {
  if (!e || (n_reads && (!d_reads_pointer || !d_containers || !d_results || !d_regs || !d_hits))) return mic_set_error(MIC_E_INVALID, "null argument");
  if (n_reads > 0xFFFFFFFFull) return mic_set_error(MIC_E_INVALID, "at most 2^32 - 1 reads per call");
  if (((uintptr_t)d_regs & 3) || ((uintptr_t)d_hits & 7) || ((uintptr_t)d_reads_pointer & 3) || ((uintptr_t)d_containers & 1) || ((uintptr_t)d_results & 3))
    return mic_set_error(MIC_E_INVALID, "d_regs must be 4-byte aligned, d_hits 8-byte aligned, the reads and results as for mic_query_device");
  MicTable t; int sc, ncu, dev, k; uint32_t nt;
  int rc = mic_engine_table(e, &t, &sc, &ncu, &dev, &k, &nt);
  if (rc) return rc;
  if (!t.slots) return mic_set_error(MIC_E_STATE, "no database loaded");
  MIC_TRY(hipSetDevice(dev));
  hipStream_t s = stream ? (hipStream_t)stream : mic_engine_stream(e);
  MIC_TRY(mic_launch_ksketch(t, sc, ncu, d_reads_pointer, d_containers, n_reads, d_results, nt, d_regs, (unsigned long long*)d_hits, nullptr, s));
  return MIC_OK;
}

}  // extern "C"
