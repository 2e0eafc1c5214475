// mic_hitmap.hip — hit maps: per read, the runs of k-mer assignments along it (include/mi_clark.h: mic_hitmap_*; the rule: mic_hitmap.h).
// The kernel and its launcher live in mic_kernels.hip, next to the probes they use (probe_any and what it calls); the text kernels and
// the slot's buffers live in mic_ingest.hip, next to the CSV kernels whose pattern they follow.  This file is the engine state, the
// scan between the kernel's two passes and the C ABI of the stand-alone call.
//   pass 1   hitmap_kernel<*, false>   the words per read
//   scan     hipcub ExclusiveSum over n_reads + 1 items: the offsets, item n_reads = the total
//   pass 2   hitmap_kernel<*, true>    the words at their offsets
// The table is probed twice.  The alternative that probes once is a worst-case buffer of one word per k-mer position - four times the
// bytes of the text the reads came from - for maps that are a few words per read on real data; the second pass costs what the
// k-mer sketches' pass costs and the map is exact for any batch: it is never truncated.
#include "mi_clark.h"
#include "mic_internal.h"
#include "mic_hitmap.h"
#include "mic_abund.h"

#include <hipcub/hipcub.hpp>

size_t mic_hitmap_tmp_bytes(size_t n_items) {
  size_t tb = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)n_items);
  return tb + 256;
}

hipError_t mic_hitmap_scan(void* d_tmp, size_t tmp_bytes, const uint32_t* counts, uint32_t* offsets, size_t n_items, hipStream_t s) {
  size_t tb = tmp_bytes;
  return hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, counts, offsets, (int)n_items, s);
}

int mic_hitmap_run(const MicTable& t, int slot_class, int n_cu, const uint32_t* d_rp, const uint16_t* d_cont, size_t n_reads,
                   const uint32_t* d_results, uint32_t n_targets, uint32_t* d_offsets, uint32_t* d_words, size_t cap_words, uint64_t* n_words,
                   hipStream_t s) {
  int rc = MIC_OK;
  void* d = nullptr;
  uint32_t total = 0, n_cont = 0;
  const size_t arr = ((n_reads + 1) * 4 + 255) & ~(size_t)255, tmp = mic_hitmap_tmp_bytes(n_reads + 1);
  *n_words = 0;
  if (n_reads == 0) {
    MIC_TRY_DONE(hipMemsetAsync(d_offsets, 0, 4, s));
    MIC_TRY_DONE(hipStreamSynchronize(s));
    return MIC_OK;
  }
  // a word per k-mer position and a separator per part at the most: fewer than 8 per container, so the 32-bit offsets cannot wrap
  MIC_TRY_DONE(hipMemcpyAsync(&n_cont, d_rp + n_reads, 4, hipMemcpyDeviceToHost, s));
  MIC_TRY_DONE(hipStreamSynchronize(s));
  if (n_cont >= (1u << 29)) {
    rc = mic_set_error(MIC_E_UNSUPPORTED, "hit maps: %u containers in one call may need more than 2^32 - 1 words: split the reads", n_cont);
    goto done;
  }
  MIC_TRY_DONE(hipMalloc(&d, arr + tmp));
  MIC_TRY_DONE(mic_launch_hitmap(t, slot_class, n_cu, d_rp, d_cont, n_reads, d_results, n_targets, nullptr, (uint32_t*)d, false, s));
  MIC_TRY_DONE(mic_hitmap_scan((char*)d + arr, tmp, (const uint32_t*)d, d_offsets, n_reads + 1, s));
  MIC_TRY_DONE(hipMemcpyAsync(&total, d_offsets + n_reads, 4, hipMemcpyDeviceToHost, s));
  MIC_TRY_DONE(hipStreamSynchronize(s));
  *n_words = total;
  if (d_words && total && total <= cap_words) {
    MIC_TRY_DONE(mic_launch_hitmap(t, slot_class, n_cu, d_rp, d_cont, n_reads, d_results, n_targets, d_offsets, d_words, true, s));
    MIC_TRY_DONE(hipStreamSynchronize(s));
  }
done:
  if (d) { hipStreamSynchronize(s); hipFree(d); }
  return rc;
}

extern "C" {

int mic_hitmap_start(mic_engine* e) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  MicTable t; int sc, ncu, dev, k; uint32_t nt;
  int rc = mic_engine_table(e, &t, &sc, &ncu, &dev, &k, &nt);
  if (rc) return rc;
  if (t.slots && (t.sharded || t.parted)) return mic_set_error(MIC_E_UNSUPPORTED, "hit maps on a sharded or parted table: not supported");
  MicHitmap* hm = mic_engine_hitmap(e);
  if (hm->on && hm->kraken) return mic_set_error(MIC_E_STATE, "the Kraken format is started on this engine: the two texts share the slots' buffers");
  hm->on = true;
  return MIC_OK;
}

int mic_hitmap_stop(mic_engine* e) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  MicHitmap* hm = mic_engine_hitmap(e);
  if (!hm->kraken) hm->on = false;
  return MIC_OK;
}

// the hit-map product in Kraken format (mic_kraken.h): the same engine state with another text behind the same words
int mic_kraken_start(mic_engine* e, const mic_abund_filter* filter) {
  if (!e || !filter) return mic_set_error(MIC_E_INVALID, "null argument");
  if (!mic_abund_filter_ok(*filter)) return mic_set_error(MIC_E_INVALID, "a filter threshold is num / 10^d with d <= 9 and num <= 10^d");
  MicTable t; int sc, ncu, dev, k; uint32_t nt;
  int rc = mic_engine_table(e, &t, &sc, &ncu, &dev, &k, &nt);
  if (rc) return rc;
  if (t.slots && (t.sharded || t.parted)) return mic_set_error(MIC_E_UNSUPPORTED, "the Kraken format on a sharded or parted table: not supported");
  MicHitmap* hm = mic_engine_hitmap(e);
  if (hm->on && !hm->kraken) return mic_set_error(MIC_E_STATE, "hit maps are started on this engine: the two texts share the slots' buffers");
  hm->on = true; hm->kraken = true; hm->filter = *filter;
  return MIC_OK;
}

int mic_kraken_stop(mic_engine* e) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  MicHitmap* hm = mic_engine_hitmap(e);
  if (hm->kraken) { hm->on = false; hm->kraken = false; }
  return MIC_OK;
}

int mic_hitmap_device(mic_engine* e, const uint32_t* d_reads_pointer, const uint16_t* d_containers, size_t n_reads, const uint32_t* d_results,
                      uint32_t* d_offsets, uint32_t* d_words, size_t cap_words, uint64_t* n_words, void* stream) {
  if (!e || !d_offsets || !n_words || (n_reads && (!d_reads_pointer || !d_containers || !d_results))) return mic_set_error(MIC_E_INVALID, "null argument");
  if (n_reads >= 0xFFFFFFFFull) return mic_set_error(MIC_E_INVALID, "at most 2^32 - 2 reads per call");
  if (((uintptr_t)d_offsets & 3) || ((uintptr_t)d_words & 3) || ((uintptr_t)d_reads_pointer & 3) || ((uintptr_t)d_containers & 1) || ((uintptr_t)d_results & 3))
    return mic_set_error(MIC_E_INVALID, "d_offsets and d_words must be 4-byte aligned, the reads and results as for mic_query_device");
  MicTable t; int sc, ncu, dev, k; uint32_t nt;
  int rc = mic_engine_table(e, &t, &sc, &ncu, &dev, &k, &nt);
  if (rc) return rc;
  if (!t.slots) return mic_set_error(MIC_E_STATE, "no database loaded");
  if (t.sharded || t.parted) return mic_set_error(MIC_E_UNSUPPORTED, "hit maps on a sharded or parted table: not supported");
  hipError_t he = hipSetDevice(dev);
  if (he != hipSuccess) return mic_set_error(MIC_E_HIP, "hipSetDevice: %s", hipGetErrorString(he));
  hipStream_t s = stream ? (hipStream_t)stream : mic_engine_stream(e);
  return mic_hitmap_run(t, sc, ncu, d_reads_pointer, d_containers, n_reads, d_results, nt, d_offsets, d_words, cap_words, n_words, s);
}

}  // extern "C"
