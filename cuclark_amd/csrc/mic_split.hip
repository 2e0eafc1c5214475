// mic_split.hip — a classified text split into its classified and its unclassified records on the device (include/mi_clark.h:
// mic_split_*; the rule: mic_split.h).  Three steps behind the query, on the slot's stream:
//   split_class_kernel   one thread per read: the class by the rule, the record's byte length (clipped to the text, + 1 for the line
//                        feed an unterminated text gets) into ONE 64-bit scan input - low word: classified bytes, high word:
//                        unclassified bytes.  A text is at most 128 MiB (+ 1), so neither half can carry into the other.
//   hipcub ExclusiveSum  over n + 1 items: item r = {classified bytes, unclassified bytes} in front of record r, item n = {a, b}.
//   split_copy_kernel    a stable partition of the text into one buffer: classified records at [0, a), unclassified at [a, a + b).
// The copy is one wavefront per record.  Records (~330 B for 150-bp FASTQ) begin at arbitrary byte offsets in the text and in the
// output, so the wave's lanes own ALIGNED 4-byte words of the destination; every word is put together from the two aligned source
// words it straddles with one byte funnel shift (v_alignbyte_b32), and only the at most three bytes in front of the first and behind
// the last whole word of a record are stored byte by byte.  Loads and stores are dwords at consecutive addresses across the wave.
#include "mi_clark.h"
#include "mic_internal.h"
#include "mic_split.h"

#include <hipcub/hipcub.hpp>

namespace {

__global__ void __launch_bounds__(256) split_class_kernel(const uint8_t* __restrict__ text, uint32_t nb, const uint32_t* __restrict__ starts,
                                                          uint32_t start_sub, const uint32_t* __restrict__ results,
                                                          const uint32_t* __restrict__ norm, uint32_t norm_sub, uint32_t n, int k,
                                                          uint32_t n_targets, mic_abund_filter f, unsigned long long* __restrict__ len2,
                                                          uint32_t* __restrict__ n_classified, const uint32_t* __restrict__ status) {
  if (status && *status) return;                  // the batch goes back to the host path, which splits it there
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool cls = false;
  if (r < n) {
    cls = mic_split_classified(results + (size_t)r * MIC_RESULT_WORDS, norm ? norm[r] - norm_sub : 0u, k, n_targets, f);
    const bool last = r + 1 == n;
    uint64_t s, e;
    mic_split_extent(starts[r] - start_sub, last ? 0u : starts[r + 1] - start_sub, last, nb, &s, &e);
    const unsigned long long len = (e - s) + (last ? mic_split_appends(text, nb) : 0u);
    len2[r] = cls ? len : len << 32;
  } else if (r == n) {
    len2[r] = 0;
  }
  const uint64_t m = __builtin_amdgcn_ballot_w64(cls);
  if (m && lane == __builtin_ctzll(m)) atomicAdd(n_classified, (uint32_t)__builtin_popcountll(m));
}

// One wavefront per record.  out_cap = nb + 1: a record that would end behind it (an index whose records overlap) is not copied.
__global__ void __launch_bounds__(256) split_copy_kernel(const uint8_t* __restrict__ text, uint32_t nb, const uint32_t* __restrict__ starts,
                                                         uint32_t start_sub, uint32_t n, const unsigned long long* __restrict__ off2,
                                                         int which, uint8_t* __restrict__ out, uint32_t out_cap,
                                                         const uint32_t* __restrict__ status) {
  if (status && *status) return;
  const int lane = threadIdx.x & 63;
  const uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (r >= n) return;
  const unsigned long long o = off2[r], d = off2[r + 1] - o;       // exactly one half of d is the record's length
  const bool cls = (uint32_t)d != 0 || d == 0;
  if (!(which & (cls ? MIC_SPLIT_CLASSIFIED : MIC_SPLIT_UNCLASSIFIED))) return;
  const uint32_t len = cls ? (uint32_t)d : (uint32_t)(d >> 32);
  const uint32_t dst = cls ? (uint32_t)o : (uint32_t)off2[n] + (uint32_t)(o >> 32);
  if (len == 0 || dst > out_cap || len > out_cap - dst) return;
  const bool last = r + 1 == n;
  uint64_t s64, e64;
  mic_split_extent(starts[r] - start_sub, last ? 0u : starts[r + 1] - start_sub, last, nb, &s64, &e64);
  const uint32_t src = (uint32_t)s64, real = (uint32_t)(e64 - s64);  // real = len, or len - 1 when the line feed is appended
  if (real > len) return;
  if (real < len && lane == 63) out[dst + real] = '\n';
  // head: up to the first aligned word of the destination; body: whole words; tail: what is left
  uint32_t head = (4u - (dst & 3u)) & 3u;
  if (head > real) head = real;
  const uint32_t words = (real - head) >> 2, tail = (real - head) & 3u;
  if ((uint32_t)lane < head) out[dst + lane] = text[src + lane];
  if ((uint32_t)lane >= 4u && (uint32_t)lane - 4u < tail) {
    const uint32_t j = head + 4u * words + ((uint32_t)lane - 4u);
    out[dst + j] = text[src + j];
  }
  if (words == 0) return;
  const uint32_t sb = src + head, sh = sb & 3u;
  const uint32_t* __restrict__ s32 = (const uint32_t*)(text + (sb - sh));
  uint32_t* __restrict__ d32 = (uint32_t*)(out + dst + head);
  if (sh == 0) {
    for (uint32_t i = lane; i < words; i += 64) d32[i] = s32[i];
  } else {
    // word i of the destination = bytes sb + 4 i .. sb + 4 i + 3: the top 4 - sh bytes of source word i and the low sh bytes of
    // source word i + 1, which holds a byte of the record (sh >= 1), so no load goes past the aligned word of the text's last byte
    for (uint32_t i = lane; i < words; i += 64) d32[i] = __builtin_amdgcn_alignbyte(s32[i + 1], s32[i], sh);
  }
}

}  // namespace

size_t mic_split_tmp_bytes(size_t n_items) {
  size_t tb = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)n_items);
  return tb + 256;
}

hipError_t mic_launch_split(const uint8_t* text, uint32_t nb, const uint32_t* starts, uint32_t start_sub, const uint32_t* results,
                            const uint32_t* norm, uint32_t norm_sub, uint32_t n, int k, uint32_t n_targets, const mic_abund_filter& f,
                            int which, const MicSplitBufs& b, uint8_t* out, const uint32_t* status, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(b.d_ncls, 0, 4, s);
  if (e != hipSuccess) return e;
  split_class_kernel<<<(n + 1 + 255) / 256, 256, 0, s>>>(text, nb, starts, start_sub, results, norm, norm_sub, n, k, n_targets, f, b.d_len2, b.d_ncls, status);
  size_t tb = b.tmp_bytes;
  e = hipcub::DeviceScan::ExclusiveSum(b.d_tmp, tb, b.d_len2, b.d_off2, (int)(n + 1), s);
  if (e != hipSuccess) return e;
  split_copy_kernel<<<(n + 3) / 4, 256, 0, s>>>(text, nb, starts, start_sub, n, b.d_off2, which, out, nb + 1, status);
  return hipGetLastError();
}

extern "C" {

int mic_split_start(mic_engine* e, const mic_abund_filter* filter, int which) {
  if (!e || !filter) return mic_set_error(MIC_E_INVALID, "null argument");
  if (!mic_abund_filter_ok(*filter)) return mic_set_error(MIC_E_INVALID, "split filter: denominators must be 10^0 .. 10^9 and numerators at most them");
  if (!mic_split_which_ok(which)) return mic_set_error(MIC_E_INVALID, "which = MIC_SPLIT_CLASSIFIED | MIC_SPLIT_UNCLASSIFIED, got %d", which);
  MicSplit& sp = *mic_engine_split(e);
  sp.filter = *filter; sp.which = which; sp.on = true;
  return MIC_OK;
}

int mic_split_stop(mic_engine* e) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  mic_engine_split(e)->on = false;
  return MIC_OK;
}

int mic_split_device(mic_engine* e, const uint8_t* d_text, size_t nb, const uint32_t* d_rec_start, size_t n_reads, const uint32_t* d_results,
                     const uint32_t* d_norm, const mic_abund_filter* filter, int which, uint8_t* d_out, uint64_t totals[4], void* stream) {
  if (!e || !filter || !totals || !d_text || !d_rec_start || !d_results || !d_out) return mic_set_error(MIC_E_INVALID, "null argument");
  if (!mic_abund_filter_ok(*filter)) return mic_set_error(MIC_E_INVALID, "split filter: denominators must be 10^0 .. 10^9 and numerators at most them");
  if (!mic_split_which_ok(which)) return mic_set_error(MIC_E_INVALID, "which = MIC_SPLIT_CLASSIFIED | MIC_SPLIT_UNCLASSIFIED, got %d", which);
  if (!d_norm && filter->gamma_num) return mic_set_error(MIC_E_INVALID, "a gamma threshold needs the reads' lengths (d_norm)");
  if (nb == 0 || nb > ((size_t)128 << 20) || n_reads == 0 || n_reads > nb) return mic_set_error(MIC_E_INVALID, "a text of 1 B .. 128 MiB with 1 .. nb records");
  if (((uintptr_t)d_text | (uintptr_t)d_out) & 3) return mic_set_error(MIC_E_INVALID, "the text and the output must be 4-byte aligned");
  MicTable t; int sc, ncu, dev, k; uint32_t nt;
  int rc = mic_engine_table(e, &t, &sc, &ncu, &dev, &k, &nt);
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : mic_engine_stream(e);
  void* d = nullptr;
  MicSplitBufs b;
  const size_t arr = ((n_reads + 1) * 8 + 255) & ~(size_t)255;
  unsigned long long tot = 0; uint32_t ncls = 0;
  MIC_TRY_DONE(hipSetDevice(dev));
  b.tmp_bytes = mic_split_tmp_bytes(n_reads + 1);
  MIC_TRY_DONE(hipMalloc(&d, 2 * arr + 256 + b.tmp_bytes));
  b.d_len2 = (unsigned long long*)d; b.d_off2 = (unsigned long long*)((char*)d + arr);
  b.d_ncls = (uint32_t*)((char*)d + 2 * arr); b.d_tmp = (char*)d + 2 * arr + 256;
  MIC_TRY_DONE(mic_launch_split(d_text, (uint32_t)nb, d_rec_start, 0, d_results, d_norm, 0, (uint32_t)n_reads, k, nt, *filter, which, b, d_out, nullptr, s));
  MIC_TRY_DONE(hipMemcpyAsync(&tot, b.d_off2 + n_reads, 8, hipMemcpyDeviceToHost, s));
  MIC_TRY_DONE(hipMemcpyAsync(&ncls, b.d_ncls, 4, hipMemcpyDeviceToHost, s));
  MIC_TRY_DONE(hipStreamSynchronize(s));
  totals[0] = (uint32_t)tot; totals[1] = tot >> 32; totals[2] = ncls; totals[3] = n_reads - ncls;
done:
  if (d) { hipStreamSynchronize(s); hipFree(d); }
  return rc;
}

}  // extern "C"
