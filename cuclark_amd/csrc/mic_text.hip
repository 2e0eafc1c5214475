// mic_text.hip — the line indexer (bytes -> line ends per 4-KiB tile -> line starts; mic_internal.h), which an ingest slot's batch
// (mic_ingest.hip: index_records) shares with the texts that are RESIDENT on the device, and the index of those: a whole inflated
// FASTQ / FASTA file or a pair of mates (include/mi_clark.h: mic_text_*, mic_pairs_*), which hand record ranges to a slot.
#include "mi_clark.h"
#include "mic_internal.h"
#include "mic_qmask.h"

#include <hipcub/hipcub.hpp>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

namespace {

#define ING_TILE MIC_LINE_TILE // bytes per block of the line kernels (256 threads x 16 B)

__device__ __forceinline__ uint32_t newline_mask(uint32_t x) {       // 0x80 in every byte of x that is '\n'
  const uint32_t y = x ^ 0x0A0A0A0Au;
  return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
}

// newline flags of the 16 bytes at byte offset `pos` (16-byte aligned): bit i = byte i is '\n' and lies below nb
// (from: bytes below it are not the text's - the front of an aligned-down buffer, mic_text_index_front_device)
__device__ __forceinline__ uint32_t tile_flags(const uint8_t* __restrict__ raw, uint32_t pos, uint32_t nb, uint32_t from = 0) {
  if (pos >= nb || pos + 16 <= from) return 0;
  const uint4 v = *(const uint4*)(raw + pos);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t f = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t m = newline_mask(w[i]);     // bits 7, 15, 23, 31
    f |= (((m >> 7) & 1u) | ((m >> 14) & 2u) | ((m >> 21) & 4u) | ((m >> 28) & 8u)) << (4 * i);
  }
  const uint32_t left = nb - pos;
  if (left < 16) f &= (1u << left) - 1u;
  if (pos < from) f &= ~((1u << (from - pos)) - 1u);
  return f;
}

__global__ void __launch_bounds__(256) line_count_kernel(const uint8_t* __restrict__ raw, uint32_t nb, uint32_t* __restrict__ tile_cnt, uint32_t from = 0) {
  __shared__ uint32_t s_w[4];
  const uint32_t pos = blockIdx.x * ING_TILE + threadIdx.x * 16;
  uint32_t c = __popc(tile_flags(raw, pos, nb, from));
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// line_start[L] = offset of the first byte of line L (line 0 starts at 0; a '\n' at p starts the next line at p + 1)
__global__ void __launch_bounds__(256) line_start_kernel(const uint8_t* __restrict__ raw, uint32_t nb, const uint32_t* __restrict__ tile_off,
                                                         uint32_t* __restrict__ line_start, uint32_t cap, uint32_t from = 0) {
  __shared__ uint32_t s_w[4];
  const uint32_t pos = blockIdx.x * ING_TILE + threadIdx.x * 16;
  uint32_t f = tile_flags(raw, pos, nb, from);
  const uint32_t c = __popc(f);
  uint32_t inc = c;                               // inclusive scan inside the wave
  const int lane = threadIdx.x & 63;
  for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(inc, off); if (lane >= off) inc += t; }
  if (lane == 63) s_w[threadIdx.x >> 6] = inc;
  __syncthreads();
  uint32_t base = tile_off[blockIdx.x];
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) base += s_w[w];
  uint32_t rank = base + inc - c;                 // newlines before this thread's bytes
  if (blockIdx.x == 0 && threadIdx.x == 0) line_start[0] = from;
  while (f) {
    const int b = __ffs((int)f) - 1;
    f &= f - 1;
    ++rank;
    if (rank < cap) line_start[rank] = pos + (uint32_t)b + 1u;
  }
}

// ---- a pair of FASTQ texts resident on the device (the inflated mates of -P a.fq.gz b.fq.gz): line index, checks, merge --------------
// The reference merges a pair line by line into ">id\nseq1Nseq2\n" (file.cc:205-268); the command line's loaders do that on the
// host for plain files.  Text that was inflated ON the device (mic_gz.hip) is merged here instead, record ranges straight into an
// ingest slot's device buffer, so that the text never crosses the link.  What the line arithmetic does not cover (line counts that
// differ or are no multiple of four, a header without '@', ids that differ or are empty) is reported, and the caller goes back to
// the host reader, which treats such files the way the reference does, messages included.
enum { PS_LINES = MIC_PAIRS_LINES, PS_HEADER = MIC_PAIRS_HEADER, PS_ID = MIC_PAIRS_ID, PS_BIG = MIC_PAIRS_BIG };

__device__ __forceinline__ bool pair_sep(uint8_t c) { return c == ' ' || c == '/' || c == '\t' || c == '@'; }     // file.cc:224
// the id inside a header line [p, p + n): behind leading separators, up to the next one
__device__ __forceinline__ void pair_id(const uint8_t* __restrict__ p, uint32_t n, uint32_t& a, uint32_t& len) {
  a = 0;
  while (a < n && pair_sep(p[a])) ++a;
  uint32_t b = a;
  while (b < n && !pair_sep(p[b])) ++b;
  len = b - a;
}

struct PairText { const uint8_t* t; const uint32_t* ls; uint32_t nb; };
// line L of a text without its '\n' (an unterminated last line has its virtual line end at nb: line_start = nb + 1)
__device__ __forceinline__ void pair_line(const PairText& x, uint64_t L, const uint8_t*& p, uint32_t& n) {
  const uint32_t a = x.ls[L], b = x.ls[L + 1];
  p = x.t + a; n = b - 1u - a;
}

// one thread per record: checks, and the length of the merged record
__global__ void __launch_bounds__(256) pair_len_kernel(PairText A, PairText B, uint64_t n_rec, unsigned long long* __restrict__ mlen,
                                                       uint32_t* __restrict__ status) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > n_rec) return;
  if (r == n_rec) { mlen[r] = 0; return; }
  const uint8_t *p, *q; uint32_t n, m;
  pair_line(A, 4 * r, p, n); pair_line(B, 4 * r, q, m);
  uint32_t bad = 0, ia = 0, la = 0, ib = 0, lb = 0;
  if (n == 0 || m == 0 || p[0] != '@' || q[0] != '@') bad |= PS_HEADER;
  else {
    pair_id(p, n, ia, la); pair_id(q, m, ib, lb);
    if (la == 0 || la != lb) bad |= PS_ID;
    else for (uint32_t i = 0; i < la; ++i) if (p[ia + i] != q[ib + i]) { bad |= PS_ID; break; }
  }
  const uint32_t s1 = A.ls[4 * r + 2] - 1u - A.ls[4 * r + 1], s2 = B.ls[4 * r + 2] - 1u - B.ls[4 * r + 1];
  mlen[r] = (unsigned long long)la + 2u + s1 + 1u + s2 + 1u;
  if (bad) atomicOr(status, bad);
}

__global__ void __launch_bounds__(256) pair_sample_kernel(const unsigned long long* __restrict__ off, uint64_t n_rec, uint32_t stride,
                                                          uint64_t n_samples, unsigned long long* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_samples) return;
  const uint64_t r = i * stride;
  out[i] = off[r < n_rec ? r : n_rec];
}

// a single FASTQ text: out[i] = byte offset of record min(i * stride, n_rec) (line 4 r; behind the last record: the end of the text)
__global__ void __launch_bounds__(256) text_sample_kernel(const uint32_t* __restrict__ ls, uint32_t nb, uint64_t n_rec, uint32_t stride,
                                                          uint64_t n_samples, unsigned long long* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_samples) return;
  const uint64_t r = i * stride < n_rec ? i * stride : n_rec;
  const uint32_t o = ls[4 * r];
  out[i] = o < nb ? o : nb;
}

// FASTA: flag[L] = line L starts a record ('>' in its first column, CuCLARK_hh.hh:1369-1389); flag[n_lines] = 0 for the scan's total
__global__ void __launch_bounds__(256) text_fasta_flag_kernel(const uint8_t* __restrict__ raw, uint32_t nb, const uint32_t* __restrict__ ls,
                                                              uint64_t n_lines, uint32_t* __restrict__ flag) {
  const uint64_t L = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (L > n_lines) return;
  uint32_t f = 0;
  if (L < n_lines) { const uint32_t p = ls[L]; f = p < nb && raw[p] == '>'; }
  flag[L] = f;
}
// out[r / stride] = byte offset of record r for every stride-th record; the entries behind the last one: the end of the text
__global__ void __launch_bounds__(256) text_fasta_sample_kernel(const uint32_t* __restrict__ ls, const uint32_t* __restrict__ flag,
                                                                const uint32_t* __restrict__ rec_of_line, uint64_t n_lines, uint32_t stride,
                                                                unsigned long long* __restrict__ out) {
  const uint64_t L = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (L >= n_lines || !flag[L]) return;
  const uint32_t r = rec_of_line[L];
  if (r % stride == 0) out[r / stride] = ls[L];
}

// (the device code of this file is loaded when its first kernel is launched: mic_ingest_alloc does that through mic_text_warm)
__global__ void text_warm_kernel(uint32_t* p) { if (p && threadIdx.x == 1000) *p = 0; }

// what the host wants to know about a text once its line ends are counted, gathered for ONE small copy (a copy into pageable host
// memory costs about a millisecond whatever its size): out[0] = line ends, out[1] = last byte, out[2] = first byte
__global__ void text_facts_kernel(const uint8_t* __restrict__ raw, uint32_t nb, const uint32_t* __restrict__ tile_off, uint32_t n_tiles,
                                  uint32_t* __restrict__ out, uint32_t from = 0) {
  out[0] = tile_off[n_tiles]; out[1] = raw[nb - 1]; out[2] = raw[from]; out[3] = 0;
}

// one wavefront per record: ">id\n" seq1 "N" seq2 "\n" at off[r] - off[r0]
// QUAL (a threshold byte c0 is set on the engine): each mate's sequence is copied with 'N' in place of every base its own quality
// line (line 4r + 3 of its text) masks (mic_qmask.h); the lengths are those of pair_len_kernel either way
template <bool QUAL>
__global__ void __launch_bounds__(256) pair_merge_kernel(PairText A, PairText B, uint64_t r0, uint64_t r1, const unsigned long long* __restrict__ off,
                                                         uint8_t* __restrict__ dst, uint32_t c0) {
  const int lane = threadIdx.x & 63;
  const uint64_t r = r0 + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= r1) return;
  uint8_t* o = dst + (off[r] - off[r0]);
  const uint8_t *p, *q; uint32_t n, m;
  pair_line(A, 4 * r, p, n);
  uint32_t ia, la;
  pair_id(p, n, ia, la);
  if (lane == 0) o[0] = '>';
  for (uint32_t i = lane; i < la; i += 64) o[1 + i] = p[ia + i];
  if (lane == 0) o[1 + la] = '\n';
  o += la + 2;
  const uint8_t* u = nullptr; uint32_t un = 0;       // QUAL: the mate's quality line
  pair_line(A, 4 * r + 1, p, n);
  if (QUAL) pair_line(A, 4 * r + 3, u, un);
  for (uint32_t i = lane; i < n; i += 64) o[i] = (QUAL && mic_qmask_masked(u, un, i, c0)) ? (uint8_t)'N' : p[i];
  if (lane == 0) o[n] = 'N';
  o += n + 1;
  pair_line(B, 4 * r + 1, q, m);
  if (QUAL) pair_line(B, 4 * r + 3, u, un);
  for (uint32_t i = lane; i < m; i += 64) o[i] = (QUAL && mic_qmask_masked(u, un, i, c0)) ? (uint8_t)'N' : q[i];
  if (lane == 0) o[m] = '\n';
}

void launch_pair_merge(const PairText& A, const PairText& B, uint64_t r0, uint64_t r1, const unsigned long long* off, uint8_t* dst, uint32_t c0,
                       hipStream_t st) {
  const unsigned blocks = (unsigned)((r1 - r0 + 3) / 4);
  if (c0) pair_merge_kernel<true><<<blocks, 256, 0, st>>>(A, B, r0, r1, off, dst, c0);
  else pair_merge_kernel<false><<<blocks, 256, 0, st>>>(A, B, r0, r1, off, dst, 0u);
}

// ---- host side: what the two handles share -------------------------------------------------------------------------------------------
// An index is two device allocations and no hipFree on the way (each costs about a millisecond and a device-wide wait): a scratch
// block for the line counts, then - once the numbers of lines are known - one block for everything that depends on them.
struct TextIndex {
  int device = 0; uint64_t n_rec = 0; uint32_t stride = 64;
  void* d_scratch = nullptr; void* d_block = nullptr;     // the two device allocations everything of the handle is carved from
  std::vector<unsigned long long> samples;      // byte offset of record i * stride for the host's batch arithmetic, then the text's end
  ~TextIndex() { hipSetDevice(device); if (d_scratch) hipFree(d_scratch); if (d_block) hipFree(d_block); }
  // byte offset of record r, for r a multiple of the stride or r == n_rec
  bool offset_of(uint64_t r, unsigned long long& off) const {
    if (r != n_rec && (r > n_rec || r % stride)) return false;
    off = r == n_rec ? samples.back() : samples[r / stride];
    return true;
  }
  // records [r0, r1) are the bytes [o0, o1)
  int range(uint64_t r0, uint64_t r1, unsigned long long& o0, unsigned long long& o1) const {
    if (r0 >= r1 || !offset_of(r0, o0) || !offset_of(r1, o1))
      return mic_set_error(MIC_E_INVALID, "records [%llu, %llu): not a range of whole strides", (unsigned long long)r0, (unsigned long long)r1);
    return MIC_OK;
  }
};

int index_offsets(const TextIndex* p, const uint64_t** samples, size_t* n_samples, uint32_t* stride) {
  if (!p || !samples || !n_samples || !stride) return mic_set_error(MIC_E_INVALID, "null argument");
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
  *samples = (const uint64_t*)p->samples.data(); *n_samples = p->samples.size(); *stride = p->stride;
  return MIC_OK;
}

// One or two texts between the two phases of an index.  It lives in run_index's frame until the last wait for the stream: facts,
// virt_end and n_rec32 are host ends of asynchronous copies, which have to outlive them.
struct Scan {
  struct Text {
    const uint8_t* raw; uint32_t nb, from;        // the text is raw[from, nb) (mic_internal.h: mic_line_ends)
    uint32_t n_tiles; uint32_t* d_tile_off;       // in the handle's scratch block
    uint32_t nl; uint8_t first, last;             // line ends; the text's first and last byte
    uint64_t n_lines; uint32_t virt_end;          // nl, + 1 for an unterminated last line, which has its virtual line end at nb
  } x[2];
  int n;
  uint32_t facts[8], n_rec32;                     // text_facts_kernel's four words per text; FASTA: the number of records
};

// MIC_GZ_TIMING=1: the host time from one point of mic_pairs_index_device to the next (tools/gz_* read these lines)
void lap(double* tl, const char* what) { if (!tl) return; const double t = now_s(); fprintf(stderr, "[pairs] %s: %.3f ms\n", what, (t - *tl) * 1e3); *tl = t; }
size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// phase 1 of an index, for all texts of sc at once: ONE scratch allocation carved per text, line ends and facts per text, ONE small
// copy of all facts (16 bytes per text) and one wait
int count_lines(TextIndex* p, Scan& sc, hipStream_t st, double* tl) {
  size_t arr[2] = {0, 0}, tmp_bytes = 0; uint32_t* d_tile[2];
  for (int i = 0; i < sc.n; ++i) {
    const uint32_t nt = sc.x[i].n_tiles = mic_line_tiles(sc.x[i].nb);
    tmp_bytes = std::max(tmp_bytes, mic_line_scan_bytes(nt)); arr[i] = up256(((size_t)nt + 1) * 4);
  }
  MIC_TRY(hipMalloc(&p->d_scratch, 2 * arr[0] + 2 * arr[1] + 256 + up256(tmp_bytes + 16)));
  char* q = (char*)p->d_scratch;
  for (int i = 0; i < sc.n; ++i) { d_tile[i] = (uint32_t*)q; q += arr[i]; sc.x[i].d_tile_off = (uint32_t*)q; q += arr[i]; }
  uint32_t* d_facts = (uint32_t*)q; void* d_tmp = q + 256;
  lap(tl, "scratch allocated");
  for (int i = 0; i < sc.n; ++i) {
    const Scan::Text& x = sc.x[i];
    MIC_TRY(mic_line_ends(x.raw, x.nb, x.from, d_tile[i], x.d_tile_off, d_tmp, tmp_bytes, st));
    text_facts_kernel<<<1, 1, 0, st>>>(x.raw, x.nb, x.d_tile_off, x.n_tiles, d_facts + 4 * i, x.from);
  }
  MIC_TRY(hipGetLastError());
  MIC_TRY(hipMemcpyAsync(sc.facts, d_facts, 16 * (size_t)sc.n, hipMemcpyDeviceToHost, st));
  MIC_TRY(hipStreamSynchronize(st));
  for (int i = 0; i < sc.n; ++i) {
    Scan::Text& x = sc.x[i]; const uint32_t* f = sc.facts + 4 * i;
    x.nl = f[0]; x.last = (uint8_t)f[1]; x.first = (uint8_t)f[2]; x.n_lines = (uint64_t)x.nl + (x.last != '\n' ? 1 : 0);
  }
  lap(tl, "lines counted");
  return MIC_OK;
}

// phase 2: the line starts of one text into d_ls (n_lines + 2 entries of the block the caller has sized), and the virtual line end of
// an unterminated last line (lines_finish_kernel's convention)
int line_starts(Scan::Text& x, uint32_t* d_ls, hipStream_t st) {
  MIC_TRY(mic_line_starts(x.raw, x.nb, x.from, x.d_tile_off, d_ls, (uint32_t)std::min<uint64_t>(x.n_lines + 2, 0xFFFFFFFFull), st));
  x.virt_end = x.nb + 1;
  if (x.last != '\n') MIC_TRY(hipMemcpyAsync(d_ls + x.n_lines, &x.virt_end, 4, hipMemcpyHostToDevice, st));
  return MIC_OK;
}

// One index from end to end: e's device made current, `body` on a new handle and on e's upload stream (one of its own would cost 2 ms
// to create), the last wait.  The handle goes out unless body failed, set *status or found no record.
template <typename H, typename Body>
int run_index(mic_engine* e, H** out, uint64_t* n_records, uint32_t* status, Body body) {
  MicTable t; int sl, ncu, dev, k; uint32_t nt; hipStream_t st, down;
  if (int rc = mic_engine_table(e, &t, &sl, &ncu, &dev, &k, &nt)) return rc;
  if (hipSetDevice(dev) != hipSuccess) return mic_set_error(MIC_E_HIP, "hipSetDevice failed");
  mic_engine_copy_streams(e, &st, &down);
  H* p = new H; p->device = dev;
  Scan sc = {};
  const int rc = body(p, sc, st);
  hipStreamSynchronize(st);
  if (rc != MIC_OK || *status || p->n_rec == 0) { delete p; return rc; }
  *out = p; *n_records = p->n_rec;
  return MIC_OK;
}

}  // namespace

struct mic_text : TextIndex {
  const uint8_t* t = nullptr; uint32_t nb = 0;    // the text as the kernels see it: from the 4-KiB boundary below its first byte
  uint32_t* d_ls = nullptr; bool fasta = false;
};

struct mic_pairs : TextIndex {
  PairText t[2];
  uint32_t* d_ls[2] = {nullptr, nullptr}; unsigned long long* d_off = nullptr;     // d_off[r] = bytes of merged text in front of record r (n_rec + 1 entries)
};

// ---- the line indexer (mic_internal.h) -----------------------------------------------------------------------------------------------
size_t mic_line_scan_bytes(size_t n_tiles) {
  size_t tb = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)(n_tiles + 1));
  return tb;
}

hipError_t mic_line_ends(const uint8_t* raw, uint32_t nb, uint32_t from, uint32_t* d_tile, uint32_t* d_tile_off, void* d_scan, size_t scan_bytes, hipStream_t s) {
  const uint32_t n_tiles = mic_line_tiles(nb);
  line_count_kernel<<<n_tiles, 256, 0, s>>>(raw, nb, d_tile, from);
  const hipError_t e = hipMemsetAsync(d_tile + n_tiles, 0, 4, s);
  return e != hipSuccess ? e : hipcub::DeviceScan::ExclusiveSum(d_scan, scan_bytes, d_tile, d_tile_off, (int)(n_tiles + 1), s);
}

hipError_t mic_line_starts(const uint8_t* raw, uint32_t nb, uint32_t from, const uint32_t* d_tile_off, uint32_t* d_line_start, uint32_t cap, hipStream_t s) {
  line_start_kernel<<<mic_line_tiles(nb), 256, 0, s>>>(raw, nb, d_tile_off, d_line_start, cap, from);
  return hipGetLastError();
}
hipError_t mic_text_warm(hipStream_t s) { text_warm_kernel<<<1, 64, 0, s>>>(nullptr); return hipGetLastError(); }

namespace {

// a pair: lines -> pair checks, merged offsets, samples
int index_pairs(mic_pairs* p, Scan& sc, hipStream_t st, uint32_t* status) {
  static const bool timing = getenv("MIC_GZ_TIMING") != nullptr;
  double t0 = timing ? now_s() : 0, *tl = timing ? &t0 : nullptr;
  if (int rc = count_lines(p, sc, st, tl)) return rc;
  const uint64_t n_lines = sc.x[0].n_lines;
  if (n_lines != sc.x[1].n_lines || n_lines % 4 != 0 || n_lines == 0) { *status = PS_LINES; return MIC_OK; }
  const uint64_t n_rec = p->n_rec = n_lines / 4, n_samples = n_rec / p->stride + 2;
  size_t tmp2 = 0;
  MIC_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp2, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)(n_rec + 1), st));
  const size_t b_ls = up256((n_lines + 2) * 4), b_off = up256((n_rec + 1) * 8), b_smp = up256(n_samples * 8);
  MIC_TRY(hipMalloc(&p->d_block, 2 * b_ls + 2 * b_off + b_smp + 256 + up256(tmp2 + 16)));
  char* q = (char*)p->d_block;
  p->d_ls[0] = (uint32_t*)q; q += b_ls; p->d_ls[1] = (uint32_t*)q; q += b_ls;
  p->d_off = (unsigned long long*)q; q += b_off;
  unsigned long long* d_mlen = (unsigned long long*)q; q += b_off;
  unsigned long long* d_samples = (unsigned long long*)q; q += b_smp;
  uint32_t* d_status = (uint32_t*)q; q += 256;
  void* d_tmp2 = q;
  lap(tl, "index block allocated");
  for (int i = 0; i < 2; ++i) {
    if (int rc = line_starts(sc.x[i], p->d_ls[i], st)) return rc;
    p->t[i].t = sc.x[i].raw; p->t[i].ls = p->d_ls[i]; p->t[i].nb = sc.x[i].nb;
  }
  MIC_TRY(hipMemsetAsync(d_status, 0, 4, st));
  pair_len_kernel<<<(unsigned)((n_rec + 1 + 255) / 256), 256, 0, st>>>(p->t[0], p->t[1], n_rec, d_mlen, d_status);
  MIC_TRY(hipGetLastError());
  MIC_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp2, tmp2, d_mlen, p->d_off, (int)(n_rec + 1), st));
  p->samples.resize(n_samples);
  pair_sample_kernel<<<(unsigned)((n_samples + 255) / 256), 256, 0, st>>>(p->d_off, n_rec, p->stride, n_samples, d_samples);
  MIC_TRY(hipGetLastError());
  MIC_TRY(hipMemcpyAsync(p->samples.data(), d_samples, n_samples * 8, hipMemcpyDeviceToHost, st));
  MIC_TRY(hipMemcpyAsync(status, d_status, 4, hipMemcpyDeviceToHost, st));
  MIC_TRY(hipStreamSynchronize(st));
  lap(tl, "line starts, pair checks, offsets, samples");
  return MIC_OK;
}

// FASTA: a record is a '>' line and what follows it up to the next one (sequences over several lines)
int index_fasta(mic_text* p, Scan& sc, hipStream_t st, uint32_t* status) {
  Scan::Text& x = sc.x[0]; const uint64_t n_lines = x.n_lines;
  p->fasta = true;
  if (n_lines >= 0x7FFFFFF0ull) { *status = PS_BIG; return MIC_OK; }
  size_t tmp2 = 0;
  MIC_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp2, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)(n_lines + 1), st));
  // (the samples are sized by the lines - there are no more records than lines - and cut down once the count is known)
  const size_t b_ls = up256((n_lines + 2) * 4), b_fl = up256((n_lines + 1) * 4), b_smp = up256((n_lines / p->stride + 2) * 8);
  MIC_TRY(hipMalloc(&p->d_block, b_ls + 2 * b_fl + b_smp + up256(tmp2 + 16)));
  char* q = (char*)p->d_block;
  p->d_ls = (uint32_t*)q; q += b_ls;
  uint32_t* d_flag = (uint32_t*)q; q += b_fl;
  uint32_t* d_rec = (uint32_t*)q; q += b_fl;
  unsigned long long* d_samples = (unsigned long long*)q; q += b_smp;
  void* d_tmp2 = q;
  if (int rc = line_starts(x, p->d_ls, st)) return rc;
  const unsigned gl = (unsigned)((n_lines + 1 + 255) / 256);
  text_fasta_flag_kernel<<<gl, 256, 0, st>>>(x.raw, x.nb, p->d_ls, n_lines, d_flag);
  MIC_TRY(hipcub::DeviceScan::ExclusiveSum(d_tmp2, tmp2, d_flag, d_rec, (int)(n_lines + 1), st));
  MIC_TRY(hipMemcpyAsync(&sc.n_rec32, d_rec + n_lines, 4, hipMemcpyDeviceToHost, st));
  text_fasta_sample_kernel<<<gl, 256, 0, st>>>(p->d_ls, d_flag, d_rec, n_lines, p->stride, d_samples);
  MIC_TRY(hipGetLastError());
  MIC_TRY(hipStreamSynchronize(st));
  if ((p->n_rec = sc.n_rec32) == 0) { *status = PS_HEADER; return MIC_OK; }
  p->samples.assign(p->n_rec / p->stride + 2, (unsigned long long)x.nb);
  const uint64_t have = (p->n_rec + p->stride - 1) / p->stride;          // samples the kernel wrote: records 0, stride, ...
  MIC_TRY(hipMemcpy(p->samples.data(), d_samples, have * 8, hipMemcpyDeviceToHost));
  return MIC_OK;
}

// partial: the text is the front of a longer one (a stripe of a member still being inflated, mic_gz_stream_next) - FASTQ only, the
// whole records of it are indexed (lines that end in '\n', four to a record), *n_used = where the first record that is not whole
// starts; no whole record yet: n_rec stays 0 and run_index gives no handle (MIC_OK, *out = nullptr, *n_used = 0)
int index_text(mic_text* p, Scan& sc, const void* d_text, size_t n, bool partial, hipStream_t st, uint64_t* n_used, uint32_t* status) {
  Scan::Text& x = sc.x[0]; sc.n = 1;
  // the kernels read 16 aligned bytes a thread: the text counts from the 4-KiB boundary in front of it, `from` bytes are not its own
  x.from = (uint32_t)((uintptr_t)d_text & 4095u);
  if (n + x.from >= 0xFFFFFF00ull) { *status = PS_BIG; return MIC_OK; }
  p->t = x.raw = (const uint8_t*)d_text - x.from; p->nb = x.nb = (uint32_t)(n + x.from);
  if (int rc = count_lines(p, sc, st, nullptr)) return rc;
  if (partial) {
    if (x.first != '@') { *status = PS_HEADER; return MIC_OK; }
    x.n_lines = (uint64_t)x.nl / 4 * 4; x.last = '\n';       // whole records of whole lines; what follows is the next call's
    if (x.n_lines == 0) return MIC_OK;
  }
  if (x.first == '>') return index_fasta(p, sc, st, status);
  if (x.first != '@') { *status = PS_HEADER; return MIC_OK; }                 // (anything else: the host path)
  if (x.n_lines % 4 != 0 || x.n_lines == 0) { *status = PS_LINES; return MIC_OK; }
  const uint64_t n_rec = p->n_rec = x.n_lines / 4, n_samples = n_rec / p->stride + 2;
  const size_t b_ls = up256((x.n_lines + 2) * 4), b_smp = up256(n_samples * 8);
  MIC_TRY(hipMalloc(&p->d_block, b_ls + b_smp));
  p->d_ls = (uint32_t*)p->d_block;
  unsigned long long* d_samples = (unsigned long long*)((char*)p->d_block + b_ls);
  if (int rc = line_starts(x, p->d_ls, st)) return rc;
  p->samples.resize(n_samples);
  text_sample_kernel<<<(unsigned)((n_samples + 255) / 256), 256, 0, st>>>(p->d_ls, x.nb, n_rec, p->stride, n_samples, d_samples);
  MIC_TRY(hipGetLastError());
  MIC_TRY(hipMemcpyAsync(p->samples.data(), d_samples, n_samples * 8, hipMemcpyDeviceToHost, st));
  MIC_TRY(hipStreamSynchronize(st));
  *n_used = p->samples.back() - x.from;
  return MIC_OK;
}

int text_index(mic_engine* e, const void* d_text, size_t n, bool partial, mic_text** out, uint64_t* n_records, uint64_t* n_used, uint32_t* status) {
  if (!e || !d_text || !out || !n_records || !status) return mic_set_error(MIC_E_INVALID, "null argument");
  *out = nullptr; *n_records = 0; *status = 0; *n_used = 0;
  if (n == 0 || n >= 0xFFFFFF00ull) { *status = PS_BIG; return MIC_OK; }      // 32-bit line starts
  return run_index(e, out, n_records, status, [&](mic_text* p, Scan& sc, hipStream_t st) { return index_text(p, sc, d_text, n, partial, st, n_used, status); });
}

}  // namespace

extern "C" {
// ---- paired-end texts on the device -----------------------------------------------------------------------------------------------
int mic_pairs_free(mic_engine* e, mic_pairs* p) { (void)e; delete p; return MIC_OK; }
// The texts keep from = 0: they come 16-byte aligned from the inflater (mic_gz.hip), which the line kernels' 16-byte loads need.
int mic_pairs_index_device(mic_engine* e, const void* d_text1, size_t n1, const void* d_text2, size_t n2, mic_pairs** out,
                           uint64_t* n_records, uint32_t* status) {
  if (!e || !d_text1 || !d_text2 || !out || !n_records || !status) return mic_set_error(MIC_E_INVALID, "null argument");
  *out = nullptr; *n_records = 0; *status = 0;
  if (n1 == 0 || n2 == 0 || n1 >= 0xFFFFFF00ull || n2 >= 0xFFFFFF00ull) { *status = PS_BIG; return MIC_OK; }   // 32-bit line starts
  return run_index(e, out, n_records, status, [&](mic_pairs* p, Scan& sc, hipStream_t st) {
    sc.x[0].raw = (const uint8_t*)d_text1; sc.x[0].nb = (uint32_t)n1;
    sc.x[1].raw = (const uint8_t*)d_text2; sc.x[1].nb = (uint32_t)n2; sc.n = 2;
    return index_pairs(p, sc, st, status);
  });
}

int mic_pairs_offsets(const mic_pairs* p, const uint64_t** samples, size_t* n_samples, uint32_t* stride) { return index_offsets(p, samples, n_samples, stride); }
int mic_pairs_merge_to_slot(mic_engine* e, mic_pairs* p, uint64_t r0, uint64_t r1, size_t slot_id, size_t* n_bytes) {
  if (!e || !p || !n_bytes) return mic_set_error(MIC_E_INVALID, "null argument");
  MicSlotText s; unsigned long long o0, o1;
  int rc = mic_ingest_slot_text(e, slot_id, &s);
  if (rc || (rc = p->range(r0, r1, o0, o1))) return rc;
  if (o1 - o0 > s.max_bytes) return mic_set_error(MIC_E_INVALID, "merged text of %llu bytes does not fit the slot (%zu)", o1 - o0, s.max_bytes);
  // the kernel runs on the SLOT's device and stream; when the texts live on another device (several engines, one inflated input)
  // it reads them through peer access
  if (s.device != p->device && !mic_peer_enable(s.device, p->device))
    return mic_set_error(MIC_E_UNSUPPORTED, "device %d has no peer access to device %d, where the inflated text lives", s.device, p->device);
  MIC_TRY(hipSetDevice(s.device));
  launch_pair_merge(p->t[0], p->t[1], r0, r1, p->d_off, s.d_raw, *mic_engine_min_quality(e), s.stream);
  MIC_TRY(hipGetLastError());
  *n_bytes = (size_t)(o1 - o0);
  return MIC_OK;
}

int mic_pairs_text(mic_engine* e, mic_pairs* p, uint64_t r0, uint64_t r1, void* host_dst, size_t cap, size_t* n_bytes) {
  if (!e || !p || !host_dst || !n_bytes) return mic_set_error(MIC_E_INVALID, "null argument");
  unsigned long long o0, o1;
  const int rc = p->range(r0, r1, o0, o1);
  if (rc) return rc;
  *n_bytes = (size_t)(o1 - o0);
  if (*n_bytes > cap) return mic_set_error(MIC_E_INVALID, "merged text of %zu bytes does not fit the buffer (%zu)", *n_bytes, cap);
  MIC_TRY(hipSetDevice(p->device));
  uint8_t* d = nullptr;
  MIC_TRY(hipMalloc(&d, *n_bytes + 16));
  launch_pair_merge(p->t[0], p->t[1], r0, r1, p->d_off, d, *mic_engine_min_quality(e), 0);
  hipError_t he = hipGetLastError();
  if (he == hipSuccess) he = hipMemcpy(host_dst, d, *n_bytes, hipMemcpyDeviceToHost);
  hipFree(d);
  MIC_TRY(he);
  return MIC_OK;
}

// ---- one FASTQ / FASTA text on the device (the inflated file of -O reads.fq.gz): where its records start -----------------------------
int mic_text_free(mic_engine* e, mic_text* p) { (void)e; delete p; return MIC_OK; }
int mic_text_index_device(mic_engine* e, const void* d_text, size_t n, mic_text** out, uint64_t* n_records, uint32_t* status) {
  uint64_t used = 0; return text_index(e, d_text, n, false, out, n_records, &used, status);
}
int mic_text_index_front_device(mic_engine* e, const void* d_text, size_t n, mic_text** out, uint64_t* n_records, uint64_t* n_used, uint32_t* status) {
  if (!n_used) return mic_set_error(MIC_E_INVALID, "null argument");
  return text_index(e, d_text, n, true, out, n_records, n_used, status);
}

int mic_text_format(const mic_text* p) { return p ? (p->fasta ? '>' : '@') : 0; }
int mic_text_offsets(const mic_text* p, const uint64_t** samples, size_t* n_samples, uint32_t* stride) { return index_offsets(p, samples, n_samples, stride); }
int mic_text_to_slot(mic_engine* e, mic_text* p, uint64_t r0, uint64_t r1, size_t slot_id, size_t* n_bytes) {
  if (!e || !p || !n_bytes) return mic_set_error(MIC_E_INVALID, "null argument");
  MicSlotText s; unsigned long long o0, o1;
  int rc = mic_ingest_slot_text(e, slot_id, &s);
  if (rc || (rc = p->range(r0, r1, o0, o1))) return rc;
  if (o1 - o0 > s.max_bytes) return mic_set_error(MIC_E_INVALID, "text of %llu bytes does not fit the slot (%zu)", o1 - o0, s.max_bytes);
  MIC_TRY(hipSetDevice(s.device));
  if (s.device != p->device) {
    mic_peer_enable(s.device, p->device);      // (without peer access the runtime stages the copy through host memory)
    MIC_TRY(hipMemcpyPeerAsync(s.d_raw, s.device, p->t + o0, p->device, (size_t)(o1 - o0), s.stream));
  } else MIC_TRY(hipMemcpyAsync(s.d_raw, p->t + o0, (size_t)(o1 - o0), hipMemcpyDeviceToDevice, s.stream));
  *n_bytes = (size_t)(o1 - o0);
  return MIC_OK;
}

int mic_text_copy(mic_engine* e, mic_text* p, uint64_t r0, uint64_t r1, void* host_dst, size_t cap, size_t* n_bytes) {
  if (!e || !p || !host_dst || !n_bytes) return mic_set_error(MIC_E_INVALID, "null argument");
  unsigned long long o0, o1;
  const int rc = p->range(r0, r1, o0, o1);
  if (rc) return rc;
  *n_bytes = (size_t)(o1 - o0);
  if (*n_bytes > cap) return mic_set_error(MIC_E_INVALID, "text of %zu bytes does not fit the buffer (%zu)", *n_bytes, cap);
  MIC_TRY(hipSetDevice(p->device));
  MIC_TRY(hipMemcpy(host_dst, p->t + o0, *n_bytes, hipMemcpyDeviceToHost));
  return MIC_OK;
}

}  // extern "C"

