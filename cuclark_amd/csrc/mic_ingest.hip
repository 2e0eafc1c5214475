// mic_ingest.hip — device-side ingest: raw FASTA / FASTQ bytes in, result-CSV text out (include/mi_clark.h, mic_ingest_*).
//
// Moves onto the GPU what the reference does on the host around queryBatch, for well-formed input:
//   read indexing            CuCLARK_hh.hh:1339-1534   -> line_count / line_start (mic_text.hip) / record kernels
//   2-bit packing, N-split   CuCLARK_hh.hh:1616-1716   -> pack_kernel  (same container format, same part rules)
//   result CSV lines         CuCLARK_hh.hh:1951-2139   -> csv_len / csv_fmt kernels ("%g" exact, mic_fmt.h)
// The host only moves bytes: file -> pinned buffer -> (H2D) ... (D2H) -> pinned buffer -> file.
//
// A batch is a run of whole records.  Anything the kernels do not reproduce exactly is DETECTED and reported as
// MIC_INGEST_FALLBACK so that the caller sends that batch through the host indexer / packer instead (mic_index_reads,
// mic_pack_reads, mic_csv_line): an empty read name (the reference's name scan then crosses the line end), a FASTA
// record without a sequence line, a truncated FASTQ record, a sequence longer than MIC_MAX_PART bytes, more lines or
// reads than the slot was sized for, a read that needs the dense fallback of the query kernel.
// This file is the ingest SLOTS.  The line indexer, and the index of whole texts resident on the device (mic_text_*, mic_pairs_*: the
// inflated input of -O x.fq.gz / -P a.fq.gz b.fq.gz), are mic_text.hip, which reaches a slot through mic_ingest_slot_text.
#include "mi_clark.h"
#include "mic_internal.h"
#include "mic_fmt.h"
#include "mic_qmask.h"
#include "mic_lowc.h"
#include "mic_hitmap.h"
#include "mic_kraken.h"

#include <hipcub/hipcub.hpp>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {

enum { H_NLINES = 0, H_NREADS = 1, H_STATUS = 2, H_CSV_BYTES = 3, H_FLAGGED = 4, H_NEWLINES = 5, H_CONT = 6, H_WORDS = 8 };

// one thread: number of lines (an unterminated last line counts and gets a virtual line end at nb), FASTQ record count
__global__ void lines_finish_kernel(const uint8_t* __restrict__ raw, uint32_t nb, const uint32_t* __restrict__ tile_off, uint32_t n_tiles,
                                    uint32_t* __restrict__ line_start, uint32_t cap, int fasta, uint32_t lpr, uint32_t max_reads,
                                    uint32_t* __restrict__ hdr) {
  const uint32_t nl = tile_off[n_tiles];
  uint32_t n_lines = nl;
  if (nb && raw[nb - 1] != '\n') { ++n_lines; if (n_lines < cap) line_start[n_lines] = nb + 1; }
  uint32_t status = 0;
  if (n_lines + 1 >= cap) status |= MIC_INGEST_TOO_MANY;
  hdr[H_NEWLINES] = nl;
  hdr[H_NLINES] = n_lines;
  if (!fasta) {
    if (n_lines % lpr) status |= MIC_INGEST_TRUNCATED;
    const uint32_t nr = n_lines / lpr;
    if (nr > max_reads) status |= MIC_INGEST_TOO_MANY;
    hdr[H_NREADS] = nr;
  }
  if (status) atomicOr(&hdr[H_STATUS], status);
}

// FASTA: flag[L] = line L starts a record ('>' in its first column, CuCLARK_hh.hh:1369-1389)
__global__ void __launch_bounds__(256) fasta_flag_kernel(const uint8_t* __restrict__ raw, uint32_t nb, const uint32_t* __restrict__ line_start,
                                                         const uint32_t* __restrict__ hdr, uint32_t cap, uint32_t n_scan,
                                                         uint32_t* __restrict__ flag) {
  const uint32_t L = blockIdx.x * 256 + threadIdx.x;
  if (L >= n_scan) return;
  const uint32_t n_lines = hdr[H_NLINES];
  uint32_t f = 0;
  if (L < n_lines && n_lines + 1 < cap) { const uint32_t p = line_start[L]; f = p < nb && raw[p] == '>'; }
  flag[L] = f;
}

__global__ void __launch_bounds__(256) fasta_scatter_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rec_of_line,
                                                            uint32_t cap, uint32_t max_reads, uint32_t* __restrict__ hdr_line, uint32_t* __restrict__ hdr) {
  const uint32_t L = blockIdx.x * 256 + threadIdx.x;
  const uint32_t n_lines = hdr[H_NLINES];
  if (n_lines + 1 >= cap) return;
  if (L < n_lines && flag[L]) { const uint32_t r = rec_of_line[L]; if (r < max_reads) hdr_line[r] = L; }
  if (L == n_lines) {                             // rec_of_line[n_lines] = number of records (flags past n_lines are 0)
    const uint32_t nr = rec_of_line[L];
    if (nr > max_reads) atomicOr(&hdr[H_STATUS], (uint32_t)MIC_INGEST_TOO_MANY);
    else hdr_line[nr] = n_lines;
    hdr[H_NREADS] = nr;
  }
}

struct RecArrays {
  uint32_t* name_s; uint32_t* seq_s; uint32_t* seq_e; uint32_t* length; uint32_t* bound;   // bound: containers reserved (scan input)
  uint8_t* name_len;                                                                       // min(name length, 40)
};

__device__ __forceinline__ bool name_sep_dev(uint8_t c) { return c == ' ' || c == '\t' || c == '\n'; }   // CuCLARK_hh.hh:300

// One thread per record: where its name and sequence are, its Length column, how many containers to reserve.
// FASTQ: record r = lines 4r .. 4r+3 (CuCLARK_hh.hh:1496-1523); FASTA: header line hdr_line[r], sequence lines up to the
// next header (CuCLARK_hh.hh:1369-1389), Length = bytes of the sequence lines without their line ends.
template <bool FASTA>
__global__ void __launch_bounds__(256) record_kernel(const uint8_t* __restrict__ raw, uint32_t nb, const uint32_t* __restrict__ line_start,
                                                     const uint32_t* __restrict__ hdr_line, uint32_t n_reads, uint32_t lpr, int k, RecArrays a,
                                                     uint32_t* __restrict__ hdr) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r > n_reads) return;
  if (r == n_reads) { a.bound[r] = 0; return; }
  uint32_t hl, hn;
  if (FASTA) { hl = hdr_line[r]; hn = hdr_line[r + 1]; } else { hl = lpr * r; hn = lpr * r + 2; }
  const uint32_t hs = line_start[hl], ss = line_start[hl + 1], se = line_start[hn] - 1;
  uint32_t status = 0, len;
  if (FASTA) {
    const uint32_t c = hn - hl - 1;               // sequence lines
    if (c == 0) status |= MIC_INGEST_ODD_RECORD;  // the reference counts a phantom byte for such a record: host path
    len = (se + 1 - ss) - c;
  } else {
    len = se - ss;
  }
  // name: from the byte after the marker to the first separator strictly after it (CuCLARK_hh.hh:1369-1372)
  const uint32_t ns = hs + 1;
  if (ns + 1 >= ss) status |= MIC_INGEST_ODD_RECORD;   // header line holds the marker only: the reference's scan leaves the line
  uint32_t j = ns + 1;
  while (j < ss && j - ns < 40 && !name_sep_dev(raw[j])) ++j;
  const uint32_t nbytes = se >= ss ? se - ss : 0;
  if (nbytes > MIC_MAX_PART) status |= MIC_INGEST_LONG_READ;
  a.name_s[r] = ns; a.name_len[r] = (uint8_t)(j - ns);
  a.seq_s[r] = ss; a.seq_e[r] = ss + nbytes; a.length[r] = len;
  // containers reserved for the read: every part of L >= k nt takes 1 + ceil(L/8) <= 2 + L/8, parts are separated by at
  // least one byte; + slack for a trailing run that is dropped after its first containers were written, + the terminator
  // (a base masked by its quality or by the low-complexity mask is still one byte between two parts: the bound holds as it stands)
  a.bound[r] = (len < (uint32_t)k || status) ? 0u : nbytes / 8 + 2 * (nbytes / (uint32_t)(k + 1) + 1) + 8;
  if (status) atomicOr(&hdr[H_STATUS], status);
  (void)nb;
}

// ---- the packer (CuCLARK_hh.hh:1616-1716): one wavefront per read ---------------------------------------------------
// A part is a maximal run of ACGTU (either case); '\n' is transparent, any other byte ends the run; runs shorter than k
// are dropped.  Stored per part: one length slot + ceil(len/8) containers, 8 nt per u16, first nt in the top bits,
// A=3 C=2 G=1 T/U=0, the last container left-aligned.  Reads are laid out at the reserved offsets rp[r] and end with a 0
// length slot when they do not fill their reservation (the query kernel stops there, include/mi_clark.h).
// QUAL (four-line FASTQ with a threshold set, mic_ingest_set_min_quality): the lane that loads raw[p] also loads the quality byte at
// the same offset of the record's quality line and takes a masked base (mic_qmask.h) for an "other byte" - what an 'N' is.  The
// quality line comes from the slot's LINE INDEX, passed in (no new per-record arrays): line 4r + 3, which ends at
// line_start[4r + 4] - 1 - the virtual line end of an unterminated last line included (lines_finish_kernel).  Both loads are byte
// loads at consecutive addresses across the wavefront.  <false> is the kernel as it was; every launch without a threshold takes it.
// LOWC (a low-complexity level set, mic_ingest_set_low_complexity): the same lane also takes bit p of the slot's bitmap, which
// lowc_kernel wrote in front of this kernel (mic_lowc.h), and a set bit is an "other byte" too.  The text itself is never rewritten.
template <bool QUAL, bool LOWC>
__global__ void __launch_bounds__(256) pack_kernel(const uint8_t* __restrict__ raw, const uint32_t* __restrict__ seq_s,
                                                   const uint32_t* __restrict__ seq_e, const uint32_t* __restrict__ rp,
                                                   uint16_t* __restrict__ cont, uint32_t n_reads, int k,
                                                   const uint32_t* __restrict__ line_start, uint32_t c0,
                                                   const uint32_t* __restrict__ lowc) {
  __shared__ uint8_t s_codes[4][80];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint8_t* codes = s_codes[wv];
  const uint32_t n_waves = gridDim.x * 4;
  for (uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv); r < n_reads; r += n_waves) {
    const uint32_t o0 = rp[r], o1 = rp[r + 1];
    if (o1 == o0) continue;                       // shorter than k: nothing stored (CuCLARK_hh.hh:1633)
    uint16_t* out = cont + o0;
    const uint32_t s = seq_s[r], e = seq_e[r];
    uint32_t qs = 0, qn = 0;                      // QUAL: where the record's quality line starts, its bytes
    if (QUAL) { qs = line_start[4 * r + 3]; qn = line_start[4 * r + 4] - 1u - qs; }
    uint32_t hdr = 0, run = 0;                    // header slot of the open part (relative), its nucleotides so far
    auto close_run = [&]() {
      if (run >= (uint32_t)k) {
        const uint32_t rem = run & 7u;
        if (rem && lane == 0) {
          uint32_t v = 0;
          for (uint32_t i = 0; i < rem; ++i) v = (v << 2) | codes[i];
          out[hdr + 1 + run / 8] = (uint16_t)(v << (2 * (8 - rem)));
        }
        if (lane == 0) out[hdr] = (uint16_t)run;
        hdr += 1 + (run + 7) / 8;
      }
      run = 0;
    };
    for (uint32_t base = s; base < e; base += 64) {
      const uint32_t p = base + lane;
      uint32_t cls = 3, code = 0;                 // 0 nucleotide, 1 line end, 2 other byte, 3 past the end
      if (p < e) {
        const uint32_t b = raw[p], u = b & 0xDFu;
        if (u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'U') { cls = 0; code = (0x4Bu >> (2 * ((u >> 1) & 3u))) & 3u; }
        else cls = b == '\n' ? 1 : 2;
        if (QUAL && mic_qmask_masked(raw + qs, qn, p - s, c0)) cls = 2;
        if (LOWC && ((lowc[p >> 5] >> (p & 31u)) & 1u)) cls = 2;
      }
      const uint64_t m_nt = __ballot(cls == 0), m_ot = __ballot(cls == 2);
      int lo = 0;
      for (;;) {
        const uint64_t from = lo >= 64 ? 0ull : ~0ull << lo;
        const uint64_t mo = m_ot & from;
        const int hi = mo ? __builtin_ctzll(mo) : 64;
        const uint64_t upto = hi >= 64 ? ~0ull : ((1ull << hi) - 1);
        const uint64_t seg = m_nt & from & upto;
        const uint32_t n = __popcll(seg);
        if (n) {
          const uint32_t off = run & 7u;
          __builtin_amdgcn_wave_barrier();
          if ((seg >> lane) & 1) codes[off + __popcll(seg & ((1ull << lane) - 1))] = (uint8_t)code;
          __builtin_amdgcn_wave_barrier();
          const uint32_t total = off + n, nfull = total >> 3, rem = total & 7u;
          uint32_t keep = 0;
          if ((uint32_t)lane < nfull) {
            const uint8_t* c = codes + 8 * lane;
            const uint32_t v = (c[0] << 14) | (c[1] << 12) | (c[2] << 10) | (c[3] << 8) | (c[4] << 6) | (c[5] << 4) | (c[6] << 2) | c[7];
            out[hdr + 1 + (run - off) / 8 + lane] = (uint16_t)v;
          }
          if ((uint32_t)lane < rem) keep = codes[8 * nfull + lane];
          __builtin_amdgcn_wave_barrier();
          if ((uint32_t)lane < rem) codes[lane] = (uint8_t)keep;
          __builtin_amdgcn_wave_barrier();
          run += n;
        }
        if (hi >= 64) break;
        close_run();
        lo = hi + 1;
      }
    }
    close_run();
    if (lane == 0 && hdr < o1 - o0) out[hdr] = 0;
  }
}

// ---- the low-complexity mask (mic_lowc.h): one wavefront per read, between record_kernel and pack_kernel -----------------
// Writes bit p of `bits` (zeroed in front of the launch) for every masked base at text offset p; the text is not touched.
// The read's bytes are taken 64 at a time as the packer takes them.  '\n' is dropped by ballot / popcount, what is left (a nucleotide's
// 2-bit code, or 4 for a byte that ends the run) goes into a ring of 256 LOGICAL positions per wavefront with the text offset beside it.
// Whenever 80 undecided positions are in the ring (64 + the 16 a window looks ahead; at the read's end: what is left), 64 of them are
// decided, one per lane: six ballots turn the 96 ring entries around them into three 128-bit masks (run end, low and high code bit),
// every lane shifts its own 32-bit window out of them - the nearest run ends on either side clip it - and counts equal triplets at
// every distance 1..29 with shifts, ANDs and popcounts of those three words (mic_lowc_T_planes): no histogram, no LDS traffic and no
// cross-lane step inside the count; about 12 vector instructions per distance.  Ring: an entry is read until it is 16 behind the
// decided front and written up to 143 ahead of it, 160 < 256 apart.  QUAL: a base masked by its quality ends the run (the rule is
// applied to the quality-masked text).  Reads of which nothing is packed (rp[r] == rp[r + 1]: shorter than k, or a batch that goes
// back to the host) are skipped.
template <bool QUAL>
__global__ void __launch_bounds__(256) lowc_kernel(const uint8_t* __restrict__ raw, const uint32_t* __restrict__ seq_s,
                                                   const uint32_t* __restrict__ seq_e, const uint32_t* __restrict__ rp, uint32_t n_reads,
                                                   uint32_t level, const uint32_t* __restrict__ line_start, uint32_t c0,
                                                   uint32_t* __restrict__ bits) {
  __shared__ uint8_t s_code[4][256];
  __shared__ uint32_t s_pos[4][256];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint8_t* ring_c = s_code[wv];
  uint32_t* ring_p = s_pos[wv];
  const uint32_t n_waves = gridDim.x * 4;
  for (uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv); r < n_reads; r += n_waves) {
    if (rp[r + 1] == rp[r]) continue;
    const uint32_t s = seq_s[r], e = seq_e[r];
    uint32_t qs = 0, qn = 0;
    if (QUAL) { qs = line_start[4 * r + 3]; qn = line_start[4 * r + 4] - 1u - qs; }
    uint32_t produced = 0, consumed = 0;          // logical positions in the ring so far; decided so far (both wave-uniform)
    auto decide = [&]() {                         // logical positions [consumed, consumed + 64), lane by lane
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      // ring entries consumed - 16 + i, i in [0, 96): lane i holds entry i, lanes 0..31 entry 64 + i as well; what lies in front of
      // the read or behind what was produced (only at the read's end) ends a run
      const uint32_t qa = consumed - 16u + (uint32_t)lane, qb = qa + 64u;      // (qa wraps below 0: not < produced)
      uint32_t ca = 4, cb = 4;
      if (qa < produced) ca = ring_c[qa & 255u];
      if (lane < 32 && qb < produced) cb = ring_c[qb & 255u];
      const uint64_t e_lo = __ballot(ca > 3u), e_hi = __ballot(cb > 3u);
      const uint64_t a_lo = __ballot((ca & 1u) != 0), a_hi = __ballot((cb & 1u) != 0);
      const uint64_t b_lo = __ballot((ca & 2u) != 0), b_hi = __ballot((cb & 2u) != 0);
      auto window = [&](uint64_t lo, uint64_t hi) { return lane ? (uint32_t)((lo >> lane) | (hi << (64 - lane))) : (uint32_t)lo; };
      const uint32_t we = window(e_lo, e_hi), w0 = window(a_lo, a_hi), w1 = window(b_lo, b_hi);   // bit i: position q - 16 + i
      const uint32_t q = consumed + (uint32_t)lane;
      if (q < produced && !((we >> 16) & 1u)) {
        const uint32_t below = we & 0xFFFFu, above = we >> 17;
        const uint32_t lo = below ? 32u - (uint32_t)__clz((int)below) : 0u;
        const uint32_t hi = above ? 16u + (uint32_t)__ffs((int)above) : 32u;
        if (hi - lo >= 4u) {
          const uint32_t l = hi - lo - 2u;
          if (mic_lowc_over(mic_lowc_T_planes(w0, w1, lo, l), l, level)) {
            const uint32_t p = ring_p[q & 255u];
            atomicOr(&bits[p >> 5], 1u << (p & 31u));
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      consumed += 64u;
    };
    for (uint32_t base = s; base < e; base += 64) {
      const uint32_t p = base + lane;
      uint32_t code = 5;                          // 0..3 nucleotide, 4 ends the run, 5 line end or past the end: no logical position
      if (p < e) {
        const uint32_t b = raw[p];
        if (b != '\n') {
          code = mic_lowc_code(b);
          if (QUAL && mic_qmask_masked(raw + qs, qn, p - s, c0)) code = 4;
        }
      }
      const uint64_t m = __ballot(code < 5u);
      if (code < 5u) {
        const uint32_t idx = (produced + (uint32_t)__popcll(m & ((1ull << lane) - 1))) & 255u;
        ring_c[idx] = (uint8_t)code; ring_p[idx] = p;
      }
      produced += (uint32_t)__popcll(m);
      while (produced - consumed >= 80u) decide();
    }
    while (consumed < produced) decide();
  }
}

// ---- CSV (CuCLARK_hh.hh:1951-2139, non-extended): "name,len,gamma,1st,score1,2nd,score2,confidence\n" ----------------
struct CsvArgs {
  const uint8_t* raw; const uint32_t* name_s; const uint8_t* name_len; const uint32_t* length; const uint32_t* results;
  const char* tnames; const uint32_t* tname_off;   // target names back to back; name t = [off[t], off[t+1])
  uint32_t n_targets, n_reads; int k, paired;
};

__device__ __forceinline__ uint32_t digits_u32(uint32_t v) {
  return v < 10 ? 1 : v < 100 ? 2 : v < 1000 ? 3 : v < 10000 ? 4 : v < 100000 ? 5 : v < 1000000 ? 6 : v < 10000000 ? 7 : v < 100000000 ? 8 : v < 1000000000 ? 9 : 10;
}

__device__ __forceinline__ uint32_t tname_len(const CsvArgs& a, uint32_t idx1) {     // idx1 = target + 1, 0 or out of range = "NA"
  return (idx1 == 0 || idx1 > a.n_targets) ? 2u : a.tname_off[idx1] - a.tname_off[idx1 - 1];
}

__global__ void __launch_bounds__(256) csv_len_kernel(CsvArgs a, uint32_t* __restrict__ line_len, uint32_t* __restrict__ hdr) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r > a.n_reads) return;
  if (r == a.n_reads) { line_len[r] = 0; return; }
  const uint32_t* res = a.results + (size_t)r * 8;
  const uint4 lo = *(const uint4*)res;
  const uint32_t total = lo.x, ib = lo.y, best = lo.z, is = lo.w, sbest = res[4];
  const uint32_t len = a.length[r], norm = a.paired ? len - 1u : len;
  uint32_t nl = a.name_len[r]; if (nl >= 40) nl = 39;                 // OBJECTNAMEMAX (CuCLARK_hh.hh:2114-2117)
  char tmp[16];
  const int g = mic_fmt_gamma(total, norm, a.k, tmp);
  const int c = mic_fmt_conf(best, sbest, tmp);
  if (g < 0) atomicOr(&hdr[H_STATUS], (uint32_t)MIC_INGEST_ODD_RECORD);
  uint32_t ll = nl + 1 + digits_u32(norm) + 1 + (uint32_t)(g < 0 ? 1 : g) + 1 + tname_len(a, ib) + 1 + digits_u32(best) + 1 + tname_len(a, is) + 1 +
                digits_u32(sbest) + 1 + (uint32_t)c + 1;
  // a line this long (target names of hundreds of characters) goes through the host path: with every line below the bound the
  // 32-bit sum of a slot's line lengths cannot wrap (mic_ingest_alloc limits the slot size accordingly)
  if (ll > 768u) { atomicOr(&hdr[H_STATUS], (uint32_t)MIC_INGEST_TOO_MANY); ll = 0; }
  line_len[r] = ll;
}

#define CSV_LDS 24576
__global__ void __launch_bounds__(256) csv_fmt_kernel(CsvArgs a, const uint32_t* __restrict__ line_off, char* __restrict__ out) {
  __shared__ char s_buf[CSV_LDS];
  const uint32_t r0 = blockIdx.x * 256, r = r0 + threadIdx.x;
  const uint32_t r1 = r0 + 256 < a.n_reads ? r0 + 256 : a.n_reads;
  const uint32_t b0 = line_off[r0], b1 = line_off[r1];
  const bool staged = b1 - b0 <= CSV_LDS;
  if (r < a.n_reads) {
    const uint32_t* res = a.results + (size_t)r * 8;
    const uint4 lo = *(const uint4*)res;
    const uint32_t total = lo.x, ib = lo.y, best = lo.z, is = lo.w, sbest = res[4];
    const uint32_t len = a.length[r], norm = a.paired ? len - 1u : len;
    uint32_t nl = a.name_len[r]; if (nl >= 40) nl = 39;
    char* p = staged ? s_buf + (line_off[r] - b0) : out + line_off[r];
    const uint8_t* nm = a.raw + a.name_s[r];
    for (uint32_t i = 0; i < nl; ++i) *p++ = (char)nm[i];
    char tmp[16];
    *p++ = ','; { const int n = mic_fmt_u32(norm, tmp); for (int i = 0; i < n; ++i) *p++ = tmp[i]; }
    *p++ = ','; { int n = mic_fmt_gamma(total, norm, a.k, tmp); if (n < 0) { tmp[0] = '?'; n = 1; } for (int i = 0; i < n; ++i) *p++ = tmp[i]; }
    for (int f = 0; f < 2; ++f) {
      const uint32_t idx1 = f ? is : ib, sc = f ? sbest : best;
      *p++ = ',';
      if (idx1 == 0 || idx1 > a.n_targets) { *p++ = 'N'; *p++ = 'A'; }
      else { const char* t = a.tnames + a.tname_off[idx1 - 1]; const uint32_t tl = a.tname_off[idx1] - a.tname_off[idx1 - 1]; for (uint32_t i = 0; i < tl; ++i) *p++ = t[i]; }
      *p++ = ','; { const int n = mic_fmt_u32(sc, tmp); for (int i = 0; i < n; ++i) *p++ = tmp[i]; }
    }
    *p++ = ','; { const int n = mic_fmt_conf(best, sbest, tmp); for (int i = 0; i < n; ++i) *p++ = tmp[i]; }
    *p++ = '\n';
  }
  if (staged) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < b1 - b0; i += 256) out[b0 + i] = s_buf[i];
  }
}

// (the caps are checked here as well as on the host: the counting kernel behind this one reads the status word on the device)
__global__ void csv_finish_kernel(const uint32_t* __restrict__ line_off, uint32_t n_reads, const uint32_t* __restrict__ flagged,
                                  const uint32_t* __restrict__ rp, uint32_t csv_cap, uint32_t cont_cap, uint32_t* __restrict__ hdr) {
  hdr[H_CSV_BYTES] = line_off[n_reads];
  hdr[H_FLAGGED] = flagged[0];
  hdr[H_CONT] = rp[n_reads];
  if (flagged[0]) atomicOr(&hdr[H_STATUS], (uint32_t)MIC_INGEST_DENSE);
  if (line_off[n_reads] > csv_cap || rp[n_reads] > cont_cap) atomicOr(&hdr[H_STATUS], (uint32_t)MIC_INGEST_TOO_MANY);
}

// MIC_INGEST_NO_CSV: what csv_len_kernel + csv_finish_kernel report that does not come from the lengths of the CSV lines - a gamma the
// formatter does not cover (csv_len_kernel: mic_fmt_gamma < 0), a read that needs the dense path, more containers than the slot holds
__global__ void __launch_bounds__(256) nocsv_status_kernel(const uint32_t* __restrict__ results, const uint32_t* __restrict__ length, int paired, int k,
                                                           uint32_t n_reads, const uint32_t* __restrict__ flagged, const uint32_t* __restrict__ rp,
                                                           uint32_t cont_cap, uint32_t* __restrict__ hdr) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r < n_reads) {
    const uint32_t total = results[(size_t)r * 8], norm = paired ? length[r] - 1u : length[r];
    const double den = ((double)norm - (double)k) + 1.0;
    if (total != 0 && !(den >= (double)total)) atomicOr(&hdr[H_STATUS], (uint32_t)MIC_INGEST_ODD_RECORD);
  }
  if (r == 0) {
    hdr[H_CSV_BYTES] = 0;
    hdr[H_FLAGGED] = flagged[0];
    hdr[H_CONT] = rp[n_reads];
    if (flagged[0]) atomicOr(&hdr[H_STATUS], (uint32_t)MIC_INGEST_DENSE);
    if (rp[n_reads] > cont_cap) atomicOr(&hdr[H_STATUS], (uint32_t)MIC_INGEST_TOO_MANY);
  }
}

// ---- hit-map text (mic_hitmap.h: "<name>,<tokens joined by spaces>\n") - csv_len_kernel / csv_fmt_kernel's pattern: one thread per
// read computes its line's length from the name, the words and the target-name offsets, a 64-bit exclusive sum gives the lines'
// places, one thread per read writes its line.  No cap on a line's length and no hand-back: a long read's line is as long as its map.
struct HitmapTextArgs {
  const uint8_t* raw; const uint32_t* name_s; const uint8_t* name_len;
  const uint32_t* offsets; const uint32_t* words;
  const char* tnames; const uint32_t* tname_off; uint32_t n_targets, n_reads;
};

__global__ void __launch_bounds__(256) hitmap_len_kernel(HitmapTextArgs a, unsigned long long* __restrict__ line_len) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r > a.n_reads) return;
  if (r == a.n_reads) { line_len[r] = 0; return; }
  uint32_t nl = a.name_len[r]; if (nl >= 40) nl = MIC_HITMAP_NAME_MAX;
  const uint32_t w0 = a.offsets[r], w1 = a.offsets[r + 1];
  unsigned long long ll = (unsigned long long)nl + 2u + (w1 > w0 ? w1 - w0 - 1u : 0u);      // name , tokens' spaces \n
  for (uint32_t i = w0; i < w1; ++i) {
    const uint32_t w = a.words[i], l = mic_hitmap_word_label(w);
    ll += w == MIC_HITMAP_SEP ? 1u : (l == 0 ? 1u : l > a.n_targets ? 2u : a.tname_off[l] - a.tname_off[l - 1]) + 1u + digits_u32(mic_hitmap_word_len(w));
  }
  line_len[r] = ll;
}

__global__ void __launch_bounds__(256) hitmap_fmt_kernel(HitmapTextArgs a, const unsigned long long* __restrict__ line_off, char* __restrict__ out) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.n_reads) return;
  uint32_t nl = a.name_len[r]; if (nl >= 40) nl = MIC_HITMAP_NAME_MAX;
  char* p = out + line_off[r];
  const uint8_t* nm = a.raw + a.name_s[r];
  for (uint32_t i = 0; i < nl; ++i) *p++ = (char)nm[i];
  *p++ = ',';
  char tmp[16];
  const uint32_t w0 = a.offsets[r], w1 = a.offsets[r + 1];
  for (uint32_t i = w0; i < w1; ++i) {
    const uint32_t w = a.words[i], l = mic_hitmap_word_label(w);
    if (i != w0) *p++ = ' ';
    if (w == MIC_HITMAP_SEP) { *p++ = '|'; continue; }
    if (l == 0) *p++ = '0';
    else if (l > a.n_targets) { *p++ = 'N'; *p++ = 'A'; }
    else { const char* t = a.tnames + a.tname_off[l - 1]; const uint32_t tl = a.tname_off[l] - a.tname_off[l - 1]; for (uint32_t j = 0; j < tl; ++j) *p++ = t[j]; }
    *p++ = ':';
    const int n = mic_fmt_u32(mic_hitmap_word_len(w), tmp);
    for (int j = 0; j < n; ++j) *p++ = tmp[j];
  }
  *p++ = '\n';
}

// ---- Kraken per-read text (mic_kraken.h: "<C|U>\t<name>\t<taxid>\t<length>\t<map>\n") - the hit-map text's place in the batch and its
// buffers, another line.  The length kernel is hitmap_len_kernel's shape: one thread per read, 64-bit lengths, the 64-bit exclusive sum.
// The format kernel is csv_fmt_kernel's shape, not hitmap_fmt_kernel's: a line of a 150-bp read is 60 to 90 bytes, so threads that
// store their bytes straight to global memory write 60 to 90 bytes apart.  A block's 256 lines are contiguous in the output
// (line_off[r0] .. line_off[r1]): they are formatted into an LDS stage and the stage is copied out with consecutive lanes on
// consecutive addresses - dwords over the aligned middle, bytes at the two ends; the stage is shifted by the output's misalignment, so
// that a dword of the stage is a dword of the output.  A block whose text does not fit the stage (long reads, many runs) stores
// directly.  Both kernels count and write through mic_kraken_line: they cannot disagree about a line's length.
struct KrakenTextArgs {
  HitmapTextArgs h;
  const uint32_t* results; const uint32_t* length; uint32_t norm_sub; int k;
  mic_abund_filter filter;
};

struct KrakenCount { unsigned long long n; __device__ __forceinline__ void operator()(char) { ++n; } };
template <typename P> struct KrakenStore { P p; __device__ __forceinline__ void operator()(char c) { *p++ = c; } };
struct KrakenTarget {
  const char* tnames; const uint32_t* tname_off;
  template <typename Put> __device__ __forceinline__ void operator()(uint32_t l, Put& put) const {
    const uint32_t a = tname_off[l - 1], b = tname_off[l];
    for (uint32_t i = a; i < b; ++i) put(tnames[i]);
  }
};
template <typename Put> __device__ __forceinline__ void kraken_line_of(const KrakenTextArgs& a, uint32_t r, Put& put) {
  const uint32_t w0 = a.h.offsets[r], w1 = a.h.offsets[r + 1];
  KrakenTarget tg{a.h.tnames, a.h.tname_off};
  mic_kraken_line(put, a.h.raw + a.h.name_s[r], a.h.name_len[r], a.results + (size_t)r * 8, a.length[r] - a.norm_sub, a.k, a.h.n_targets, a.filter,
                  a.h.words + w0, w1 - w0, tg);
}

__global__ void __launch_bounds__(256) kraken_len_kernel(KrakenTextArgs a, unsigned long long* __restrict__ line_len) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r > a.h.n_reads) return;
  if (r == a.h.n_reads) { line_len[r] = 0; return; }
  KrakenCount cnt{0};
  kraken_line_of(a, r, cnt);
  line_len[r] = cnt.n;
}

// 24 KiB, csv_fmt_kernel's size: 256 lines of up to 96 bytes, which holds the 60 to 90 bytes of a 150-bp read's line; six blocks
// (24 of a CU's 32 waves) fit the 160 KiB of LDS, and a larger stage would buy longer lines with resident waves
#define KRAKEN_LDS 24576
__global__ void __launch_bounds__(256) kraken_fmt_kernel(KrakenTextArgs a, const unsigned long long* __restrict__ line_off, char* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) char s_buf[KRAKEN_LDS];
  const uint32_t r0 = blockIdx.x * 256, r = r0 + threadIdx.x;
  const uint32_t r1 = r0 + 256 < a.h.n_reads ? r0 + 256 : a.h.n_reads;
  const unsigned long long b0 = line_off[r0], b1 = line_off[r1];
  const uint32_t sh = (uint32_t)((uintptr_t)(out + b0) & 3u);           // stage byte sh + i is output byte b0 + i
  const bool staged = b1 - b0 <= (unsigned long long)(KRAKEN_LDS - 3);
  if (r < a.h.n_reads) {
    if (staged) { KrakenStore<char*> put{s_buf + sh + (uint32_t)(line_off[r] - b0)}; kraken_line_of(a, r, put); }
    else { KrakenStore<char*> put{out + line_off[r]}; kraken_line_of(a, r, put); }
  }
  if (staged) {
    __syncthreads();
    const uint32_t end = sh + (uint32_t)(b1 - b0), t = threadIdx.x;
    char* g = out + b0 - sh;                                              // 4-byte aligned; bytes [sh, end) are this block's
    const uint32_t body = sh ? 4u : 0u, e4 = end & ~3u;
    if (sh && t >= sh && t < 4u && t < end) g[t] = s_buf[t];
    for (uint32_t i = body / 4u + t; i < e4 / 4u; i += 256) ((uint32_t*)g)[i] = ((const uint32_t*)s_buf)[i];
    if (e4 >= body && e4 + t < end) g[e4 + t] = s_buf[e4 + t];
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
// (the device code of this file is loaded when its first kernel is launched: mic_ingest_alloc does that, not the first batch)
__global__ void ingest_warm_kernel(uint32_t* p) { if (p && threadIdx.x == 1000) *p = 0; }

struct Slot {
  // pinned host
  uint8_t* h_raw = nullptr; char* h_csv = nullptr; uint32_t* h_hdr = nullptr; uint32_t* h_results = nullptr;
  // device
  uint8_t* d_raw = nullptr; uint32_t* d_tile = nullptr; uint32_t* d_tile_off = nullptr; uint32_t* d_line_start = nullptr;
  uint32_t* d_flag = nullptr; uint32_t* d_rec_of_line = nullptr; uint32_t* d_hdr_line = nullptr;
  RecArrays rec{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  uint32_t* d_rp = nullptr; uint16_t* d_cont = nullptr; uint32_t* d_results = nullptr; uint32_t* d_flagged = nullptr;
  uint32_t* d_crowd = nullptr;   // work area of the crowded runs' follow-up (mic_internal.h: mic_crowd_dims)
  uint32_t* d_lowc = nullptr;    // low-complexity bitmap, one bit per text byte (mic_lowc.h); allocated with the first batch that has a level set
  uint32_t* d_line_len = nullptr; uint32_t* d_line_off = nullptr; char* d_csv = nullptr; uint32_t* d_hdr = nullptr;
  void* d_tmp = nullptr; size_t tmp_bytes = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev = nullptr, ev_up = nullptr, ev_k = nullptr;
  uint32_t n_reads = 0, cont_used = 0;
  std::vector<void*> dev_allocs, host_allocs;
  // rank roll-up (mic_rollup_start on the slot's engine; allocated with the first such batch): the sparse rows of the batch, ru_row_words
  // u32 per read, their roll-up rows, and the pinned copy of those when the slots were allocated with want_results
  uint32_t* d_ru_rows = nullptr; uint32_t* d_rollup = nullptr; uint32_t* h_rollup = nullptr;
  uint32_t ru_row_words = 0; bool ru_valid = false;
  // read splitting (mic_split_start on the slot's engine; allocated with the first such batch): the partition buffer and its pinned twin,
  // max_bytes + 8 each, the work arrays of the three steps, and {a | b << 32, classified records} of the last batch in pinned memory
  uint8_t* d_split = nullptr; uint8_t* h_split = nullptr; uint64_t* h_split_tot = nullptr;
  MicSplitBufs split_b;
  int split_which = 0; bool split_valid = false;
  // hit maps (mic_hitmap_start on the slot's engine; allocated with the slots when started by then, else with the first such batch):
  // counts / offsets (u32) and line lengths / line offsets (u64) of max_reads + 2 items each with the two scans' storage in one allocation;
  // the word buffer, the text buffer and its pinned twin are allocations of their own that grow when a batch needs more and never shrink;
  // {words, text bytes} of the last batch in pinned memory
  uint32_t* d_hm_cnt = nullptr; uint32_t* d_hm_off = nullptr; unsigned long long* d_hm_len = nullptr; unsigned long long* d_hm_loff = nullptr;
  void* d_hm_tmp = nullptr; size_t hm_tmp_bytes = 0;
  uint32_t* d_hm_words = nullptr; size_t hm_words_cap = 0;
  char* d_hm_text = nullptr; char* h_hm_text = nullptr; size_t hm_text_cap = 0;
  uint64_t* h_hm_tot = nullptr;
  bool hm_valid = false, hm_kraken = false;      // hm_kraken: the text is the Kraken format's (mic_kraken_start)
  // table-sharded batches (mic_ingest_classify_group): what this slot keeps on every engine of its group, the owner included
  struct Peer {
    mic_engine* eng = nullptr; int device = 0;
    void* block = nullptr;
    uint32_t* d_rp = nullptr; uint16_t* d_cont = nullptr;   // the packed reads (helpers: a peer copy; owner: the slot's own arrays)
    uint32_t* d_rows = nullptr;                             // this engine's partial rows of ALL reads of the batch
    uint32_t* d_gather = nullptr; uint32_t* d_acc = nullptr; uint32_t* d_acc2 = nullptr;  // rows of this engine's read range from the others; the running sum's two buffers
    uint32_t* d_res = nullptr;                              // helpers: results of all reads from the query kernel, then of the range
    uint32_t* d_flagged = nullptr; uint32_t* d_crowd = nullptr;
    hipStream_t stream = nullptr;                           // helpers: a stream on their device; owner: the slot's stream
    hipEvent_t ev_q = nullptr, ev_done = nullptr;           // this engine's rows are written; its range is finished and delivered
    // MIC_GROUP_TIMING: packed reads asked for / arrived (= kernel start) / kernel done / all other engines' rows ready / range delivered
    hipEvent_t tv[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const void* table_id = nullptr;                         // the engine's table when the buffers were set up (a reloaded engine is another peer)
  };
  std::vector<Peer> peers;
  hipEvent_t ev_pack = nullptr;
  size_t group_owner = 0;
  uint64_t fan_bytes = 0, x_bytes = 0;                      // MIC_GROUP_TIMING: bytes of the last batch's fan-out and row exchange
  bool timed = false;
};

// MIC_GROUP_TIMING=1: what the table-sharded batches of an engine's slots cost, summed over its batches (mic_ingest_group_stats)
struct GroupStats {
  std::mutex mu;
  uint64_t batches = 0, reads = 0, fan_bytes = 0, x_bytes = 0;
  double fan_ms_sum = 0, fan_ms_max = 0, kernel_ms_sum = 0, kernel_ms_max = 0, x_ms_sum = 0, x_ms_max = 0, span_ms = 0;
};

struct Ingest {
  mic_engine* eng = nullptr; int device = 0;
  size_t max_bytes = 0, max_lines = 0, max_reads = 0, max_tiles = 0, cont_cap = 0, csv_cap = 0;
  // reads the work area of the crowded runs' follow-up is sized for (mic_internal.h: mic_crowd_dims), 0: none - the engine's table has no
  // side table (a slot holds max_bytes / 32 reads at most and ~max_bytes / 160 in practice: a quarter of the bound; what does not fit
  // takes the dense path).  Sized by the bound it was 100 MB per slot and per helper engine of a group - 13 GB of allocations in
  // front of the first batches of an 8-part run.
  size_t crowd_reads = 0;
  char* d_tnames = nullptr; uint32_t* d_tname_off = nullptr; uint32_t n_targets = 0;
  int want_results = 0;
  std::vector<Slot> slots;
  GroupStats gstats;
};

const uint32_t kFlaggedCapI = 1024;

// The wait of a slot's host thread for its stream (three times per batch) does not spin: the command line runs one such thread per
// slot next to its loaders, and a job that is allowed 16 CPUs (cgroup quota) has none to burn in busy-waits - with
// hipEventSynchronize's spinning one and the same box gave 108-195 Mreads/s from run to run, with this 189-194.
// Polling with short sleeps, not hipEventBlockingSync: the interrupt-driven wait stalled once for minutes under rocprofv3 --pmc.
// MIC_INGEST_SPIN=1 restores the busy-wait (lowest latency on an idle host).
static hipError_t wait_event(hipEvent_t ev) {
  static const bool spin = getenv("MIC_INGEST_SPIN") != nullptr;
  if (spin) return hipEventSynchronize(ev);
  // (hipErrorNotReady is recorded as the thread's last error like any other: an error of a launch before the wait is taken
  // out first and returned, and the "not ready" answers are taken out behind the wait - hipGetLastError() keeps its meaning
  // for the launches that follow)
  hipError_t pending = hipGetLastError();
  if (pending != hipSuccess) return pending;
  struct timespec ts = {0, 30000};                     // 30 us: a batch takes ~1 ms on the device
  hipError_t e;
  for (int i = 0;; ++i) {
    e = hipEventQuery(ev);
    if (e != hipErrorNotReady) break;
    if (i >= 64) nanosleep(&ts, nullptr);              // a batch that is nearly done: a few microseconds of queries first
  }
  (void)hipGetLastError();
  return e;
}

// one host wait of a batch: until `on` has done what was enqueued on it so far
hipError_t wait_stream(Slot& s, hipStream_t on) {
  const hipError_t e = hipEventRecord(s.ev, on);
  return e != hipSuccess ? e : wait_event(s.ev);
}

// A slot is ONE device allocation and ONE pinned allocation carved into its arrays (a few hundred hipMalloc /
// hipHostMalloc calls cost more than the first batches take): pass 1 adds the sizes up, pass 2 hands the pieces out.
struct Arena {
  char* base = nullptr; size_t off = 0;
  template <typename T> void take(T** p, size_t n) {
    off = (off + 255) & ~(size_t)255;
    if (base) *p = (T*)(base + off);
    off += n * sizeof(T) + 64;
  }
};

void carve_slot(Ingest* g, Slot& s, Arena& dv, Arena& hs, size_t tmp) {
  hs.take(&s.h_raw, g->max_bytes + 64);
  hs.take(&s.h_csv, g->csv_cap);
  hs.take(&s.h_hdr, (size_t)H_WORDS);
  if (g->want_results) hs.take(&s.h_results, g->max_reads * 8);
  dv.take(&s.d_raw, g->max_bytes + 64);
  dv.take(&s.d_tile, g->max_tiles + 1);
  dv.take(&s.d_tile_off, g->max_tiles + 1);
  dv.take(&s.d_line_start, g->max_lines + 2);
  dv.take(&s.d_flag, g->max_lines + 2);
  dv.take(&s.d_rec_of_line, g->max_lines + 2);
  dv.take(&s.d_hdr_line, g->max_reads + 2);
  dv.take(&s.rec.name_s, g->max_reads + 1);
  dv.take(&s.rec.seq_s, g->max_reads + 1);
  dv.take(&s.rec.seq_e, g->max_reads + 1);
  dv.take(&s.rec.length, g->max_reads + 1);
  dv.take(&s.rec.bound, g->max_reads + 1);
  dv.take(&s.rec.name_len, g->max_reads + 1);
  dv.take(&s.d_rp, g->max_reads + 2);
  dv.take(&s.d_cont, g->cont_cap + 192);
  dv.take(&s.d_results, (g->max_reads + 1) * 8);
  dv.take(&s.d_flagged, (size_t)kFlaggedCapI + 1);
  if (g->crowd_reads) dv.take(&s.d_crowd, mic_crowd_dims(g->max_reads / 4 + 64).words);
  dv.take(&s.d_line_len, g->max_reads + 1);
  dv.take(&s.d_line_off, g->max_reads + 1);
  dv.take(&s.d_csv, g->csv_cap);
  dv.take(&s.d_hdr, (size_t)H_WORDS);
  dv.take((char**)&s.d_tmp, tmp);
  s.tmp_bytes = tmp;
}

int alloc_slot(Ingest* g, Slot& s, size_t tmp, int device) {
  if (hipSetDevice(device) != hipSuccess) return mic_set_error(MIC_E_HIP, "hipSetDevice failed");
  Arena dv, hs;
  carve_slot(g, s, dv, hs, tmp);
  void* d = nullptr; void* h = nullptr;
  hipError_t e = hipMalloc(&d, dv.off + 256);
  if (e != hipSuccess) return mic_set_error(MIC_E_NOMEM, "ingest slot: %zu bytes of device memory: %s", dv.off, hipGetErrorString(e));
  s.dev_allocs.push_back(d);
  mic_bind_thread_near_device(device, 1);           // pinned memory on the device's socket: the link runs ~1.4x faster
  e = hipHostMalloc(&h, hs.off + 256, hipHostMallocDefault);
  if (e == hipSuccess) memset(h, 0, hs.off + 256);
  mic_bind_thread_near_device(device, 0);
  if (e != hipSuccess) return mic_set_error(MIC_E_NOMEM, "ingest slot: %zu bytes of pinned memory: %s", hs.off, hipGetErrorString(e));
  s.host_allocs.push_back(h);
  Arena dv2, hs2;
  dv2.base = (char*)d; hs2.base = (char*)h;
  carve_slot(g, s, dv2, hs2, tmp);
  if ((e = mic_stream_get(&s.stream)) != hipSuccess ||
      (e = mic_event_get(&s.ev, false)) != hipSuccess ||
      (e = mic_event_get(&s.ev_up, false)) != hipSuccess ||
      (e = mic_event_get(&s.ev_k, false)) != hipSuccess ||
      // the query kernel's read-ahead looks past the last read of a batch: no stale length slots there
      (e = hipMemsetAsync(s.d_cont, 0, (g->cont_cap + 192) * 2, s.stream)) != hipSuccess ||
      (e = hipStreamSynchronize(s.stream)) != hipSuccess)
    return mic_set_error(MIC_E_HIP, "ingest slot setup: %s", hipGetErrorString(e));
  return MIC_OK;
}

void free_peers(Slot& s);
void free_ingest(Ingest* g) {
  if (!g) return;
  for (Slot& s : g->slots) {
    if (s.stream) hipStreamSynchronize(s.stream);
    free_peers(s);
    if (s.ev_pack) mic_event_put(s.ev_pack);
    hipSetDevice(g->device);
    for (void* p : s.dev_allocs) hipFree(p);
    for (void* p : s.host_allocs) hipHostFree(p);
    if (s.ev) mic_event_put(s.ev);
    if (s.ev_up) mic_event_put(s.ev_up);
    if (s.ev_k) mic_event_put(s.ev_k);
    if (s.stream) mic_stream_put(s.stream);
  }
  if (g->d_tnames) hipFree(g->d_tnames);
  if (g->d_tname_off) hipFree(g->d_tname_off);
  delete g;
}

// the slot's roll-up buffers for rows of rw words (a slot that changes between single-engine and table-sharded batches gets new ones)
int ensure_rollup_buffers(Ingest* g, Slot& s, uint32_t rw) {
  if (s.d_rollup && s.ru_row_words == rw) return MIC_OK;
  const size_t n = g->max_reads + 1;
  void* d = nullptr;
  hipError_t e = hipMalloc(&d, n * ((size_t)rw + MIC_ROLLUP_WORDS) * 4 + 512);
  if (e != hipSuccess) return mic_set_error(MIC_E_NOMEM, "ingest slot: roll-up rows of %u words for %zu reads: %s", rw, n, hipGetErrorString(e));
  s.dev_allocs.push_back(d);
  s.d_rollup = (uint32_t*)d;
  s.d_ru_rows = (uint32_t*)((char*)d + ((n * MIC_ROLLUP_WORDS * 4 + 255) & ~(size_t)255));
  s.ru_row_words = rw;
  if (g->want_results && !s.h_rollup) {
    void* h = nullptr;
    e = hipHostMalloc(&h, n * MIC_ROLLUP_WORDS * 4, hipHostMallocDefault);
    if (e != hipSuccess) return mic_set_error(MIC_E_NOMEM, "ingest slot: pinned roll-up rows: %s", hipGetErrorString(e));
    s.host_allocs.push_back(h);
    s.h_rollup = (uint32_t*)h;
  }
  return MIC_OK;
}

// the slot's split buffers: one device allocation and one pinned one, with the slot's first batch that is split; they go with the slot
int ensure_split_buffers(Ingest* g, Slot& s) {
  if (s.d_split) return MIC_OK;
  const size_t text = (g->max_bytes + 8 + 255) & ~(size_t)255, arr = ((g->max_reads + 2) * 8 + 255) & ~(size_t)255;
  const size_t tmp = mic_split_tmp_bytes(g->max_reads + 2);
  void* d = nullptr; void* h = nullptr;
  // the pinned buffer first: when it fails nothing is held, when the device allocation fails it is given back
  mic_bind_thread_near_device(g->device, 1);
  hipError_t e = hipHostMalloc(&h, text + 64, hipHostMallocDefault);
  if (e == hipSuccess) memset((char*)h + text, 0, 64);
  mic_bind_thread_near_device(g->device, 0);
  if (e != hipSuccess) return mic_set_error(MIC_E_NOMEM, "ingest slot: %zu bytes of pinned memory for the split text: %s", text + 64, hipGetErrorString(e));
  e = hipMalloc(&d, text + 2 * arr + 256 + tmp);
  if (e != hipSuccess) {
    hipHostFree(h);
    return mic_set_error(MIC_E_NOMEM, "ingest slot: split buffers of %zu bytes: %s", text + 2 * arr + 256 + tmp, hipGetErrorString(e));
  }
  s.host_allocs.push_back(h);
  s.dev_allocs.push_back(d);
  char* q = (char*)d;
  s.split_b.d_len2 = (unsigned long long*)(q + text); s.split_b.d_off2 = (unsigned long long*)(q + text + arr);
  s.split_b.d_ncls = (uint32_t*)(q + text + 2 * arr); s.split_b.d_tmp = q + text + 2 * arr + 256; s.split_b.tmp_bytes = tmp;
  s.h_split = (uint8_t*)h; s.h_split_tot = (uint64_t*)((char*)h + text);
  s.d_split = (uint8_t*)d;
  return MIC_OK;
}

// the slot's hit-map buffers: the fixed arrays once; the word buffer for at least `words` words and the text buffer (with its pinned
// twin) for at least `text` bytes - grown, never shrunk; what they held is not kept (the caller grows them before the pass that fills them)
// A buffer that grows is in the slot's allocation lists like every other (free_ingest frees what the lists hold): the grown one is
// pushed there, the outgrown one is given back with this (is_dev: dev_allocs and hipFree, else host_allocs and hipHostFree)
template <typename T> void drop_alloc(Slot& s, T*& p, bool is_dev) {
  if (!p) return;
  std::vector<void*>& list = is_dev ? s.dev_allocs : s.host_allocs;
  list.erase(std::remove(list.begin(), list.end(), (void*)p), list.end());
  if (is_dev) hipFree(p); else hipHostFree(p);
  p = nullptr;
}
size_t hitmap_scan64_bytes(size_t n_items) {
  size_t tb = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)n_items);
  return tb + 256;
}
int ensure_hitmap_buffers(Ingest* g, Slot& s, size_t words, size_t text) {
  hipError_t e;
  if (!s.d_hm_cnt) {
    const size_t n = g->max_reads + 2;
    const size_t a32 = (n * 4 + 255) & ~(size_t)255, a64 = (n * 8 + 255) & ~(size_t)255;
    const size_t tmp = std::max(mic_hitmap_tmp_bytes(n), hitmap_scan64_bytes(n));
    void* d = nullptr; void* h = nullptr;
    e = hipHostMalloc(&h, 64, hipHostMallocDefault);
    if (e != hipSuccess) return mic_set_error(MIC_E_NOMEM, "ingest slot: pinned memory for the hit maps' totals: %s", hipGetErrorString(e));
    memset(h, 0, 64);
    e = hipMalloc(&d, 2 * a32 + 2 * a64 + tmp);
    if (e != hipSuccess) {
      hipHostFree(h);
      return mic_set_error(MIC_E_NOMEM, "ingest slot: hit-map arrays of %zu bytes: %s", 2 * a32 + 2 * a64 + tmp, hipGetErrorString(e));
    }
    s.host_allocs.push_back(h);
    s.dev_allocs.push_back(d);
    char* q = (char*)d;
    s.d_hm_len = (unsigned long long*)q; s.d_hm_loff = (unsigned long long*)(q + a64);
    s.d_hm_cnt = (uint32_t*)(q + 2 * a64); s.d_hm_off = (uint32_t*)(q + 2 * a64 + a32);
    s.d_hm_tmp = q + 2 * a64 + 2 * a32; s.hm_tmp_bytes = tmp;
    s.h_hm_tot = (uint64_t*)h;
    // first sizes: a word per 64 bytes of the slot's text (a 150-nt read without its quality line is ~165 bytes and a few runs), a
    // quarter of its bytes of text (a name, a comma and ~10 bytes per run); a batch of denser maps grows them once
    words = std::max(words, g->max_bytes / 64);
    text = std::max(text, g->max_bytes / 4);
  }
  if (words > s.hm_words_cap) {
    const size_t cap = std::max(words + words / 2, (size_t)1024);
    drop_alloc(s, s.d_hm_words, true);
    s.hm_words_cap = 0;
    void* d = nullptr;
    e = hipMalloc(&d, cap * 4);
    if (e != hipSuccess) return mic_set_error(MIC_E_NOMEM, "ingest slot: %zu hit-map words: %s", cap, hipGetErrorString(e));
    s.dev_allocs.push_back(d);
    s.d_hm_words = (uint32_t*)d; s.hm_words_cap = cap;
  }
  if (text > s.hm_text_cap) {
    const size_t cap = (std::max(text + text / 4, (size_t)4096) + 255) & ~(size_t)255;
    drop_alloc(s, s.d_hm_text, true);
    drop_alloc(s, s.h_hm_text, false);
    s.hm_text_cap = 0;
    void* d = nullptr; void* h = nullptr;
    mic_bind_thread_near_device(g->device, 1);
    e = hipHostMalloc(&h, cap, hipHostMallocDefault);
    mic_bind_thread_near_device(g->device, 0);
    if (e != hipSuccess) return mic_set_error(MIC_E_NOMEM, "ingest slot: %zu bytes of pinned memory for the hit-map text: %s", cap, hipGetErrorString(e));
    e = hipMalloc(&d, cap);
    if (e != hipSuccess) { hipHostFree(h); return mic_set_error(MIC_E_NOMEM, "ingest slot: %zu bytes of hit-map text: %s", cap, hipGetErrorString(e)); }
    s.host_allocs.push_back(h);
    s.dev_allocs.push_back(d);
    s.d_hm_text = (char*)d; s.h_hm_text = (char*)h; s.hm_text_cap = cap;
  }
  return MIC_OK;
}

// ---- table-sharded batches: the slot's buffers on the engines of its group, and the exchange ------------------------------
const uint32_t kGroupRowWords = 16;      // 15 (target, count) pairs per partial row = the reference's MAXHITS rows (parameters.hh:44)

// reads whose summed row did not fit (result word 6: MIC_FLAG_ROW_OVERFLOW) are counted into the slot's flagged counter: the
// batch is then handed back with MIC_INGEST_DENSE like a batch with a read of more than 64 targets
__global__ void __launch_bounds__(256) group_overflow_kernel(const uint32_t* __restrict__ results, uint32_t n, uint32_t* __restrict__ flagged) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && (results[(size_t)i * 8 + 6] & MIC_FLAG_ROW_OVERFLOW_)) atomicAdd(&flagged[0], 1u);
}

void free_peers(Slot& s) {
  for (Slot::Peer& p : s.peers) {
    hipSetDevice(p.device);
    if (p.stream && p.stream != s.stream) { hipStreamSynchronize(p.stream); mic_stream_put(p.stream); }
    if (p.ev_q) mic_event_put(p.ev_q);
    if (p.ev_done) mic_event_put(p.ev_done);
    for (hipEvent_t e : p.tv) if (e) mic_event_put(e);
    if (p.block) hipFree(p.block);
  }
  s.peers.clear();
}

static bool group_timing() { static const bool on = getenv("MIC_GROUP_TIMING") != nullptr; return on; }

// The engines of a group must answer for ONE database cut into disjoint pieces that cover it: the same k and target count, and
// either slot-range parts (mic_db_set_part on a super-k-mer table) or bucket ranges (the other layouts, explicit shards) that
// tile the whole table.  Engines that each hold the whole table, or overlapping pieces, would count every hit several times.
int check_group(mic_engine* const* group, size_t P) {
  struct Piece { uint64_t lo, hi; };
  std::vector<Piece> pieces(P);
  int k0 = 0, layout0 = 0, parted0 = 0; uint32_t nt0 = 0; uint64_t whole = 0;
  for (size_t p = 0; p < P; ++p) {
    MicTable t; int sc, ncu, dev, k; uint32_t nt;
    int rc = mic_engine_table(group[p], &t, &sc, &ncu, &dev, &k, &nt);
    if (rc) return rc;
    if (!t.slots) return mic_set_error(MIC_E_STATE, "no database loaded on engine %zu of the group", p);
    if (p == 0) { k0 = k; nt0 = nt; layout0 = t.layout; parted0 = t.parted; whole = t.parted ? t.n_main : t.div.d; }
    if (k != k0 || nt != nt0) return mic_set_error(MIC_E_INVALID, "engine %zu of the group differs in k or in the number of targets (%d / %u against %d / %u)", p, k, nt, k0, nt0);
    if (t.layout != layout0 || t.parted != parted0) return mic_set_error(MIC_E_INVALID, "engine %zu of the group holds another table layout than engine 0", p);
    if (t.parted) {
      if (t.n_main != whole) return mic_set_error(MIC_E_INVALID, "engine %zu of the group holds a part of another table (%llu slots against %llu)", p, (unsigned long long)t.n_main, (unsigned long long)whole);
      pieces[p] = {t.slot_lo, (uint64_t)t.slot_lo + t.slot_cnt};
    } else {
      if (t.div.d != whole) return mic_set_error(MIC_E_INVALID, "engine %zu of the group holds a table of another size", p);
      pieces[p] = {t.shard_start, t.shard_end};
    }
  }
  std::sort(pieces.begin(), pieces.end(), [](const Piece& a, const Piece& b) { return a.lo < b.lo || (a.lo == b.lo && a.hi < b.hi); });
  uint64_t at = 0;
  for (size_t p = 0; p < P; ++p) {
    if (pieces[p].lo == pieces[p].hi) continue;            // (an empty part answers nothing)
    if (pieces[p].lo != at)
      return mic_set_error(MIC_E_INVALID, "the engines of the group do not hold disjoint pieces that cover the table: piece [%llu, %llu) follows %llu%s",
                           (unsigned long long)pieces[p].lo, (unsigned long long)pieces[p].hi, (unsigned long long)at,
                           P > 1 && pieces[p].lo == 0 && pieces[p].hi == whole ? " (whole tables: use mic_db_set_part)" : "");
    at = pieces[p].hi;
  }
  if (at != whole) return mic_set_error(MIC_E_INVALID, "the engines of the group cover %llu of %llu %s of the table", (unsigned long long)at,
                                        (unsigned long long)whole, parted0 ? "slots" : "buckets");
  return MIC_OK;
}

int setup_peers(Ingest* g, Slot& s, mic_engine* const* group, size_t P, size_t owner) {
  free_peers(s);
  int rc = check_group(group, P);
  if (rc) return rc;
  s.peers.resize(P);
  s.group_owner = owner;
  s.timed = group_timing();
  const size_t len_max = g->max_reads / P + 2, rw = kGroupRowWords;
  for (size_t p = 0; p < P; ++p) {
    Slot::Peer& q = s.peers[p];
    MicTable t; int sc, ncu, dev, k; uint32_t nt;
    rc = mic_engine_table(group[p], &t, &sc, &ncu, &dev, &k, &nt);
    if (rc) return rc;
    q.eng = group[p]; q.device = dev; q.table_id = t.slots;
    MIC_TRY(hipSetDevice(dev));
    const bool own = p == owner;
    for (int pass = 0; pass < 2; ++pass) {          // pass 0 adds the sizes up, pass 1 hands the pieces out
      Arena a;
      a.base = pass ? (char*)q.block : nullptr;
      a.take(&q.d_rows, (g->max_reads + 1) * rw);
      a.take(&q.d_gather, (P - 1) * len_max * rw);
      a.take(&q.d_acc, len_max * rw);
      a.take(&q.d_acc2, len_max * rw);
      if (!own) {
        a.take(&q.d_rp, g->max_reads + 2);
        a.take(&q.d_cont, g->cont_cap + 192);
        a.take(&q.d_res, (g->max_reads + 1) * 8);
        a.take(&q.d_flagged, (size_t)kFlaggedCapI + 1);
        if (t.side) a.take(&q.d_crowd, mic_crowd_dims(g->max_reads / 4 + 64).words);      // (a helper whose PART has a side table, whatever the owner's has)
      }
      if (!pass) {
        hipError_t e = hipMalloc(&q.block, a.off + 256);
        if (e != hipSuccess) return mic_set_error(MIC_E_NOMEM, "table-sharded ingest slot: %zu bytes on device %d: %s", a.off, dev, hipGetErrorString(e));
      }
    }
    MIC_TRY(mic_event_get(&q.ev_q, false));
    MIC_TRY(mic_event_get(&q.ev_done, false));
    if (s.timed) for (hipEvent_t& e : q.tv) MIC_TRY(mic_event_get(&e, true));
    if (own) { q.d_rp = s.d_rp; q.d_cont = s.d_cont; q.d_res = s.d_results; q.d_flagged = s.d_flagged; q.d_crowd = s.d_crowd; q.stream = s.stream; }
    else {
      MIC_TRY(mic_stream_get(&q.stream));
      MIC_TRY(hipMemsetAsync(q.d_cont, 0, (g->cont_cap + 192) * 2, q.stream));     // (the query kernel's read-ahead looks past the last read)
      MIC_TRY(hipStreamSynchronize(q.stream));
    }
  }
  MIC_TRY(hipSetDevice(s.peers[owner].device));
  if (!s.ev_pack) MIC_TRY(mic_event_get(&s.ev_pack, false));
  mic_peer_enable_engines(group, P);
  return MIC_OK;
}

// Every engine of the group probes the batch's packed reads (on the owner's device after pack_kernel) against its part; the rows
// are summed read-range owned; the owner's d_results hold best / second-best of all reads when its stream has passed the waits
// queued here.  Nothing blocks the host.
int group_query_issue(mic_engine* const* group, size_t P, size_t owner, Ingest* g, Slot& s, uint32_t n, uint32_t nb, int k, uint32_t* d_merged) {
  const size_t rw = kGroupRowWords;
  Slot::Peer& O = s.peers[owner];
  // containers the packer can have written for nb bytes in n reads (record_kernel's reservations) + what the kernel reads ahead
  const size_t cont_n = std::min<size_t>(g->cont_cap + 192, (size_t)nb / 8 + 2 * ((size_t)nb / (size_t)(k + 1)) + 10 * (size_t)n + 128);
  const bool timed = s.timed;
  s.fan_bytes = s.x_bytes = 0;
  MIC_TRY(hipSetDevice(O.device));
  MIC_TRY(hipEventRecord(s.ev_pack, s.stream));
  for (size_t p = 0; p < P; ++p) {
    Slot::Peer& q = s.peers[p];
    MicTable t; int sc, ncu, dev, kk; uint32_t nt;
    int rc = mic_engine_table(group[p], &t, &sc, &ncu, &dev, &kk, &nt);
    if (rc) return rc;
    if (!t.slots) return mic_set_error(MIC_E_STATE, "no database loaded on engine %zu of the group", p);
    MIC_TRY(hipSetDevice(dev));
    if (p != owner) {
      MIC_TRY(hipStreamWaitEvent(q.stream, s.ev_pack, 0));
      if (timed) MIC_TRY(hipEventRecord(q.tv[0], q.stream));
      MIC_TRY(hipMemcpyPeerAsync(q.d_rp, dev, O.d_rp, O.device, ((size_t)n + 2) * 4, q.stream));
      MIC_TRY(hipMemcpyPeerAsync(q.d_cont, dev, O.d_cont, O.device, cont_n * 2, q.stream));
      s.fan_bytes += ((size_t)n + 2) * 4 + cont_n * 2;
    } else if (timed) MIC_TRY(hipEventRecord(q.tv[0], q.stream));
    MIC_TRY(hipMemsetAsync(q.d_flagged, 0, 4, q.stream));
    if (timed) MIC_TRY(hipEventRecord(q.tv[1], q.stream));
    MicQueryArgs qa;
    qa.t = t; qa.reads_ptr = q.d_rp; qa.cont = q.d_cont; qa.n_reads = n; qa.row_words = (uint32_t)rw; qa.results = q.d_res;
    qa.rows = q.d_rows; qa.flagged = q.d_flagged; qa.flagged_cap = kFlaggedCapI;
    mic_crowd_attach(qa, q.d_crowd, g->max_reads / 4 + 64);
    MIC_TRY(mic_launch_query(qa, sc, ncu, q.stream));
    MIC_TRY(hipEventRecord(q.ev_q, q.stream));
    if (timed) MIC_TRY(hipEventRecord(q.tv[2], q.stream));
  }
  for (size_t j = 0; j < P; ++j) {
    Slot::Peer& q = s.peers[j];
    const size_t lo = (size_t)n * j / P, hi = (size_t)n * (j + 1) / P, len = hi - lo;
    MIC_TRY(hipSetDevice(q.device));
    if (timed) {
      // measuring runs: the stream first waits for EVERY engine's rows, so that what tv[3] .. tv[4] brackets is the copies and the
      // merges alone and not the other engines' kernels (the product form below lets a copy start as soon as its source is written)
      for (size_t p = 0; p < P; ++p) if (p != j) MIC_TRY(hipStreamWaitEvent(q.stream, s.peers[p].ev_q, 0));
      MIC_TRY(hipEventRecord(q.tv[3], q.stream));
    }
    if (len) {
      // the running sum: this engine's own rows of the range, then the two spare buffers in turn (the partial rows stay as the
      // kernel wrote them: mic_ingest_fetch_group_rows)
      const uint32_t* cur = q.d_rows + lo * rw;
      uint32_t* spare[2] = {q.d_acc, q.d_acc2};
      int c = 0; size_t got = 0;
      for (size_t p = 0; p < P; ++p) {
        if (p == j) continue;
        uint32_t* in = q.d_gather + got * len * rw;
        if (!timed) MIC_TRY(hipStreamWaitEvent(q.stream, s.peers[p].ev_q, 0));
        MIC_TRY(hipMemcpyPeerAsync(in, q.device, s.peers[p].d_rows + lo * rw, s.peers[p].device, len * rw * 4, q.stream));
        MIC_TRY(mic_launch_merge_rows(cur, in, spare[c], (uint32_t)rw, len, nullptr, q.stream));
        cur = spare[c]; c ^= 1; ++got;
        s.x_bytes += len * rw * 4;
      }
      if (j == owner) MIC_TRY(mic_launch_result_from_rows(cur, (uint32_t)rw, O.d_res + lo * 8, len, q.stream));
      else {
        MIC_TRY(mic_launch_result_from_rows(cur, (uint32_t)rw, q.d_res, len, q.stream));
        MIC_TRY(hipMemcpyPeerAsync(O.d_res + lo * 8, O.device, q.d_res, q.device, len * 32, q.stream));
        s.x_bytes += len * 32;
      }
      if (d_merged) {        // roll-up: the summed rows of the range go to the owner as well (64 bytes a read next to the 32 of its result)
        MIC_TRY(hipMemcpyPeerAsync(d_merged + lo * rw, O.device, cur, q.device, len * rw * 4, q.stream));
        if (j != owner) s.x_bytes += len * rw * 4;
      }
    }
    if (timed) MIC_TRY(hipEventRecord(q.tv[4], q.stream));
    MIC_TRY(hipEventRecord(q.ev_done, q.stream));
  }
  MIC_TRY(hipSetDevice(O.device));
  for (size_t j = 0; j < P; ++j) if (j != owner) MIC_TRY(hipStreamWaitEvent(s.stream, s.peers[j].ev_done, 0));
  group_overflow_kernel<<<(n + 255) / 256, 256, 0, s.stream>>>(O.d_res, n, s.d_flagged);
  MIC_TRY(hipGetLastError());
  return MIC_OK;
}

int group_query(mic_engine* const* group, size_t P, size_t owner, Ingest* g, Slot& s, uint32_t n, uint32_t nb, int k, uint32_t* d_merged) {
  // the slot's buffers on the engines of its group are kept from batch to batch while the group is the same: the same engines in the
  // same order, each on the device and with the table it had (an engine destroyed and another created at its address is not the same)
  bool same = s.peers.size() == P && s.group_owner == owner && s.timed == group_timing();
  for (size_t p = 0; same && p < P; ++p) {
    MicTable t; int sc, ncu, dev, kk; uint32_t nt;
    same = s.peers[p].eng == group[p] && mic_engine_table(group[p], &t, &sc, &ncu, &dev, &kk, &nt) == MIC_OK &&
           dev == s.peers[p].device && (const void*)t.slots == s.peers[p].table_id;
  }
  if (!same) { int rc = setup_peers(g, s, group, P, owner); if (rc) { free_peers(s); return rc; } }
  const int rc = group_query_issue(group, P, owner, g, s, n, nb, k, d_merged);
  if (rc) {
    // an error in the middle leaves work queued on the helpers' streams that reads and writes the slot's buffers: wait for it
    // before the caller reuses or frees them (the error text is kept)
    const std::string msg = mic_last_error();
    for (Slot::Peer& q : s.peers) if (q.stream) { hipSetDevice(q.device); hipStreamSynchronize(q.stream); }
    (void)hipGetLastError();
    hipSetDevice(s.peers[owner].device);
    return mic_set_error(rc, "%s", msg.c_str());
  }
  return MIC_OK;
}

// MIC_GROUP_TIMING: the slot's last table-sharded batch has finished (the owner's stream waited for every engine): its events' times
void group_harvest(Ingest* g, Slot& s, uint32_t n) {
  if (!s.timed || s.peers.empty()) return;
  double fan_sum = 0, fan_max = 0, k_sum = 0, k_max = 0, x_sum = 0, x_max = 0;
  for (size_t p = 0; p < s.peers.size(); ++p) {
    Slot::Peer& q = s.peers[p];
    hipSetDevice(q.device);
    float fan = 0, kq = 0, x = 0;
    if (hipEventElapsedTime(&fan, q.tv[0], q.tv[1]) != hipSuccess || hipEventElapsedTime(&kq, q.tv[1], q.tv[2]) != hipSuccess ||
        hipEventElapsedTime(&x, q.tv[3], q.tv[4]) != hipSuccess) { (void)hipGetLastError(); return; }
    if (p != s.group_owner) { fan_sum += fan; fan_max = std::max(fan_max, (double)fan); }
    k_sum += kq; k_max = std::max(k_max, (double)kq);
    x_sum += x; x_max = std::max(x_max, (double)x);
  }
  hipSetDevice(g->device);
  std::lock_guard<std::mutex> lk(g->gstats.mu);
  GroupStats& G = g->gstats;
  ++G.batches; G.reads += n; G.fan_bytes += s.fan_bytes; G.x_bytes += s.x_bytes;
  G.fan_ms_sum += fan_sum; G.fan_ms_max += fan_max; G.kernel_ms_sum += k_sum; G.kernel_ms_max += k_max; G.x_ms_sum += x_sum; G.x_ms_max += x_max;
}

}  // namespace

extern "C" {

int mic_ingest_alloc(mic_engine* e, size_t n_slots, size_t max_bytes, const char* const* target_names, uint32_t n_targets,
                     int want_results, uint8_t** raw) {
  if (!e || !raw || n_slots == 0 || n_slots > 64) return mic_set_error(MIC_E_INVALID, "bad argument");
  // at most 128 MiB: with the per-line bound of csv_len_kernel (768 bytes) the 32-bit scan of the CSV line lengths cannot wrap
  if (max_bytes < 4096 || max_bytes > ((size_t)128 << 20)) return mic_set_error(MIC_E_INVALID, "ingest slots hold 4 KiB .. 128 MiB of input");
  MicTable t; int sc, ncu, dev, k; uint32_t nt;
  int rc = mic_engine_table(e, &t, &sc, &ncu, &dev, &k, &nt);
  if (rc) return rc;
  MIC_TRY(hipSetDevice(dev));
  mic_ingest_free(e);
  Ingest* g = new Ingest();
  g->eng = e; g->device = dev;
  g->max_bytes = (max_bytes + MIC_LINE_TILE - 1) / MIC_LINE_TILE * MIC_LINE_TILE;
  g->max_tiles = g->max_bytes / MIC_LINE_TILE;
  g->max_lines = g->max_bytes / 16 + 64;          // fewer than 16 bytes per line on average: host path
  g->max_reads = g->max_bytes / 32 + 16;          // fewer than 32 bytes per record on average: host path
  // sum of the per-read reservations of record_kernel: nbytes / 8 + 2 (nbytes / (k + 1) + 1) + 8 containers per read
  g->cont_cap = g->max_bytes / 8 + 2 * (g->max_bytes / (size_t)(k + 1)) + 10 * g->max_reads + 64;
  g->csv_cap = g->max_bytes;
  g->crowd_reads = (t.slots && !t.side) ? 0 : g->max_reads / 4 + 64;      // (no table yet: one may come with a side table)
  g->want_results = want_results;
  g->n_targets = n_targets;
  *mic_engine_ingest_slot(e) = g;
  {  // target names on the device
    std::vector<uint32_t> off(n_targets + 1, 0);
    std::vector<char> names;
    for (uint32_t i = 0; i < n_targets; ++i) {
      const char* s = target_names && target_names[i] ? target_names[i] : "";
      names.insert(names.end(), s, s + strlen(s));
      off[i + 1] = (uint32_t)names.size();
    }
    MIC_TRY(hipMalloc(&g->d_tnames, names.size() + 16));
    ingest_warm_kernel<<<1, 64>>>((uint32_t*)g->d_tnames);       // (loads this file's device code now, not with the first batch)
    (void)mic_text_warm(nullptr);                                // (and the line kernels', which live in mic_text.hip)
    MIC_TRY(hipMalloc(&g->d_tname_off, off.size() * 4));
    if (!names.empty()) MIC_TRY(hipMemcpy(g->d_tnames, names.data(), names.size(), hipMemcpyHostToDevice));
    MIC_TRY(hipMemcpy(g->d_tname_off, off.data(), off.size() * 4, hipMemcpyHostToDevice));
  }
  g->slots.resize(n_slots);
  size_t tmp1 = mic_line_scan_bytes(g->max_tiles), tmp2 = 0, tmp3 = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmp2, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)(g->max_lines + 1));
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmp3, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)(g->max_reads + 1));
  const size_t tmp = std::max(tmp1, std::max(tmp2, tmp3)) + 256;
  {  // slots are set up concurrently: pinning host pages is the slow part
    std::vector<int> rcs(n_slots, MIC_OK);
    std::vector<std::string> msgs(n_slots);
    std::vector<std::thread> th;
    // (read splitting already started on the engine: the slots' split buffers come now, pinned side by side, not with the first batches)
    const bool split_now = mic_engine_split(e)->on, hitmap_now = mic_engine_hitmap(e)->on;
    for (size_t i = 0; i < n_slots; ++i)
      th.emplace_back([&, i] {
        rcs[i] = alloc_slot(g, g->slots[i], tmp, dev);
        if (!rcs[i] && split_now) rcs[i] = ensure_split_buffers(g, g->slots[i]);
        if (!rcs[i] && hitmap_now) rcs[i] = ensure_hitmap_buffers(g, g->slots[i], 0, 0);
        if (rcs[i]) msgs[i] = mic_last_error();
      });
    for (auto& t : th) t.join();
    for (size_t i = 0; i < n_slots; ++i) {
      if (rcs[i]) return mic_set_error(rcs[i], "%s", msgs[i].c_str());
      raw[i] = g->slots[i].h_raw;
    }
  }
  return MIC_OK;
}

int mic_ingest_free(mic_engine* e) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  void** slot = mic_engine_ingest_slot(e);
  if (*slot) { free_ingest((Ingest*)*slot); *slot = nullptr; }
  return MIC_OK;
}

int mic_ingest_classify(mic_engine* e, size_t slot_id, size_t n_bytes, int flags, mic_ingest_result* out) {
  return mic_ingest_classify_group(&e, 1, 0, slot_id, n_bytes, flags, out);
}

}  // extern "C"

// ---- one batch through a slot: the stages of mic_ingest_classify_group (below), in the order it runs them -----------------------------
namespace {

// What every stage reads.  A stage returns an error code; one that hands the batch back to the host path sets out->status.
struct BatchCtx {
  Ingest* g = nullptr; Slot* s = nullptr; mic_engine* e = nullptr;      // the slot's engine: the owner of a table-sharded batch
  MicTable t; int sc = 0, ncu = 0, dev = 0, k = 0; uint32_t nt = 0;     // mic_engine_table(e)
  uint32_t n_reads = 0, nb = 0, gr = 0; int paired = 0, fasta = 0; uint32_t lpr = 4;   // gr: blocks of 256 over n_reads + 1 items; lpr: lines per FASTQ record
  // e's base-quality threshold (pack_kernel<true, *>) and low-complexity level (lowc_kernel, pack_kernel<*, true>), 0: none; the modes; e's split setting
  uint32_t c0 = 0, lc = 0; bool no_csv = false, roll = false, resident = false, hitmaps = false; MicSplit sp;
  MicHitmap hm;                                                         // e's hit-map setting: the text's format, the Kraken format's filter
  hipStream_t st = nullptr, up = nullptr, down = nullptr;               // the slot's stream; e's upload and download streams
};

// the slot's Ingest when it has slot `slot_id`, else nullptr with the error set
Ingest* ingest_with_slot(mic_engine* e, size_t slot_id) {
  Ingest* g = (Ingest*)*mic_engine_ingest_slot(e);
  if (!g || slot_id >= g->slots.size()) { mic_set_error(MIC_E_STATE, "ingest slots are not allocated"); return nullptr; }
  return g;
}

// argument checks, every feature's "not supported with" rule, the slot's state cleared; b filled but for n_reads, gr and roll
int begin_batch(mic_engine* const* group, size_t n_group, size_t owner, size_t slot_id, size_t n_bytes, int flags, mic_ingest_result* out,
                BatchCtx& b) {
  if (!group || n_group == 0 || owner >= n_group) return mic_set_error(MIC_E_INVALID, "bad group");
  for (size_t p = 0; p < n_group; ++p) if (!group[p]) return mic_set_error(MIC_E_INVALID, "null engine in the group");
  mic_engine* e = b.e = group[owner];
  // k-mer sketches count the k-mers of ONE engine's table behind ITS query: the table-sharded mode is not integrated
  if (n_group > 1) for (size_t p = 0; p < n_group; ++p) if (mic_engine_ksketch(group[p])->on)
    return mic_set_error(MIC_E_UNSUPPORTED, "k-mer sketches are started on an engine of a table-sharded group: not supported");
  // hit maps are the labels of ONE engine's table along the read: likewise
  if (n_group > 1) for (size_t p = 0; p < n_group; ++p) if (mic_engine_hitmap(group[p])->on)
    return mic_set_error(MIC_E_UNSUPPORTED, "hit maps are started on an engine of a table-sharded group: not supported");
  b.paired = flags & MIC_INGEST_PAIRED; b.no_csv = (flags & MIC_INGEST_NO_CSV) != 0; b.lpr = (flags & MIC_INGEST_FASTQ_2LINE) ? 2u : 4u;
  if (!e || !out) return mic_set_error(MIC_E_INVALID, "null argument");
  b.c0 = *mic_engine_min_quality(e);
  if (b.c0 && b.lpr == 2) return mic_set_error(MIC_E_INVALID, "MIC_INGEST_FASTQ_2LINE while a base-quality threshold is set: the quality lines are gone");
  b.sp = *mic_engine_split(e);
  if (b.sp.on && b.lpr == 2) return mic_set_error(MIC_E_INVALID, "MIC_INGEST_FASTQ_2LINE while read splitting is started: the quality lines are gone");
  b.lc = *mic_engine_low_complexity(e);
  Ingest* g = b.g = ingest_with_slot(e, slot_id); if (!g) return MIC_E_STATE;
  if (n_bytes == 0 || n_bytes > g->max_bytes) return mic_set_error(MIC_E_INVALID, "batch of %zu bytes does not fit the slot (%zu)", n_bytes, g->max_bytes);
  int rc = mic_engine_table(e, &b.t, &b.sc, &b.ncu, &b.dev, &b.k, &b.nt);
  if (rc) return rc;
  if (!b.t.slots) return mic_set_error(MIC_E_STATE, "no database loaded");
  MIC_TRY(hipSetDevice(b.dev));
  Slot& s = *(b.s = &g->slots[slot_id]);
  s.ru_valid = false; s.split_valid = false; s.hm_valid = false;
  b.hm = *mic_engine_hitmap(e); b.hitmaps = b.hm.on;
  if (b.hitmaps && (b.t.sharded || b.t.parted)) return mic_set_error(MIC_E_UNSUPPORTED, "hit maps on a sharded or parted table: not supported");
  memset(out, 0, sizeof(*out));
  b.resident = (flags & MIC_INGEST_RESIDENT) != 0;      // the text is in the slot's device buffer already (mic_pairs_merge_to_slot: merged pairs)
  const uint8_t first = b.resident ? (uint8_t)((flags & MIC_INGEST_RESIDENT_FASTQ) == MIC_INGEST_RESIDENT_FASTQ ? '@' : '>') : s.h_raw[0];
  if (first != '>' && first != '@') { out->status = MIC_INGEST_FALLBACK | MIC_INGEST_ODD_RECORD; return MIC_OK; }
  b.fasta = first == '>';
  b.st = s.stream; b.nb = (uint32_t)n_bytes;
  mic_engine_copy_streams(e, &b.up, &b.down);
  return MIC_OK;
}

// phase 1: bytes -> lines -> number of records, the header to the host and the batch's first wait.  The upload runs on the engine's
// upload stream, the CSV comes back on its download stream (mic_engine.hip: one stream per direction keeps both directions busy)
int index_records(BatchCtx& b, mic_ingest_result* out) {
  Ingest* g = b.g; Slot& s = *b.s; const hipStream_t st = b.st;
  const uint32_t nb = b.nb, n_tiles = mic_line_tiles(nb), lpr = b.lpr; const int fasta = b.fasta;
  if (!b.resident) {
    MIC_TRY(hipMemcpyAsync(s.d_raw, s.h_raw, nb, hipMemcpyHostToDevice, b.up));
    MIC_TRY(hipEventRecord(s.ev_up, b.up));
    MIC_TRY(hipStreamWaitEvent(st, s.ev_up, 0));
  }
  MIC_TRY(hipMemsetAsync(s.d_hdr, 0, H_WORDS * 4, st));
  MIC_TRY(mic_line_ends(s.d_raw, nb, 0, s.d_tile, s.d_tile_off, s.d_tmp, s.tmp_bytes, st));
  MIC_TRY(mic_line_starts(s.d_raw, nb, 0, s.d_tile_off, s.d_line_start, (uint32_t)g->max_lines, st));
  lines_finish_kernel<<<1, 1, 0, st>>>(s.d_raw, nb, s.d_tile_off, n_tiles, s.d_line_start, (uint32_t)g->max_lines, fasta, lpr, (uint32_t)g->max_reads, s.d_hdr);
  if (fasta) {
    // a line is at least one byte long, so there are at most nb of them: flags and their scan cover lines 0 .. n_scan - 1
    // (n_lines < n_scan whenever the batch is within the slot's line capacity)
    const uint32_t n_scan = (uint32_t)std::min<size_t>(g->max_lines, (size_t)nb + 2);
    const uint32_t gl = (n_scan + 255) / 256;
    fasta_flag_kernel<<<gl, 256, 0, st>>>(s.d_raw, nb, s.d_line_start, s.d_hdr, (uint32_t)g->max_lines, n_scan, s.d_flag);
    size_t tb = s.tmp_bytes;
    MIC_TRY(hipcub::DeviceScan::ExclusiveSum(s.d_tmp, tb, s.d_flag, s.d_rec_of_line, (int)n_scan, st));
    fasta_scatter_kernel<<<gl, 256, 0, st>>>(s.d_flag, s.d_rec_of_line, (uint32_t)g->max_lines, (uint32_t)g->max_reads, s.d_hdr_line, s.d_hdr);
  }
  MIC_TRY(hipMemcpyAsync(s.h_hdr, s.d_hdr, H_WORDS * 4, hipMemcpyDeviceToHost, st));
  MIC_TRY(wait_stream(s, st));
  b.n_reads = s.h_hdr[H_NREADS]; b.gr = (b.n_reads + 1 + 255) / 256;
  out->n_lines = s.h_hdr[H_NLINES];
  if (s.h_hdr[H_STATUS] || b.n_reads == 0) out->status = MIC_INGEST_FALLBACK | s.h_hdr[H_STATUS];
  return MIC_OK;
}

// lowc_kernel (LOWC) and pack_kernel<QUAL, LOWC>: the arguments of the four instantiations in one place
template <bool QUAL, bool LOWC>
void launch_pack(const BatchCtx& b, unsigned blocks) {
  Slot& s = *b.s; const uint32_t* line_start = QUAL ? s.d_line_start : nullptr; const uint32_t c0 = QUAL ? b.c0 : 0u;
  if (LOWC) lowc_kernel<QUAL><<<blocks, 256, 0, b.st>>>(s.d_raw, s.rec.seq_s, s.rec.seq_e, s.d_rp, b.n_reads, b.lc, line_start, c0, s.d_lowc);
  pack_kernel<QUAL, LOWC><<<blocks, 256, 0, b.st>>>(s.d_raw, s.rec.seq_s, s.rec.seq_e, s.d_rp, s.d_cont, b.n_reads, b.k, line_start, c0,
                                                    LOWC ? s.d_lowc : nullptr);
}

// phase 2 begins: records -> packed reads
int pack_reads(BatchCtx& b) {
  Slot& s = *b.s; const hipStream_t st = b.st; const uint32_t n_reads = b.n_reads, nb = b.nb;
  if (b.fasta) record_kernel<true><<<b.gr, 256, 0, st>>>(s.d_raw, nb, s.d_line_start, s.d_hdr_line, n_reads, b.lpr, b.k, s.rec, s.d_hdr);
  else record_kernel<false><<<b.gr, 256, 0, st>>>(s.d_raw, nb, s.d_line_start, nullptr, n_reads, b.lpr, b.k, s.rec, s.d_hdr);
  size_t tb = s.tmp_bytes;
  MIC_TRY(hipcub::DeviceScan::ExclusiveSum(s.d_tmp, tb, s.rec.bound, s.d_rp, (int)(n_reads + 1), st));
  unsigned blocks = (n_reads + 3) / 4, cap = (unsigned)b.ncu * 64u;
  if (blocks > cap) blocks = cap;
  const bool qual = b.c0 && !b.fasta;
  if (b.lc) {
    if (!s.d_lowc) {   // the slot's first batch that is masked: one bit per byte of the slot's text; it goes with the slot
      void* d = nullptr;
      MIC_TRY(hipMalloc(&d, b.g->max_bytes / 8 + 64));
      s.dev_allocs.push_back(d);
      s.d_lowc = (uint32_t*)d;
    }
    MIC_TRY(hipMemsetAsync(s.d_lowc, 0, ((size_t)nb + 31) / 32 * 4, st));
    qual ? launch_pack<true, true>(b, blocks) : launch_pack<false, true>(b, blocks);
  } else qual ? launch_pack<true, false>(b, blocks) : launch_pack<false, false>(b, blocks);
  return MIC_OK;
}

// the query: one engine's launch, or the exchange of a table-sharded group.  Rank roll-up started on the slot's engine: the rows
// instantiation of the same kernel fills the slot's row buffer.  One engine: rows of the --extended width, so that a batch is handed
// back exactly when it is handed back without roll-up (a row that does not fit is a read of more than 64 targets, which the kernel
// flags anyway); a group: the summed rows, kGroupRowWords wide.
int query_batch(BatchCtx& b, mic_engine* const* group, size_t n_group, size_t owner) {
  Ingest* g = b.g; Slot& s = *b.s; const hipStream_t st = b.st; int rc;
  const MicRollup& ru = *mic_engine_rollup(b.e);
  const bool roll = b.roll = ru.on && ru.d_counts && ru.n_levels;
  if (roll && (rc = ensure_rollup_buffers(g, s, n_group == 1 ? std::min<uint32_t>(b.nt + 1, 65u) : kGroupRowWords))) return rc;
  if (n_group == 1) {
    MIC_TRY(hipMemsetAsync(s.d_flagged, 0, 4, st));
    MicQueryArgs qa;
    qa.t = b.t; qa.reads_ptr = s.d_rp; qa.cont = s.d_cont; qa.n_reads = b.n_reads; qa.row_words = roll ? s.ru_row_words : 0; qa.results = s.d_results;
    qa.rows = roll ? s.d_ru_rows : nullptr; qa.flagged = s.d_flagged; qa.flagged_cap = kFlaggedCapI;
    mic_crowd_attach(qa, s.d_crowd, g->max_reads / 4 + 64);
    MIC_TRY(mic_launch_query(qa, b.sc, b.ncu, st));
  } else {
    // table-sharded: all engines of the group probe the batch against their parts, the rows are summed read-range owned
    if ((rc = group_query(group, n_group, owner, g, s, b.n_reads, b.nb, b.k, roll ? s.d_ru_rows : nullptr))) return rc;
    MIC_TRY(hipSetDevice(b.dev));
  }
  return MIC_OK;
}

CsvArgs csv_args(const BatchCtx& b) {
  const Ingest* g = b.g; const Slot& s = *b.s; CsvArgs ca;
  ca.raw = s.d_raw; ca.name_s = s.rec.name_s; ca.name_len = s.rec.name_len; ca.length = s.rec.length; ca.results = s.d_results;
  ca.tnames = g->d_tnames; ca.tname_off = g->d_tname_off; ca.n_targets = g->n_targets; ca.n_reads = b.n_reads; ca.k = b.k; ca.paired = b.paired ? 1 : 0;
  return ca;
}

// the CSV line lengths, their scan and the batch's status word - or the status word alone
int csv_lengths(BatchCtx& b) {
  Ingest* g = b.g; Slot& s = *b.s; const hipStream_t st = b.st; const uint32_t n_reads = b.n_reads;
  const uint32_t cont_cap = (uint32_t)std::min<size_t>(g->cont_cap, 0xFFFFFFFFu);
  if (!b.no_csv) {
    csv_len_kernel<<<b.gr, 256, 0, st>>>(csv_args(b), s.d_line_len, s.d_hdr);
    size_t tb = s.tmp_bytes;
    MIC_TRY(hipcub::DeviceScan::ExclusiveSum(s.d_tmp, tb, s.d_line_len, s.d_line_off, (int)(n_reads + 1), st));
    csv_finish_kernel<<<1, 1, 0, st>>>(s.d_line_off, n_reads, s.d_flagged, s.d_rp, (uint32_t)std::min<size_t>(g->csv_cap, 0xFFFFFFFFu), cont_cap, s.d_hdr);
  } else {
    nocsv_status_kernel<<<(n_reads + 255) / 256, 256, 0, st>>>(s.d_results, s.rec.length, b.paired ? 1 : 0, b.k, n_reads, s.d_flagged, s.d_rp, cont_cap, s.d_hdr);
  }
  return MIC_OK;
}

// what is counted on the device for the slot's engine (the owner of a table-sharded batch): every kernel here adds nothing when the
// status word says that the batch goes back to the host path
int count_products(BatchCtx& b) {
  Slot& s = *b.s; const hipStream_t st = b.st; const uint32_t* status = s.d_hdr + H_STATUS;
  const uint32_t n_reads = b.n_reads, nt = b.nt, norm_sub = b.paired ? 1u : 0u; const int k = b.k;
  const MicAbund& ab = *mic_engine_abund(b.e);
  if (ab.on && ab.d_counts && ab.n_words == nt + 2)
    MIC_TRY(mic_launch_abund(s.d_results, s.rec.length, norm_sub, n_reads, k, nt, ab, ab.d_counts, status, st));
  if (b.roll) {
    const MicRollup& ru = *mic_engine_rollup(b.e);
    MIC_TRY(mic_launch_rollup(ru, s.d_ru_rows, s.ru_row_words, s.rec.length, norm_sub, n_reads, k, nt, ru.filter, s.d_rollup, nullptr, ru.d_counts, status, st));
    if (s.h_rollup) MIC_TRY(hipMemcpyAsync(s.h_rollup, s.d_rollup, (size_t)n_reads * MIC_ROLLUP_WORDS * 4, hipMemcpyDeviceToHost, st));
  }
  const MicDensity& dn = *mic_engine_density(b.e);      // score densities (mic_density_start)
  if (dn.on && dn.d_counts)
    MIC_TRY(mic_launch_density(s.d_results, s.rec.length, norm_sub, n_reads, k, nt, b.ncu, dn.d_counts, status, st));
  const MicKsketch& ks = *mic_engine_ksketch(b.e);      // k-mer sketches (mic_ksketch_start): a second probe pass over the reads that hit
  if (ks.on && ks.d_regs && ks.n_targets == nt)
    MIC_TRY(mic_launch_ksketch(b.t, b.sc, b.ncu, s.d_rp, s.d_cont, n_reads, s.d_results, nt, ks.d_regs, ks.d_hits, status, st));
  return MIC_OK;
}

// the tail of a product that goes to the host on the download stream: with a CSV, phase 3's wait for that stream covers the copy
int wait_down_without_csv(const BatchCtx& b) {
  if (b.no_csv) MIC_TRY(wait_stream(*b.s, b.down));
  return MIC_OK;
}

// read splitting (mic_split_start on the slot's engine, the owner of a table-sharded batch), behind the status check: class and
// length per record, one scan, the stable partition of the slot's text; then the classes asked for go to the slot's pinned buffer
int split_product(BatchCtx& b) {
  Slot& s = *b.s; const hipStream_t st = b.st; const MicSplit& sp = b.sp; const uint32_t n_reads = b.n_reads, nb = b.nb;
  int rc = ensure_split_buffers(b.g, s);
  if (rc) return rc;
  MIC_TRY(mic_launch_split(s.d_raw, nb, s.rec.name_s, 1u, s.d_results, s.rec.length, b.paired ? 1u : 0u, n_reads, b.k, b.nt, sp.filter, sp.which,
                           s.split_b, s.d_split, nullptr, st));
  MIC_TRY(hipMemcpyAsync(s.h_split_tot, s.split_b.d_off2 + n_reads, 8, hipMemcpyDeviceToHost, st));
  MIC_TRY(hipMemcpyAsync(s.h_split_tot + 1, s.split_b.d_ncls, 4, hipMemcpyDeviceToHost, st));
  MIC_TRY(wait_stream(s, st));
  const uint64_t n_cls = (uint32_t)s.h_split_tot[0], n_unc = s.h_split_tot[0] >> 32;      // bytes of the two classes
  if (n_cls + n_unc > (uint64_t)nb + 1)
    return mic_set_error(MIC_E_STATE, "split: %llu + %llu bytes from a text of %u", (unsigned long long)n_cls, (unsigned long long)n_unc, nb);
  const uint64_t lo = (sp.which & MIC_SPLIT_CLASSIFIED) ? 0 : n_cls, hi = (sp.which & MIC_SPLIT_UNCLASSIFIED) ? n_cls + n_unc : n_cls;
  if (hi > lo) MIC_TRY(hipMemcpyAsync(s.h_split + lo, s.d_split + lo, hi - lo, hipMemcpyDeviceToHost, b.down));   // (the partition is complete: the wait above)
  if ((rc = wait_down_without_csv(b))) return rc;
  s.split_which = sp.which; s.split_valid = true;
  return MIC_OK;
}

// hit maps (mic_hitmap_start on the slot's engine), behind the status check like the split: words per read, their exclusive sum,
// the words; line lengths, their exclusive sum, the lines.  The host reads the word total and later the text total (8 bytes
// each) and grows the buffer that is too small before the pass that fills it.
int hitmap_product(BatchCtx& b) {
  Ingest* g = b.g; Slot& s = *b.s; const hipStream_t st = b.st;
  const MicTable& t = b.t; const int sc = b.sc, ncu = b.ncu; const uint32_t n_reads = b.n_reads, nt = b.nt;
  int rc = ensure_hitmap_buffers(g, s, 0, 0);
  if (rc) return rc;
  MIC_TRY(mic_launch_hitmap(t, sc, ncu, s.d_rp, s.d_cont, n_reads, s.d_results, nt, nullptr, s.d_hm_cnt, false, st));
  MIC_TRY(mic_hitmap_scan(s.d_hm_tmp, s.hm_tmp_bytes, s.d_hm_cnt, s.d_hm_off, (size_t)n_reads + 1, st));
  s.h_hm_tot[0] = 0;
  MIC_TRY(hipMemcpyAsync(s.h_hm_tot, s.d_hm_off + n_reads, 4, hipMemcpyDeviceToHost, st));
  MIC_TRY(wait_stream(s, st));
  const size_t n_words = (size_t)s.h_hm_tot[0];
  if ((rc = ensure_hitmap_buffers(g, s, n_words, 0))) return rc;
  MIC_TRY(mic_launch_hitmap(t, sc, ncu, s.d_rp, s.d_cont, n_reads, s.d_results, nt, s.d_hm_off, s.d_hm_words, true, st));
  HitmapTextArgs ha;
  ha.raw = s.d_raw; ha.name_s = s.rec.name_s; ha.name_len = s.rec.name_len; ha.offsets = s.d_hm_off; ha.words = s.d_hm_words;
  ha.tnames = g->d_tnames; ha.tname_off = g->d_tname_off; ha.n_targets = g->n_targets; ha.n_reads = n_reads;
  KrakenTextArgs ka;                          // the Kraken format (mic_kraken_start): the same place, buffers and scan, another pair of text kernels
  if (b.hm.kraken) {
    ka.h = ha; ka.results = s.d_results; ka.length = s.rec.length; ka.norm_sub = b.paired ? 1u : 0u; ka.k = b.k; ka.filter = b.hm.filter;
    kraken_len_kernel<<<b.gr, 256, 0, st>>>(ka, s.d_hm_len);
  } else {
    hitmap_len_kernel<<<b.gr, 256, 0, st>>>(ha, s.d_hm_len);
  }
  size_t tb = s.hm_tmp_bytes;
  MIC_TRY(hipcub::DeviceScan::ExclusiveSum(s.d_hm_tmp, tb, s.d_hm_len, s.d_hm_loff, (int)(n_reads + 1), st));
  MIC_TRY(hipMemcpyAsync(s.h_hm_tot + 1, s.d_hm_loff + n_reads, 8, hipMemcpyDeviceToHost, st));
  MIC_TRY(wait_stream(s, st));
  const size_t n_text = (size_t)s.h_hm_tot[1];
  if ((rc = ensure_hitmap_buffers(g, s, 0, n_text))) return rc;
  if (b.hm.kraken) kraken_fmt_kernel<<<(n_reads + 255) / 256, 256, 0, st>>>(ka, s.d_hm_loff, s.d_hm_text);
  else hitmap_fmt_kernel<<<(n_reads + 255) / 256, 256, 0, st>>>(ha, s.d_hm_loff, s.d_hm_text);
  MIC_TRY(hipGetLastError());
  MIC_TRY(hipEventRecord(s.ev_k, st));
  MIC_TRY(hipStreamWaitEvent(b.down, s.ev_k, 0));
  MIC_TRY(hipMemcpyAsync(s.h_hm_text, s.d_hm_text, n_text, hipMemcpyDeviceToHost, b.down));
  if ((rc = wait_down_without_csv(b))) return rc;
  s.hm_valid = true; s.hm_kraken = b.hm.kraken;
  return MIC_OK;
}

// phase 3: CSV text -> host, and the batch's last wait
int csv_to_host(BatchCtx& b, uint32_t csv_bytes) {
  Slot& s = *b.s; const hipStream_t st = b.st, down = b.down;
  csv_fmt_kernel<<<(b.n_reads + 255) / 256, 256, 0, st>>>(csv_args(b), s.d_line_off, s.d_csv);
  MIC_TRY(hipGetLastError());
  MIC_TRY(hipEventRecord(s.ev_k, st));
  MIC_TRY(hipStreamWaitEvent(down, s.ev_k, 0));
  MIC_TRY(hipMemcpyAsync(s.h_csv, s.d_csv, csv_bytes, hipMemcpyDeviceToHost, down));
  if (b.g->want_results) MIC_TRY(hipMemcpyAsync(s.h_results, s.d_results, (size_t)b.n_reads * 32, hipMemcpyDeviceToHost, down));
  MIC_TRY(wait_stream(s, down));
  return MIC_OK;
}

}  // namespace

int mic_ingest_slot_text(mic_engine* e, size_t slot_id, MicSlotText* out) {
  Ingest* g = ingest_with_slot(e, slot_id); if (!g) return MIC_E_STATE;
  *out = {g->slots[slot_id].d_raw, g->slots[slot_id].stream, g->max_bytes, g->device};
  return MIC_OK;
}

extern "C" {

int mic_ingest_classify_group(mic_engine* const* group, size_t n_group, size_t owner, size_t slot_id, size_t n_bytes, int flags,
                              mic_ingest_result* out) {
  BatchCtx b;
  int rc = begin_batch(group, n_group, owner, slot_id, n_bytes, flags, out, b);
  if (rc || out->status) return rc;
  static const bool timing = getenv("MIC_INGEST_TIMING") != nullptr;
  const double t0 = timing ? now_s() : 0;
  if ((rc = index_records(b, out)) || out->status) return rc;
  const double t1 = timing ? now_s() : 0;
  // ---- phase 2: records -> packed reads -> query -> CSV line lengths -> what is counted on the device
  if ((rc = pack_reads(b)) || (rc = query_batch(b, group, n_group, owner)) || (rc = csv_lengths(b)) || (rc = count_products(b))) return rc;
  Ingest* g = b.g; Slot& s = *b.s; const uint32_t n_reads = b.n_reads;
  if (b.no_csv && g->want_results) MIC_TRY(hipMemcpyAsync(s.h_results, s.d_results, (size_t)n_reads * 32, hipMemcpyDeviceToHost, b.st));
  MIC_TRY(hipMemcpyAsync(s.h_hdr, s.d_hdr, H_WORDS * 4, hipMemcpyDeviceToHost, b.st));
  MIC_TRY(wait_stream(s, b.st));
  const double t2 = timing ? now_s() : 0;
  if (n_group > 1) group_harvest(g, s, n_reads);
  s.n_reads = n_reads; s.cont_used = s.h_hdr[H_CONT];
  const uint32_t csv_bytes = s.h_hdr[H_CSV_BYTES];
  uint32_t status = s.h_hdr[H_STATUS];
  if (csv_bytes > g->csv_cap || s.h_hdr[H_CONT] > g->cont_cap) status |= MIC_INGEST_TOO_MANY;
  if (status) { out->status = MIC_INGEST_FALLBACK | status; return MIC_OK; }
  s.ru_valid = b.roll && s.h_rollup;
  // ---- the products behind the status check, then phase 3
  if (b.sp.on && (rc = split_product(b))) return rc;
  if (b.hitmaps && (rc = hitmap_product(b))) return rc;
  if (!b.no_csv && (rc = csv_to_host(b, csv_bytes))) return rc;
  out->n_reads = n_reads; out->csv_bytes = b.no_csv ? 0 : csv_bytes; out->csv = s.h_csv; out->results = g->want_results ? s.h_results : nullptr;
  out->status = MIC_INGEST_OK;
  if (timing) {
    char csv_us[32] = "no csv";
    if (!b.no_csv) snprintf(csv_us, sizeof(csv_us), "csv %.0f us", (now_s() - t2) * 1e6);
    fprintf(stderr, "[ingest] slot %zu: %u bytes, %u reads: lines %.0f us, pack+query+%s %.0f us, %s\n", slot_id, b.nb, n_reads,
            (t1 - t0) * 1e6, b.no_csv ? "count" : "lengths", (t2 - t1) * 1e6, csv_us);
  }
  return MIC_OK;
}

int mic_ingest_set_min_quality(mic_engine* e, uint32_t threshold_byte) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  if (threshold_byte > 255) return mic_set_error(MIC_E_INVALID, "a threshold byte is 0 (off) .. 255, got %u", threshold_byte);
  *mic_engine_min_quality(e) = threshold_byte;
  return MIC_OK;
}

int mic_ingest_set_low_complexity(mic_engine* e, uint32_t level) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  if (level > MIC_LOWC_MAX_LEVEL) return mic_set_error(MIC_E_INVALID, "a low-complexity level is 0 (off) .. %u, got %u", MIC_LOWC_MAX_LEVEL, level);
  *mic_engine_low_complexity(e) = level;
  return MIC_OK;
}

int mic_ingest_rollup_rows(mic_engine* e, size_t slot_id, const uint32_t** rollup, uint64_t* n_reads) {
  if (!e || !rollup || !n_reads) return mic_set_error(MIC_E_INVALID, "null argument");
  Ingest* g = ingest_with_slot(e, slot_id); if (!g) return MIC_E_STATE;
  const Slot& s = g->slots[slot_id];
  if (!s.ru_valid) return mic_set_error(MIC_E_STATE, "the slot's last batch left no roll-up rows (mic_rollup_start, want_results, MIC_INGEST_OK)");
  *rollup = s.h_rollup; *n_reads = s.n_reads;
  return MIC_OK;
}

int mic_ingest_split_text(mic_engine* e, size_t slot_id, const uint8_t** classified, uint64_t* classified_bytes, uint64_t* n_classified,
                          const uint8_t** unclassified, uint64_t* unclassified_bytes, uint64_t* n_unclassified) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  Ingest* g = ingest_with_slot(e, slot_id); if (!g) return MIC_E_STATE;
  const Slot& s = g->slots[slot_id];
  if (!s.split_valid) return mic_set_error(MIC_E_STATE, "the slot's last batch left no split text (mic_split_start, MIC_INGEST_OK)");
  const uint64_t a = (uint32_t)s.h_split_tot[0], b = s.h_split_tot[0] >> 32, nc = s.h_split_tot[1];
  const bool wc = (s.split_which & MIC_SPLIT_CLASSIFIED) != 0, wu = (s.split_which & MIC_SPLIT_UNCLASSIFIED) != 0;
  if (classified) *classified = wc ? s.h_split : nullptr;
  if (classified_bytes) *classified_bytes = wc ? a : 0;
  if (n_classified) *n_classified = nc;
  if (unclassified) *unclassified = wu ? s.h_split + a : nullptr;
  if (unclassified_bytes) *unclassified_bytes = wu ? b : 0;
  if (n_unclassified) *n_unclassified = s.n_reads - nc;
  return MIC_OK;
}

int mic_ingest_hitmap_text(mic_engine* e, size_t slot_id, const uint8_t** text, uint64_t* bytes) {
  if (!e || !text || !bytes) return mic_set_error(MIC_E_INVALID, "null argument");
  Ingest* g = ingest_with_slot(e, slot_id); if (!g) return MIC_E_STATE;
  const Slot& s = g->slots[slot_id];
  if (mic_engine_hitmap(e)->kraken || (s.hm_valid && s.hm_kraken))
    return mic_set_error(MIC_E_STATE, "the Kraken format is on: the slot's text is mic_ingest_kraken_text's");
  if (!s.hm_valid) return mic_set_error(MIC_E_STATE, "the slot's last batch left no hit-map text (mic_hitmap_start, MIC_INGEST_OK)");
  *text = (const uint8_t*)s.h_hm_text; *bytes = s.h_hm_tot[1];
  return MIC_OK;
}

int mic_ingest_kraken_text(mic_engine* e, size_t slot_id, const uint8_t** text, uint64_t* bytes) {
  if (!e || !text || !bytes) return mic_set_error(MIC_E_INVALID, "null argument");
  Ingest* g = ingest_with_slot(e, slot_id); if (!g) return MIC_E_STATE;
  const Slot& s = g->slots[slot_id];
  const MicHitmap& hm = *mic_engine_hitmap(e);
  if ((hm.on && !hm.kraken) || (s.hm_valid && !s.hm_kraken))
    return mic_set_error(MIC_E_STATE, "the hit-map format is on: the slot's text is mic_ingest_hitmap_text's");
  if (!s.hm_valid) return mic_set_error(MIC_E_STATE, "the slot's last batch left no Kraken text (mic_kraken_start, MIC_INGEST_OK)");
  *text = (const uint8_t*)s.h_hm_text; *bytes = s.h_hm_tot[1];
  return MIC_OK;
}

int mic_ingest_fetch_packed(mic_engine* e, size_t slot_id, uint32_t* reads_pointer, size_t rp_cap, uint16_t* containers, size_t cont_cap,
                            uint64_t* n_reads, uint64_t* n_containers) {
  if (!e) return mic_set_error(MIC_E_INVALID, "null engine");
  Ingest* g = ingest_with_slot(e, slot_id); if (!g) return MIC_E_STATE;
  Slot& s = g->slots[slot_id];
  if (n_reads) *n_reads = s.n_reads;
  if (n_containers) *n_containers = s.cont_used;
  if (reads_pointer) {
    if (rp_cap < (size_t)s.n_reads + 1) return mic_set_error(MIC_E_INVALID, "reads_pointer capacity too small");
    MIC_TRY(hipMemcpy(reads_pointer, s.d_rp, ((size_t)s.n_reads + 1) * 4, hipMemcpyDeviceToHost));
  }
  if (containers) {
    if (cont_cap < s.cont_used) return mic_set_error(MIC_E_INVALID, "containers capacity too small");
    MIC_TRY(hipMemcpy(containers, s.d_cont, (size_t)s.cont_used * 2, hipMemcpyDeviceToHost));
  }
  return MIC_OK;
}

int mic_ingest_fetch_group_rows(mic_engine* owner, size_t slot_id, size_t part, uint32_t* rows, size_t cap_words, uint64_t* n_reads,
                                uint32_t* row_words) {
  if (!owner) return mic_set_error(MIC_E_INVALID, "null engine");
  Ingest* g = ingest_with_slot(owner, slot_id); if (!g) return MIC_E_STATE;
  Slot& s = g->slots[slot_id];
  if (part >= s.peers.size()) return mic_set_error(MIC_E_STATE, "the slot's last batch was not table-sharded over %zu parts", part + 1);
  if (n_reads) *n_reads = s.n_reads;
  if (row_words) *row_words = kGroupRowWords;
  if (rows) {
    const size_t words = (size_t)s.n_reads * kGroupRowWords;
    if (cap_words < words) return mic_set_error(MIC_E_INVALID, "rows capacity too small");
    MIC_TRY(hipSetDevice(s.peers[part].device));
    MIC_TRY(hipMemcpy(rows, s.peers[part].d_rows, words * 4, hipMemcpyDeviceToHost));
    MIC_TRY(hipSetDevice(g->device));
  }
  return MIC_OK;
}

int mic_ingest_group_stats(mic_engine* owner, double* out, size_t cap) {
  if (!owner || !out || cap < MIC_GROUP_STATS_FIELDS) return mic_set_error(MIC_E_INVALID, "bad argument");
  Ingest* g = (Ingest*)*mic_engine_ingest_slot(owner);
  if (!g) return mic_set_error(MIC_E_STATE, "ingest slots are not allocated");
  std::lock_guard<std::mutex> lk(g->gstats.mu);
  const GroupStats& G = g->gstats;
  const double v[MIC_GROUP_STATS_FIELDS] = {(double)G.batches, (double)G.reads, (double)G.fan_bytes, G.fan_ms_sum, G.fan_ms_max, G.kernel_ms_sum,
                                            G.kernel_ms_max, (double)G.x_bytes, G.x_ms_sum, G.x_ms_max};
  for (size_t i = 0; i < MIC_GROUP_STATS_FIELDS; ++i) out[i] = v[i];
  return (int)MIC_GROUP_STATS_FIELDS;
}

// host build of the device formatter (tests pin it against the C library's "%g")
int mic_format_ratio_g(uint32_t num, uint32_t den, char* out16) {
  if (!out16 || den == 0 || num == 0 || num > den) return MIC_E_INVALID;
  const int n = mic_fmt_g_unit((double)num / (double)den, out16);
  out16[n] = 0;
  return n;
}

}  // extern "C"
