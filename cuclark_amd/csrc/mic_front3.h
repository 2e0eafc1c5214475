// mic_front3.h - the front half of query_kernel_r for k = 31, m = 20 with THREE t-mers per lane (round 8), as index arithmetic
// on plain values: which window dwords, which funnel shift, the order keys, the nine-minimum combination, the sampled position,
// the order of the run records.  The kernel (mic_kernels.hip: sampled_positions3, front) and the host model below are written with the same
// functions; plain C++, so a stand-alone program checks the model against the brute force (tests/test_front_triples.py).
//
// t = 8, W = 24 t-mers per k-mer = 8 x 3: lane a (0 .. 63) owns the t-mers at chunk positions 3a, 3a+1, 3a+2 and the k-mers that
// start there.  The window of k-mer 3a is the triples of lanes a .. a+7; those of k-mers 3a+1 and 3a+2 are the same without the
// first one or two t-mers of lane a, with the first one or two of lane a+8.
#ifndef MIC_FRONT3_H
#define MIC_FRONT3_H

#include <stdint.h>

#if defined(__HIPCC__)
#define F3_FN __host__ __device__ __forceinline__
#else
#define F3_FN static inline
#endif

#define F3_K 31
#define F3_M 20
#define F3_T 8                          /* s_tlen(31, 20) */
#define F3_WIN (F3_K - F3_T + 1)        /* 24 t-mers per k-mer */
#define F3_WM (F3_K - F3_M + 1)         /* 12 m-mers per k-mer */

// Nucleotides 3a .. 3a+15 of the chunk (nucleotide 3a on top) are one funnel shift of window dwords f3_dword(a) and the next; a
// window dword holds 16 nucleotides, the first on top.  The dword is the one of nucleotide 3a - 1, so the shift stays below 32;
// lane 0 asks for dword -1 (ds_bpermute wraps to lane 63) and shifts all of it out.
F3_FN int f3_dword(int a) { return (3 * a - 1) >> 4; }
F3_FN uint32_t f3_shift(int a) { return 30u - 2u * (uint32_t)((3 * a - 1) & 15); }
F3_FN uint32_t f3_funnel(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh); }   // v_alignbit_b32

// t-mer j (0 .. 2) of the lane out of that word: 16 bits, 2 j bits below the top
F3_FN uint32_t f3_tmer(uint32_t X, int j) { return (X << (2 * j)) >> 16; }
// The reverse complements of the three t-mers are substrings of ONE reverse complement, that of the 10 nucleotides on top of X:
// Y = comp(n9) .. comp(n0) in bits 19 .. 0, and rc(t-mer j) = comp(n[j+7]) .. comp(n[j]) = bits 2j+15 .. 2j of it.
F3_FN uint32_t f3_rc10(uint32_t X) {
  uint32_t r = 0;
  for (int i = 0; i < 10; ++i) r |= (3u - ((X >> (30 - 2 * i)) & 3u)) << (2 * i);
  return r;
}
F3_FN uint32_t f3_tmer_rc(uint32_t Y, int j) { return (Y >> (2 * j)) & 0xFFFFu; }
// order key of the t-mer at chunk position pos: s_torder24 (mic_device.h) of its value, the position in the low five bits
F3_FN uint32_t f3_key(uint32_t tv, uint32_t pos) { return (((tv & 0xFFFFFFu) * 0x9E3779u + 0x27D4EB2Fu) & ~31u) | (pos & 31u); }

F3_FN uint32_t f3_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
F3_FN uint32_t f3_min3(uint32_t a, uint32_t b, uint32_t c) { return f3_min(f3_min(a, b), c); }
// The minimum over [i, i + 24) for the lane's three k-mers.  With T = min3(k0, k1, k2), e12 = min(k1, k2), e01 = min(k0, k1) of
// every lane, towards higher lanes: x1 = T[a+1], m2 = min(T, x1); y = m2[a+2], m4 = min(m2, y); z = m4[a+4]; k0n = k0[a+8],
// e01n = e01[a+8].  Nine minima and five fetches in all.  A lane number past 63 wraps: those lanes own no k-mer of a chunk.
F3_FN void f3_combine(uint32_t k2, uint32_t e12, uint32_t m4, uint32_t x1, uint32_t y, uint32_t z, uint32_t k0n, uint32_t e01n,
                      uint32_t& r0, uint32_t& r1, uint32_t& r2) {
  r0 = f3_min(m4, z);                                 // triples a .. a+7
  const uint32_t M7 = f3_min3(x1, y, z);              // triples a+1 .. a+7
  r1 = f3_min3(e12, M7, k0n);
  r2 = f3_min3(k2, M7, e01n);
}
// chunk position of the sampled m-mer of the k-mer at pos, r its window's minimal key: the minimal t-mer sits at i = (r - pos) & 31
// inside the k-mer (0 .. 23), the sampled m-mer at i mod 12
F3_FN uint32_t f3_sampled(uint32_t r, uint32_t pos) {
  const uint32_t d = (r - pos) & 31u, e = d - (uint32_t)F3_WM;
  return pos + f3_min(d, e);
}
// Run records, in k-mer order: a k-mer leads a run when its sampled position is not that of the k-mer before it; k-mers past
// the chunk's n_act count as one position no k-mer samples, so k-mer n_act (it always exists: 3 x 64 > 128) leads the closing
// record.  Record = sampled position | first k-mer << 8; of the closing record only the k-mer is ever read, its low byte is
// whatever the lane computed (below 256: a position is at most 191 + 11).  The record of element j of a lane goes to slot
// (leaders of all elements in lower lanes) + (leaders among the lane's own earlier elements).
F3_FN uint32_t f3_rank(uint32_t below0, uint32_t below1, uint32_t below2, bool f0, bool f1, int j) {
  return below0 + below1 + below2 + (j > 0 && f0 ? 1u : 0u) + (j > 1 && f1 ? 1u : 0u);
}
F3_FN uint16_t f3_record(uint32_t q, uint32_t pos) { return (uint16_t)(q | (pos << 8)); }

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole front half of one chunk on plain arrays, lane by lane as the kernel does it.  wd: the 64 window dwords (whatever the
// lanes past the part hold); canon: one-strand table; q[3a + j]: sampled position of k-mer 3a + j or ~0; rec: the records;
// returns the number of runs (rec[runs] is the closing record).  No key is masked: every window is exactly its 24 t-mers, so
// what lies past the part reaches only k-mers >= n_act.
static inline uint32_t f3_model(const uint32_t wd[64], uint32_t n_act, bool canon, uint32_t q[192], uint16_t rec[132]) {
  uint32_t s[192];
  uint32_t k0[64], k2[64], T[64], e12[64], e01[64], m2[64], m4[64];
  for (int a = 0; a < 64; ++a) {
    const int D = f3_dword(a);
    const uint32_t X = f3_funnel(wd[D & 63], wd[(D + 1) & 63], f3_shift(a)), Y = f3_rc10(X);
    uint32_t kk[3];
    for (int j = 0; j < 3; ++j) {
      uint32_t tv = f3_tmer(X, j);
      if (canon) tv = f3_min(tv, f3_tmer_rc(Y, j));
      kk[j] = f3_key(tv, (uint32_t)(3 * a + j));
    }
    k0[a] = kk[0]; k2[a] = kk[2];
    T[a] = f3_min3(kk[0], kk[1], kk[2]); e12[a] = f3_min(kk[1], kk[2]); e01[a] = f3_min(kk[0], kk[1]);
  }
  for (int a = 0; a < 64; ++a) m2[a] = f3_min(T[a], T[(a + 1) & 63]);
  for (int a = 0; a < 64; ++a) m4[a] = f3_min(m2[a], m2[(a + 2) & 63]);
  bool f[192];
  for (int a = 0; a < 64; ++a) {
    uint32_t r[3];
    f3_combine(k2[a], e12[a], m4[a], T[(a + 1) & 63], m2[(a + 2) & 63], m4[(a + 4) & 63], k0[(a + 8) & 63], e01[(a + 8) & 63], r[0], r[1], r[2]);
    for (int j = 0; j < 3; ++j) {
      const uint32_t pos = (uint32_t)(3 * a + j);
      s[pos] = f3_sampled(r[j], pos);
      q[pos] = pos < n_act ? s[pos] : ~0u;
    }
  }
  for (int i = 0; i < 192; ++i) f[i] = i == 0 || q[i] != q[i - 1];
  uint32_t below[3] = {0, 0, 0}, total = 0;
  for (int a = 0; a < 64; ++a) {
    for (int j = 0; j < 3; ++j)
      if (f[3 * a + j]) { rec[f3_rank(below[0], below[1], below[2], f[3 * a], f[3 * a + 1], j)] = f3_record(s[3 * a + j], (uint32_t)(3 * a + j)); ++total; }
    for (int j = 0; j < 3; ++j) below[j] += f[3 * a + j];
  }
  return total - 1u;
}
#endif

#endif
