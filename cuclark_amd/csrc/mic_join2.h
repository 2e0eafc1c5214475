// mic_join2.h - a read of TWO parts (one N inside it) on the pipelined road of query_kernel_r (round 9), as index arithmetic on
// plain values: does the read qualify, where its second part sits in the read-ahead entry, the window dwords of the two parts joined,
// the k-mer positions of the junction.  The kernel (mic_kernels.hip: step, front) and the host model below are written with the same
// functions; plain C++, so a stand-alone program checks the model against a brute-force concatenation (tests/test_join2.py).
//
// The read-ahead entry: 12 aligned dwords = 24 containers (u16) from the read's first length slot on; the slot is u16 `odd` of the
// entry (0 or 1: which half of its dword), container u16 i is the low (i even) or high half of dword i / 2.  A part is a length
// slot and ceil(len / 8) containers of 8 nucleotides, the first on top; window dword j of a part holds its nucleotides 16 j .. 16 j
// + 15, the first on top.  Part 2 starts on a container of its own, so in the joined window - the nucleotides of part 1 followed at
// once by those of part 2 - it is shifted by len1 mod 16 nucleotides and sits on either half of the entry's dwords.
// The k-mer positions [len1 - k + 1, len1) of the joined window span the junction: they are no k-mers of the read.
#ifndef MIC_JOIN2_H
#define MIC_JOIN2_H

#include <stdint.h>

#if defined(__HIPCC__)
#define J2_FN __host__ __device__ __forceinline__
#else
#define J2_FN static inline
#endif

#define J2_ENTRY_U16 24                 /* containers of a read-ahead entry */
#define J2_CHUNK 128                    /* k-mer positions of a chunk */

struct J2Shape {
  uint32_t ok;                          // the read takes the joined road
  uint32_t len1, len2;                  // nucleotides of the two parts
  uint32_t b2;                          // u16 of the entry where part 2's first container sits
  uint32_t n_act;                       // k-mer positions of the joined window: len1 + len2 - k + 1
  uint32_t g0, g1;                      // [g0, g1): the positions that span the junction
};

J2_FN uint32_t j2_half(uint32_t dword, uint32_t u) { return (u & 1u) ? dword >> 16 : dword & 0xFFFFu; }

// The u16 of the entry that holds the slot behind part 1 - the length of a second part, or the 0 that ends a read of one part in a
// terminated format -, or J2_NONE: the first part is no single chunk, the read ends behind it, or the slot lies behind the entry.
//   plen0: the first length slot; span: pe - pp, containers from the read's first length slot to its end as reads_ptr has it
#define J2_NONE 0xFFFFFFFFu
J2_FN uint32_t j2_slot2(uint32_t plen0, uint32_t span, uint32_t odd, uint32_t k) {
  if (plen0 - k >= (uint32_t)J2_CHUNK) return J2_NONE;             // k <= len1 < k + 128 by the unsigned wrap
  const uint32_t h2 = 1u + (plen0 + 7u) / 8u;                      // part 2's length slot, containers from the read's first slot
  return h2 < span && h2 + odd < (uint32_t)J2_ENTRY_U16 ? h2 + odd : J2_NONE;
}
// The tests a read passes, in the order the kernel makes them (every LDS read behind the test that keeps it inside the entry).
//   slot2: what u16 j2_slot2(..) of the entry holds, or anything when that is J2_NONE; at(u): u16 `u` of the entry (u < 24).
// A read qualifies with exactly two parts of at least k nucleotides each, everything up to what ends it inside the entry - the
// read's end itself (the packer's format: span) or a 0 where a third length slot would be (terminated formats) - and at most 128
// k-mer positions joined.
template <typename At>
J2_FN J2Shape j2_shape(uint32_t plen0, uint32_t slot2, uint32_t span, uint32_t odd, uint32_t k, At&& at) {
  J2Shape s;
  s.ok = 0; s.len1 = plen0; s.len2 = 0; s.b2 = 0; s.n_act = 0; s.g0 = 0; s.g1 = 0;
  if (j2_slot2(plen0, span, odd, k) == J2_NONE) return s;
  const uint32_t h2 = 1u + (plen0 + 7u) / 8u;
  const uint32_t len2 = slot2;
  if (len2 - k >= (uint32_t)J2_CHUNK) return s;
  const uint32_t end = h2 + 1u + (len2 + 7u) / 8u;                 // one past part 2's last container
  if (end + odd > (uint32_t)J2_ENTRY_U16 || end > span) return s;
  if (end < span) {
    if (end + odd >= (uint32_t)J2_ENTRY_U16) return s;
    if (at(end + odd) != 0u) return s;
  }
  const uint32_t n_act = plen0 + len2 - k + 1u;
  if (n_act > (uint32_t)J2_CHUNK) return s;
  s.ok = 1; s.len2 = len2; s.b2 = h2 + 1u + odd; s.n_act = n_act; s.g0 = plen0 - k + 1u; s.g1 = plen0;
  return s;
}

// Window dword j (0 .. 11) of the joined read.  w1: window dword j of part 1 as the one-part road takes it out of the entry
// (whatever it holds behind the part); the nucleotides of part 2 come out of entry dwords j2_dword(..) and the next.
//   t = 16 j - len1: the nucleotide of part 2 the dword starts with (negative: the dword starts in part 1); no further down than -16,
//   where nothing of part 2 is taken.  The entry read as one string of nucleotides, 16 per dword, part 2 starts at nucleotide 8 b2:
//   the dword's 16 nucleotides of part 2 start at nucleotide e = 8 b2 + t of the entry (>= 8 b2 - 16), in dword e / 16.
J2_FN int j2_t(uint32_t j, uint32_t len1) { const int t = 16 * (int)j - (int)len1; return t < -16 ? -16 : t; }
J2_FN uint32_t j2_nt(uint32_t j, uint32_t len1, uint32_t b2) { return (uint32_t)(8 * (int)b2 + j2_t(j, len1)); }
J2_FN uint32_t j2_dword(uint32_t j, uint32_t len1, uint32_t b2) { return j2_nt(j, len1, b2) >> 4; }
J2_FN uint32_t j2_window(uint32_t w1, uint32_t d0, uint32_t d1, uint32_t j, uint32_t len1, uint32_t b2) {
  // the two dwords with their containers in reading order (the lower address on top), then 32 bits from nucleotide e mod 16 on
  const uint64_t z = ((uint64_t)((d0 << 16) | (d0 >> 16)) << 32) | ((d1 << 16) | (d1 >> 16));
  const uint32_t p = (uint32_t)((z << (2u * (j2_nt(j, len1, b2) & 15u))) >> 32);
  // the first r nucleotides of the dword are part 1's: r = -t, 16: all of it (t stops there), 0 or less: none
  const int r = -j2_t(j, len1);
  const uint32_t m = (uint32_t)(0xFFFFFFFFull >> (2 * (r < 0 ? 0 : r)));
  return (w1 & ~m) | (p & m);
}

// Position bits of the order keys.  Ties between t-mers are resolved by the position inside the PART modulo 32 (mic_device.h:
// s_probe_read), so a t-mer of part 2 - joined position pos >= len1 - carries pos - len1.  The lanes of the front half own several
// positions; j2_part_offset(first, last, len1) is what a lane subtracts from all of them: len1 when its LAST position is in part 2.
// Its positions in front of len1 are then wrong by len1, and harmless: a t-mer at len1 - 7 or later spans the junction, every window
// that holds one belongs to a k-mer of [g0, g1), and so does every k-mer the lane owns in front of len1 (last - first < k - 1).
J2_FN uint32_t j2_part_offset(uint32_t last, uint32_t len1) { return last >= len1 ? len1 : 0u; }
// is k-mer position pos one of the read?  (pos < n_act and outside [g0, g1); g1 - g0 = k - 1)
J2_FN bool j2_is_kmer(uint32_t pos, uint32_t n_act, uint32_t g0, uint32_t k) { return pos < n_act && pos - g0 >= k - 1u; }

#if !defined(__HIP_DEVICE_COMPILE__)
// The joined window of a read-ahead entry on plain arrays, lane by lane as the kernel does it.  entry: 64 dwords (whatever lies
// behind the read); w1 as the one-part road computes it (mic_kernels.hip: ahead_word).
static inline uint32_t j2_model_w1(const uint32_t entry[64], uint32_t odd, uint32_t j) {
  const uint32_t raw = entry[j & 63u], up = entry[(j + 1u) & 63u];
  return odd ? (up << 16) | (up >> 16) : (raw & 0xFFFF0000u) | (up & 0xFFFFu);
}
static inline void j2_model(const uint32_t entry[64], uint32_t odd, const J2Shape& s, uint32_t wd[12]) {
  for (uint32_t j = 0; j < 12; ++j) {
    const uint32_t d = j2_dword(j, s.len1, s.b2);
    wd[j] = j2_window(j2_model_w1(entry, odd, j), entry[d & 63u], entry[(d + 1u) & 63u], j, s.len1, s.b2);
  }
}
#endif

#endif
