// join2_check - the joined window of a two-part read (cuclark_amd/csrc/mic_join2.h: j2_shape, j2_model) against a brute-force
// concatenation of the two parts' nucleotides, stand-alone (tests/test_join2.py builds it with ASan + UBSan).
//   join2_check [seed]      exit status 0 and a line of counts, or the first difference and status 1
// Per k in 31 / 27 / 32: every len1 from k to 128 (len1 mod 16 = 0 .. 15 among them), len2 from k - 1 (a short part: refused) over every
// container count that the entry can hold and one more, both alignments of the entry, the packer's format (the read ends behind
// part 2) and the terminated one (a 0 follows), a third part, what lies behind the read random.  Checked: whether the read qualifies,
// every nucleotide of every window dword, the junction's k-mer positions, and the position bits a lane's t-mers carry.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mic_join2.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}

static void put_part(std::vector<uint16_t>& s, const std::vector<uint8_t>& nt) {
  s.push_back((uint16_t)nt.size());
  for (size_t i = 0; i < nt.size(); i += 8) {
    uint32_t c = 0;
    for (size_t j = 0; j < 8; ++j) c = c << 2 | (i + j < nt.size() ? nt[i + j] : 0u);
    s.push_back((uint16_t)c);
  }
}

enum { PACKER, TERMINATED, THIRD_PART_PACKER, THIRD_PART_TERMINATED, N_FORMATS };

int main(int argc, char** argv) {
  if (argc > 1) rng_state ^= strtoull(argv[1], nullptr, 10) * 0xD1342543DE82EF95ull;
  long cases = 0, joined = 0, dwords = 0;
  const int ks[3] = {31, 27, 32}, ts[3] = {8, 12, 7};
  for (int ki = 0; ki < 3; ++ki) {
    const uint32_t k = (uint32_t)ks[ki], tl = (uint32_t)ts[ki];
    for (uint32_t len1 = k; len1 <= 128; ++len1)
      for (uint32_t len2 = k - 1; len2 <= 136; ++len2)
        for (uint32_t odd = 0; odd < 2; ++odd)
          for (int fmt = 0; fmt < N_FORMATS; ++fmt) {
            if (len2 > k + 2 && len2 % 8 > 1 && len1 + len2 - k + 1 < 126 && rnd() % 4) continue;      // (thinned where nothing changes)
            std::vector<uint8_t> n1(len1), n2(len2), n3(40);
            for (auto& x : n1) x = rnd() & 3;
            for (auto& x : n2) x = rnd() & 3;
            for (auto& x : n3) x = rnd() & 3;
            std::vector<uint16_t> s;
            put_part(s, n1); put_part(s, n2);
            const uint32_t used = (uint32_t)s.size();                  // containers of the two parts with their length slots
            if (fmt == THIRD_PART_PACKER || fmt == THIRD_PART_TERMINATED) put_part(s, n3);
            uint32_t span = (uint32_t)s.size();
            if (fmt == TERMINATED || fmt == THIRD_PART_TERMINATED) { s.push_back(0); span = (uint32_t)s.size() + 3; }
            // the entry: the read from u16 `odd` on, random behind it (the next read, or whatever the memory holds: never a 0 that
            // would pass for a terminator by accident where the read goes on)
            uint32_t entry[64];
            for (uint32_t u = 0; u < 128; ++u) {
              uint16_t v = (uint16_t)(rnd() | 1u);
              if (u >= odd && u - odd < s.size()) v = s[u - odd];
              if (u >= J2_ENTRY_U16) v = (uint16_t)(rnd() | 1u);       // what the entry's 12 dwords do not cover is not the read's
              entry[u / 2] = (u & 1u) ? (entry[u / 2] & 0xFFFFu) | ((uint32_t)v << 16) : (uint32_t)v;
            }
            int reads_past = 0;
            auto at = [&](uint32_t u) { if (u >= J2_ENTRY_U16) reads_past = 1; return j2_half(entry[(u / 2) & 63u], u); };
            const uint32_t u2 = j2_slot2(len1, span, odd, k);
            const J2Shape sh = j2_shape(len1, u2 == J2_NONE ? rnd() : at(u2), span, odd, k, at);
            ++cases;
            if (reads_past) { printf("k %u len1 %u len2 %u odd %u fmt %d: j2_shape read behind the entry\n", k, len1, len2, odd, fmt); return 1; }
            // brute force: two parts of >= k nucleotides, what ends the read inside the entry, <= 128 positions
            const bool ends_inside = (fmt == PACKER) ? odd + used <= J2_ENTRY_U16 : (fmt == TERMINATED) ? odd + used < J2_ENTRY_U16 : false;
            const bool want = len2 >= k && ends_inside && len1 + len2 - k + 1 <= 128;
            if ((sh.ok != 0) != want) {
              printf("k %u len1 %u len2 %u odd %u fmt %d: qualifies %u, expected %d\n", k, len1, len2, odd, fmt, sh.ok, (int)want);
              return 1;
            }
            if (!want) continue;
            ++joined;
            if (sh.len1 != len1 || sh.len2 != len2 || sh.n_act != len1 + len2 - k + 1 || sh.g0 != len1 - k + 1 || sh.g1 != len1) {
              printf("k %u len1 %u len2 %u odd %u fmt %d: shape %u %u %u [%u, %u)\n", k, len1, len2, odd, fmt, sh.len1, sh.len2, sh.n_act, sh.g0, sh.g1);
              return 1;
            }
            uint32_t wd[12];
            j2_model(entry, odd, sh, wd);
            for (uint32_t n = 0; n < len1 + len2; ++n) {
              const uint32_t got = (wd[n / 16] >> (30 - 2 * (n % 16))) & 3u, exp = n < len1 ? n1[n] : n2[n - len1];
              if (got != exp) {
                printf("k %u len1 %u len2 %u odd %u fmt %d: nucleotide %u is %u, expected %u\n", k, len1, len2, odd, fmt, n, got, exp);
                return 1;
              }
            }
            dwords += (len1 + len2 + 15) / 16;
            // the k-mers of the read, and the position bits of the t-mers in their windows as the lanes of the two front halves
            // compute them: three positions per lane (k = 31), one per lane (the others)
            for (uint32_t pos = 0; pos < 192; ++pos) {
              const bool is = (pos + k <= len1) || (pos >= len1 && pos + k <= len1 + len2);
              if (j2_is_kmer(pos, sh.n_act, sh.g0, k) != is) {
                printf("k %u len1 %u len2 %u: position %u is%s a k-mer\n", k, len1, len2, pos, is ? "" : " not");
                return 1;
              }
              if (!is) continue;
              for (uint32_t i = 0; i + tl <= k; ++i) {
                const uint32_t p = pos + i, rel = p < len1 ? p : p - len1;
                const uint32_t off3 = j2_part_offset(3 * (p / 3) + 2, len1), off1 = j2_part_offset(p, len1);
                const uint32_t kmer_off3 = j2_part_offset(3 * (pos / 3) + 2, len1), kmer_rel = pos < len1 ? pos : pos - len1;
                if (p - off1 != rel || (k == 31 && (p - off3 != rel || pos - kmer_off3 != kmer_rel))) {
                  printf("k %u len1 %u len2 %u: t-mer %u of k-mer %u carries position %u / %u, expected %u\n", k, len1, len2, p, pos, p - off1, p - off3, rel);
                  return 1;
                }
              }
            }
          }
  }
  printf("ok: %ld reads, %ld joined, %ld window dwords\n", cases, joined, dwords);
  return 0;
}
