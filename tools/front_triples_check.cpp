// front_triples_check - the three-t-mers-per-lane front half (cuclark_amd/csrc/mic_front3.h: f3_model) against the brute force
// min(key[i .. i+23]) on chunks of every size, stand-alone (tests/test_front_triples.py builds it with ASan + UBSan).
//   front_triples_check [seed]      exit status 0 and a line of counts, or the first difference and status 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mic_front3.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}

static uint32_t tmer_at(const std::vector<uint8_t>& nt, int p) {
  uint32_t v = 0;
  for (int i = 0; i < F3_T; ++i) v = v << 2 | nt[p + i];
  return v;
}
static uint32_t rc_tmer(uint32_t v) {
  uint32_t r = 0;
  for (int i = 0; i < F3_T; ++i) { r = r << 2 | (3u - (v & 3u)); v >>= 2; }
  return r;
}
static uint32_t key_at(const std::vector<uint8_t>& nt, int p, bool canon) {
  uint32_t tv = tmer_at(nt, p);
  if (canon) { const uint32_t tr = rc_tmer(tv); tv = tr < tv ? tr : tv; }
  return ((tv * 0x9E3779u + 0x27D4EB2Fu) & ~31u) | ((uint32_t)p & 31u);
}

// the 8-mer with the smallest order, as it stands and canonical: what lies past the part is filled with it, so a window that
// reached one t-mer too far would show
static uint32_t lowest_tmer(bool canon) {
  uint32_t best = 0, bk = 0xFFFFFFFFu;
  for (uint32_t v = 0; v < 65536u; ++v) {
    uint32_t tv = v;
    if (canon) { const uint32_t tr = rc_tmer(v); tv = tr < tv ? tr : tv; }
    const uint32_t k = (tv * 0x9E3779u + 0x27D4EB2Fu) >> 5;
    if (k < bk) { bk = k; best = v; }
  }
  return best;
}

enum { RANDOM, HOMOPOLYMER, DINUCLEOTIDE, TRINUCLEOTIDE, TWO_LETTERS, REPEATED_TMER, N_KINDS };
enum { PAST_RANDOM, PAST_LOWEST, PAST_ZERO, N_PAST };

int main(int argc, char** argv) {
  if (argc > 1) rng_state ^= strtoull(argv[1], nullptr, 10) * 0xD1342543DE82EF95ull;
  const int NT = 64 * 16;
  long chunks = 0, kmers = 0, runs = 0;
  for (int canon = 0; canon < 2; ++canon) {
    const uint32_t low = lowest_tmer(canon != 0);
    for (uint32_t n_act = 1; n_act <= 128; ++n_act)
      for (int kind = 0; kind < N_KINDS; ++kind)
        for (int past = 0; past < N_PAST; ++past)
          for (int trial = 0; trial < 3; ++trial) {
            const int plen = (int)n_act + F3_K - 1;               // nucleotides of the part from the chunk's first on
            std::vector<uint8_t> nt(NT);
            const uint32_t unit = rnd();
            for (int i = 0; i < plen; ++i) {
              switch (kind) {
                case RANDOM: nt[i] = rnd() & 3; break;
                case HOMOPOLYMER: nt[i] = unit & 3; break;
                case DINUCLEOTIDE: nt[i] = (unit >> (2 * (i % 2))) & 3; break;
                case TRINUCLEOTIDE: nt[i] = (unit >> (2 * (i % 3))) & 3; break;
                case TWO_LETTERS: nt[i] = (rnd() & 1) ? (unit & 3) : ((unit >> 2) & 3); break;
                default: nt[i] = (i / 40) % 2 ? (rnd() & 3) : (unit >> (2 * (i % F3_T))) & 3; break;   // the same t-mer every 8 positions, then random
              }
            }
            // a homopolymer run in the middle of a random read: tied t-mers between distinct ones
            if (kind == RANDOM && trial == 2 && plen > 60) for (int i = 20; i < 20 + 8 + (int)(rnd() % 24); ++i) nt[i] = unit & 3;
            for (int i = plen; i < NT; ++i)
              nt[i] = past == PAST_RANDOM ? (rnd() & 3) : past == PAST_LOWEST ? (low >> (2 * (F3_T - 1 - (i - plen) % F3_T))) & 3 : 0;
            uint32_t wd[64];
            for (int l = 0; l < 64; ++l) { uint32_t v = 0; for (int i = 0; i < 16; ++i) v = v << 2 | nt[16 * l + i]; wd[l] = v; }
            uint32_t q[192]; uint16_t rec[132];
            memset(rec, 0xEE, sizeof rec);
            const uint32_t R = f3_model(wd, n_act, canon != 0, q, rec);
            // brute force
            std::vector<uint32_t> want(n_act);
            for (uint32_t i = 0; i < n_act; ++i) {
              uint32_t best = 0xFFFFFFFFu; int at = 0;
              for (int j = 0; j < F3_WIN; ++j) { const uint32_t k = key_at(nt, (int)i + j, canon != 0); if (k < best) { best = k; at = j; } }
              want[i] = i + (uint32_t)(at % F3_WM);
            }
            for (uint32_t i = 0; i < 192; ++i) {
              const uint32_t w = i < n_act ? want[i] : ~0u;
              if (q[i] != w) {
                printf("canon %d n_act %u kind %d past %d trial %d: k-mer %u samples %u, brute force %u\n", canon, n_act, kind, past, trial, i, q[i], w);
                return 1;
              }
            }
            std::vector<uint16_t> wrec;
            for (uint32_t i = 0; i < n_act; ++i) if (i == 0 || want[i] != want[i - 1]) wrec.push_back((uint16_t)(want[i] | i << 8));
            const uint32_t wR = (uint32_t)wrec.size();
            bool ok = R == wR;
            for (uint32_t i = 0; ok && i < wR; ++i) ok = rec[i] == wrec[i];
            ok = ok && (uint32_t)(rec[wR] >> 8) == n_act;                             // the closing record: its k-mer (the low byte is never read)
            for (uint32_t i = wR + 1; ok && i < 132; ++i) ok = rec[i] == 0xEEEE;       // nothing written behind the closing record
            if (!ok) {
              printf("canon %d n_act %u kind %d past %d trial %d: %u runs, brute force %u, or other records\n", canon, n_act, kind, past, trial, R, wR);
              return 1;
            }
            ++chunks; kmers += n_act; runs += wR;
          }
  }
  printf("ok: %ld chunks, %ld k-mers, %ld runs\n", chunks, kmers, runs);
  return 0;
}
