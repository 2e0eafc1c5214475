// mic_buckets.h — the walk over the on-disk buckets (.sz / .ky images) that the table builders (mic_build.hip) and the
// census (mic_kernels.hip: census_kernel) share: one thread per bucket of a 256-bucket tile, the tile's bases from a scan of
// per-tile sums (pass A of the builders), the sampling rule and the raw key load.  Device code only; every includer gets its
// own copy (anonymous namespace), as when the pieces lived in mic_build.hip.
#ifndef MIC_BUCKETS_H
#define MIC_BUCKETS_H

#include <stdint.h>

#define TILE 256

namespace {

struct TileA { unsigned long long elems; unsigned long long nonzero; };

// exclusive scan of (a,b) pairs over a 256-thread block; returns this thread's exclusive prefix and the
// block totals through tot_a/tot_b.
__device__ inline void block_scan2(uint32_t a, uint32_t b, uint32_t& ex_a, uint32_t& ex_b, uint32_t& tot_a,
                                   uint32_t& tot_b) {
  __shared__ uint32_t sa[TILE], sb[TILE];
  const int t = threadIdx.x;
  sa[t] = a; sb[t] = b;
  __syncthreads();
  for (int off = 1; off < TILE; off <<= 1) {
    uint32_t va = 0, vb = 0;
    if (t >= off) { va = sa[t - off]; vb = sb[t - off]; }
    __syncthreads();
    sa[t] += va; sb[t] += vb;
    __syncthreads();
  }
  ex_a = sa[t] - a; ex_b = sb[t] - b;
  tot_a = sa[TILE - 1]; tot_b = sb[TILE - 1];
  __syncthreads();
}

__device__ inline bool kept_bucket(uint32_t sz, uint64_t rank_incl, uint32_t sampling) {
  // CuClarkDB.cu:508-519: choice = (all || nbNonZeroBuckets % mod == 0) ? keep : skip, counted over non-empty buckets
  return sz > 0 && (sampling <= 1 || (rank_incl % sampling) == 0);
}

template <typename RAW>
__device__ inline uint64_t raw_key(const void* keys, uint64_t i) { return (uint64_t)((const RAW*)keys)[i]; }

}  // namespace

#endif
