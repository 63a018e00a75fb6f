// The workgroup scan the integer stages of the segmentation output side share (seg_components.hip, seg_sort.h,
// seg_match.hip), and the in-chunk ranking of the radix sort (seg_sort.h).
#pragma once
#include "common.h"

namespace dfw {

// Exclusive scan of one int per thread over the workgroup of 256; *total = the sum.  Two barriers.
__device__ __forceinline__ int block_scan(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  int off = 0;
  for (int w = 0; w < wv; ++w) off += wsum[w];
  *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  return off + inc - v;
}

// One round of 256 records of a sort chunk in a stable radix scatter: the destination of this thread's record, whose
// digit is d (`on`: the thread holds a record).  run [256] holds, per digit, where the next record of that digit goes --
// the scanned table entry of the chunk, advanced here by the round's counts -- and wcnt [4][256], all zero on entry and
// again on return, the counts of the four waves.  Ranks come from ballots inside a wave, per-wave counts across the waves
// and `run` across the rounds: a fixed order, no atomic decides a position.  Three barriers; every thread of the
// workgroup calls it.  Its one caller is seg_scatter_kernel (seg_sort.h).
__device__ __forceinline__ int chunk_rank(bool on, int d, int (&run)[256], int (&wcnt)[4][256]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // the lanes of this wave that hold a record of the same digit
  unsigned long long m = __ballot(on);
#pragma unroll
  for (int bit = 0; bit < 8; ++bit) {
    const bool set = (d >> bit) & 1;
    const unsigned long long bal = __ballot(set);
    m &= set ? bal : ~bal;
  }
  const int rank = __popcll(m & ((1ull << lane) - 1ull));
  if (on && rank == 0) wcnt[wv][d] = __popcll(m);
  __syncthreads();
  int pos = 0;
  if (on) {
    pos = run[d] + rank;
    for (int w = 0; w < wv; ++w) pos += wcnt[w][d];
  }
  __syncthreads();
  run[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
#pragma unroll
  for (int w = 0; w < 4; ++w) wcnt[w][threadIdx.x] = 0;
  __syncthreads();
  return pos;
}

}  // namespace dfw
