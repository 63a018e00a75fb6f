// The workgroup scan the integer stages of the segmentation output side share (seg_components.hip, seg_rle.hip).
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

}  // namespace dfw
