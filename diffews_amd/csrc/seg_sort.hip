// The kernels of seg_sort.h that depend on no stage, and their launchers.
#include "seg_sort.h"

namespace dfw {

// a [plane][image][n], plane = blockIdx.y, image = blockIdx.x: exclusive scan in place, 4 consecutive words per thread and
// round.  nout (optional, plane 0 only): nout[stride * image + 0..1] = (min(sum, limit), sum).
__global__ __launch_bounds__(256) void seg_scan_kernel(int32_t* a, int n, int32_t* nout, int stride, int limit) {
  __shared__ int wsum[4];
  int32_t* o = a + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * n;
  int carry = 0;
  for (int base = 0; base < n; base += 1024) {
    const int i0 = base + 4 * threadIdx.x;
    int v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = i0 + j < n ? o[i0 + j] : 0;
      s += v[j];
    }
    int total;
    int e = carry + block_scan(s, wsum, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i0 + j < n) o[i0 + j] = e;
      e += v[j];
    }
    carry += total;
  }
  if (nout && blockIdx.y == 0 && threadIdx.x == 0) {
    nout[stride * blockIdx.x] = min(carry, limit);
    nout[stride * blockIdx.x + 1] = carry;
  }
}

__global__ __launch_bounds__(256) void seg_hist_kernel(const int32_t* key, int32_t* tab, const int32_t* n, int stride,
                                                       int max_records, int shift) {
  __shared__ int hist[256];
  const int b = blockIdx.y, nchunk = gridDim.x, kept = min(n[stride * b], max_records);
  hist[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSegRec / 256; ++r) {
    const int i = blockIdx.x * kSegRec + r * 256 + threadIdx.x;
    if (i < kept) atomicAdd(&hist[(key[(size_t)b * max_records + i] >> shift) & 255], 1);
  }
  __syncthreads();
  tab[((size_t)b * 256 + threadIdx.x) * nchunk + blockIdx.x] = hist[threadIdx.x];
}

int seg_scan_launch(hipStream_t st, int32_t* a, int planes, int images, int n, int32_t* nout, int stride, int limit) {
  hipLaunchKernelGGL(seg_scan_kernel, dim3(images, planes), dim3(256), 0, st, a, n, nout, stride, limit);
  DFW_CHECK_LAUNCH();
  return 0;
}

int seg_hist_launch(hipStream_t st, const int32_t* key, int32_t* tab, const int32_t* n, int stride, int B, int max_records,
                    int shift) {
  hipLaunchKernelGGL(seg_hist_kernel, dim3(seg_chunks(max_records), B), dim3(256), 0, st, key, tab, n, stride, max_records,
                     shift);
  DFW_CHECK_LAUNCH();
  return 0;
}

}  // namespace dfw
