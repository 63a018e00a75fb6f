// Tiled segmentation (pipeline.segment_tiled): an image larger than the processing size is covered with overlapping
// tile_h x tile_w windows, every window runs as a query against the prepared support, and the windows' quantised masks are
// blended back into ONE image that is thresholded once.  Two kernels around the existing query calls:
//
//   tiles_cut_kernel    staged RGB bytes [h][w][3] -> windows first .. first+count-1 as planar fp32 [count][3][th][tw]
//                       through the caller's 256-entry ToTensor + Normalize table (inputs.hip's): what
//                       DeviceImageTransform((th, tw)).image(crop) returns for the same crop, bit for bit -- Pillow's
//                       same-size resize is the identity.
//   tiles_merge_kernel  seg_u8 of every window and class [N][T][3][th][tw] -> [N][3][h][w] bytes + the per-class maximum.
//                       A GATHER: a thread owns 4 adjacent bytes of one output row, walks the windows that cover them and
//                       sums A = sum w * u and W = sum w in integers, w = min(dy + 1, th - dy, ramp) * min(dx + 1, tw - dx,
//                       ramp); the byte is (2 A + W) / (2 W), round-half-up, in 32 bits (the host proves 2 A + W fits before
//                       it launches).  No float operation and no atomic on the image: the result depends on no order.
//                       The maximum goes the way seg_u8_kernel's does (wave reduce, one atomicMax per workgroup) into
//                       mx[n], zeroed by tiles_zero_kernel (a library kernel, not a memset node: see seg_zero_kernel in
//                       misc.hip).
//
// The window plan (dfw_tile_plan: sizes, ramp, at most 64 origins per axis) travels BY VALUE in the kernel arguments, as
// dfw_fsa_attention_ragged's table does: no device allocation, no copy, and a capture keeps the values.  Both kernels are
// HBM-bound byte work; window columns are in general not 4-aligned against the image, so the merge reads a window's four
// bytes as one word only where that address is aligned and byte by byte otherwise, and both write words / float4 only where
// the destination is aligned.
#include "common.h"

namespace dfw {

__global__ void tiles_zero_kernel(uint32_t* mx, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) mx[e] = 0u;
}

// Block (64, 4): x -> 4 adjacent columns of the window, y -> row of the window, grid z -> window first + z.
__global__ __launch_bounds__(256) void tiles_cut_kernel(const dfw_tile_plan p, const uint8_t* __restrict__ img,
                                                        const float* __restrict__ lut, float* __restrict__ out,
                                                        int first) {
  const int th = p.tile_h, tw = p.tile_w;
  const int x4 = (blockIdx.x * 64 + threadIdx.x) * 4;
  const int dy = blockIdx.y * 4 + threadIdx.y;
  if (x4 >= tw || dy >= th) return;
  const int t = first + blockIdx.z;
  const int iy = t / p.nx, ix = t - iy * p.nx;
  const uint8_t* src = img + ((size_t)(p.ys[iy] + dy) * p.img_w + p.xs[ix] + x4) * 3;
  const size_t plane = (size_t)th * tw;
  float* dst = out + (size_t)blockIdx.z * 3 * plane + (size_t)dy * tw + x4;
  const int nx = min(4, tw - x4);
  if (nx == 4 && (tw & 3) == 0 && ((uintptr_t)out & 15) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = lut[src[3 * j + c]];
      *(f32x4*)(dst + c * plane) = v;
    }
  } else {
    for (int j = 0; j < nx; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[c * plane + j] = lut[src[3 * j + c]];
  }
}

// Block (64, 4): x -> 4 adjacent columns of the image, y -> row of the flat 3 * h rows of class blockIdx.z's planes.
// 32-bit sums: dfw_tiles_merge launches only where 511 * (largest sum of weights over a pixel) < 2^32.
__global__ __launch_bounds__(256) void tiles_merge_kernel(const dfw_tile_plan p, const uint8_t* __restrict__ win,
                                                          uint8_t* __restrict__ out, uint32_t* mx) {
  const int h = p.img_h, w = p.img_w, th = p.tile_h, tw = p.tile_w, ramp = p.ramp;
  const int x4 = (blockIdx.x * 64 + threadIdx.x) * 4;
  const int row = blockIdx.y * 4 + threadIdx.y;
  const int n = blockIdx.z, T = p.ny * p.nx;
  uint32_t m = 0;
  if (x4 < w && row < 3 * h) {
    const int c = row / h, y = row - c * h;
    const int nxp = min(4, w - x4);
    const size_t plane = (size_t)th * tw;
    uint32_t A[4] = {0, 0, 0, 0}, W[4] = {0, 0, 0, 0};
    for (int iy = 0; iy < p.ny; ++iy) {
      const int dy = y - p.ys[iy];
      if (dy < 0) break;                  // origins ascend: no later row of windows reaches y
      if (dy >= th) continue;
      const uint32_t wy = (uint32_t)min(min(dy + 1, th - dy), ramp);
      for (int ix = 0; ix < p.nx; ++ix) {
        const int dx0 = x4 - p.xs[ix];    // column of this thread's first pixel inside window ix (may be outside)
        if (dx0 + 3 < 0) break;           // this and every later window begin right of the four pixels
        if (dx0 >= tw) continue;
        const uint8_t* src = win + (((size_t)n * T + (size_t)iy * p.nx + ix) * 3 + c) * plane + (size_t)dy * tw;
        if (dx0 >= 0 && dx0 + 3 < tw && nxp == 4 && ((uintptr_t)(src + dx0) & 3) == 0) {
          const uint32_t v = *(const uint32_t*)(src + dx0);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int dx = dx0 + j;
            const uint32_t wt = wy * (uint32_t)min(min(dx + 1, tw - dx), ramp);
            A[j] += wt * ((v >> (8 * j)) & 255u);
            W[j] += wt;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int dx = dx0 + j;
            if (j < nxp && dx >= 0 && dx < tw) {
              const uint32_t wt = wy * (uint32_t)min(min(dx + 1, tw - dx), ramp);
              A[j] += wt * src[dx];
              W[j] += wt;
            }
          }
        }
      }
    }
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nxp) {
        const uint32_t q = (2 * A[j] + W[j]) / (2 * W[j]);   // W > 0: the plan leaves no pixel uncovered
        word |= q << (8 * j);
        m = max(m, q);
      }
    uint8_t* dst = out + ((size_t)n * 3 * h + row) * w + x4;
    if (nxp == 4 && ((uintptr_t)dst & 3) == 0) {
      *(uint32_t*)dst = word;
    } else {
      for (int j = 0; j < nxp; ++j) dst[j] = (uint8_t)(word >> (8 * j));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  __shared__ uint32_t wmax[4];
  const int tid = threadIdx.y * 64 + threadIdx.x;
  if ((tid & 63) == 0) wmax[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) atomicMax(mx + n, max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3])));
}

// One axis of the plan: n origins in 1..64, strictly ascending from 0 to len - tile, neighbours at most a tile apart (no
// pixel uncovered).  *cover = the largest number of windows over one pixel of the axis.
static bool tiles_axis_ok(const int32_t* o, int n, int len, int tile, int* cover) {
  if (n < 1 || n > DFW_TILE_MAX_ORIGINS || tile < 1 || len < tile) return false;
  if (o[0] != 0 || o[n - 1] != len - tile) return false;
  int most = 1;
  for (int i = 1; i < n; ++i) {
    if (o[i] <= o[i - 1] || o[i] - o[i - 1] > tile) return false;
    int k = 1;   // windows j < i that still cover pixel o[i]; the cover is largest at some window's first pixel
    for (int j = i - 1; j >= 0 && o[j] + tile > o[i]; --j) ++k;
    most = k > most ? k : most;
  }
  *cover = most;
  return true;
}

static bool tiles_plan_ok(const dfw_tile_plan* p, int* cover_y, int* cover_x) {
  if (!p || p->img_h < 1 || p->img_w < 1 || p->tile_h < 1 || p->tile_w < 1) return false;
  if (!tiles_axis_ok(p->ys, p->ny, p->img_h, p->tile_h, cover_y)) return false;
  if (!tiles_axis_ok(p->xs, p->nx, p->img_w, p->tile_w, cover_x)) return false;
  const int small = p->tile_h < p->tile_w ? p->tile_h : p->tile_w;
  const int ramp_max = small / 2 > 1 ? small / 2 : 1;
  return p->ramp >= 1 && p->ramp <= ramp_max;
}

}  // namespace dfw

using namespace dfw;

extern "C" int dfw_tiles_cut(const dfw_tile_plan* plan, const uint8_t* img, const float* lut, float* out, int32_t first,
                             int32_t count, dfw_stream_t stream) {
  int cy, cx;
  if (!plan || !img || !lut || !out) return DFW_EINVAL;
  if (!tiles_plan_ok(plan, &cy, &cx)) return DFW_EINVAL;
  const int T = plan->ny * plan->nx;
  if (first < 0 || count < 1 || first > T - count) return DFW_EINVAL;
  if (plan->tile_h > 65535 * 4) return DFW_ERANGE;   // grid y
  const dim3 grid((plan->tile_w + 255) / 256, (plan->tile_h + 3) / 4, count);
  hipLaunchKernelGGL(tiles_cut_kernel, grid, dim3(64, 4), 0, (hipStream_t)stream, *plan, img, lut, out, first);
  DFW_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfw_tiles_merge(const dfw_tile_plan* plan, const uint8_t* win, int32_t N, uint8_t* out, uint32_t* mx,
                               dfw_stream_t stream) {
  int cy, cx;
  if (!plan || !win || !out || !mx) return DFW_EINVAL;
  if (N < 1 || N > 254) return DFW_EINVAL;
  if (!tiles_plan_ok(plan, &cy, &cx)) return DFW_EINVAL;
  if (plan->img_h > 65535) return DFW_ERANGE;        // grid y = ceil(3 h / 4)
  // the kernel sums in 32 bits: 2 A + W <= 511 * sum w, and sum w <= (windows over the pixel) * ramp^2.  With up to 4
  // windows per axis over a pixel that holds for every ramp of tiles up to 1448 a side
  const uint64_t wsum = (uint64_t)cy * cx * (uint64_t)plan->ramp * (uint64_t)plan->ramp;
  if (wsum > 0xffffffffull / 511ull) return DFW_ERANGE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tiles_zero_kernel, dim3((N + 255) / 256), dim3(256), 0, st, mx, N);
  DFW_CHECK_LAUNCH();
  const dim3 grid((plan->img_w + 255) / 256, (3 * plan->img_h + 3) / 4, N);
  hipLaunchKernelGGL(tiles_merge_kernel, grid, dim3(64, 4), 0, st, *plan, win, out, mx);
  DFW_CHECK_LAUNCH();
  return 0;
}
