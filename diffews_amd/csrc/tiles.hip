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
//                       mx[n], zeroed by seg_zero_launch (common.h).
//
// The window plan (dfw_tile_plan: sizes, ramp, at most 64 origins per axis) travels BY VALUE in the kernel arguments, as
// dfw_fsa_attention_ragged's table does: no device allocation, no copy, and a capture keeps the values.  Both kernels are
// HBM-bound byte work; window columns are in general not 4-aligned against the image, so the merge reads a window's four
// bytes as one word only where that address is aligned and byte by byte otherwise, and both write words / float4 only where
// the destination is aligned.
#include "common.h"

namespace dfw {

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

// ---------------------------------------------------------------------------------------------- candidate classes per window
//
// dfw_tiles_labels_cand: the merge and the label rule in ONE gather over a SPARSE set of (window, class) entries.  A pair
// that is not listed counts as an all-zero mask: it adds nothing to A and its weight to W, exactly as a zero window does in
// tiles_merge_kernel, so labels / mx / counts are what dfw_tiles_merge + dfw_seg_labels give on the dense buffer -- which is
// never built, and neither is the [N][3][h][w] merged image.
//
// The origins and ends of the windows cut each axis into at most 2 * 64 - 1 intervals; inside a CELL (a y interval x an
// x interval) every pixel is covered by the same rectangle of windows iy0..iy1 x ix0..ix1.  A workgroup works inside one
// cell (grid x / y = cell, z = a share of its rows), so everything about "which windows, which classes" is uniform in
// the workgroup: it scatters the lists of its nwin windows into an LDS table slot[class][window] = entry (or -1) once,
// and then every thread walks, per 4 adjacent pixels, the classes present in ascending order and the windows that carry
// each.  The cost follows the entries present: an absent class is one LDS read per workgroup-uniform step, an absent
// (window, class) pair one broadcast LDS read.  The table holds kCandSlots words: cells of plans with N * nwin above that
// (more than 16 windows over a pixel at N = 254) go through it in chunks of classes, rebuilt per pixel step.
//
// Per pixel the divisor 2 W is the same for all classes and channels, so the byte (2 A + W) / (2 W) is taken with one
// reciprocal per pixel: q' = umulhi(n, floor((2^32 - 1) / d)) is at most 2 below floor(n / d) for n < 2^32, d >= 2, and
// two compare-and-adds on the remainder make it exact.  Scores, thresholds and the tie rule are seg_fuse's (seg_fuse.h) fp32
// expressions; maxima, counts and area go through LDS bins and one global atomic per touched bin and workgroup.
constexpr int kCandSlots = 4096;   // = 64 * 64, the most windows a valid plan puts over one pixel

struct tiles_cells {
  int32_t ncy, ncx;                    // cells per axis
  int32_t by[2 * DFW_TILE_MAX_ORIGINS + 1], bx[2 * DFW_TILE_MAX_ORIGINS + 1];   // cell i of an axis is [b[i], b[i + 1])
};

// LABELS = false: the maximum pass (mx only), run first when the threshold is dynamic.  LABELS = true: labels, counts /
// area where asked for, and with the fixed threshold also mx.
// Block (64, 4): x -> 4 adjacent columns (image-aligned, clipped to the cell), y -> row.
template <bool LABELS>
__global__ __launch_bounds__(256) void tiles_cand_kernel(const dfw_tile_plan p, const tiles_cells cells,
                                                         const uint8_t* __restrict__ ent, const int32_t* __restrict__ tab,
                                                         const uint8_t* __restrict__ gt, uint8_t* __restrict__ labels,
                                                         uint32_t* mx, unsigned long long* counts,
                                                         unsigned long long* area, int E_cap, int N, float r_thr,
                                                         float fixed_thr) {
  __shared__ int32_t slot[kCandSlots];          // [class of the chunk][window of the cell] -> entry, -1: not listed
  __shared__ uint8_t present[256];              // class of the chunk listed by any window of the cell
  __shared__ uint32_t lmax[256];                // maximum pass: per class
  __shared__ float lut[256];
  __shared__ float thr[256];
  __shared__ unsigned hist[3 * 256];            // [inter | pred | gt][N + 1]
  __shared__ unsigned ahist[2 * 256];           // [foreground | won][class]
  const int th = p.tile_h, tw = p.tile_w, ramp = p.ramp, w = p.img_w;
  const int cy0 = cells.by[blockIdx.y], cy1 = cells.by[blockIdx.y + 1];
  const int cx0 = cells.bx[blockIdx.x], cx1 = cells.bx[blockIdx.x + 1];
  const int Z = gridDim.z;
  if ((int)blockIdx.z * 4 >= cy1 - cy0) return;           // uniform, before any barrier: a cell lower than its shares
  // the windows over the cell: origins ascend, so they are a range per axis (never empty: the plan leaves no pixel uncovered)
  int iy0 = 0, iy1 = 0, ix0 = 0, ix1 = 0;
  for (int i = 0; i < p.ny; ++i) {
    if (p.ys[i] + th <= cy0) iy0 = i + 1;
    if (p.ys[i] <= cy0) iy1 = i;
  }
  for (int i = 0; i < p.nx; ++i) {
    if (p.xs[i] + tw <= cx0) ix0 = i + 1;
    if (p.xs[i] <= cx0) ix1 = i;
  }
  iy0 = min(iy0, iy1);
  ix0 = min(ix0, ix1);
  const int nwx = ix1 - ix0 + 1, nwin = (iy1 - iy0 + 1) * nwx;      // <= 64 * 64 = kCandSlots
  const int CH = min(N, kCandSlots / nwin);                         // classes per chunk of the table, >= 1
  const int T = p.ny * p.nx, NL = N + 1;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  const int32_t* cls = tab + T + 1;
  lut[tid] = (float)tid / 255.0f;
  if (LABELS) {
    if (tid < N) {
      float t = fixed_thr;
      if (r_thr > 0.f) t = ((float)mx[tid] / 255.0f) * r_thr;
      thr[tid] = t;
    }
    for (int i = tid; i < 3 * 256; i += 256) hist[i] = 0u;
    for (int i = tid; i < 2 * 256; i += 256) ahist[i] = 0u;
  }
  lmax[tid] = 0u;
  const bool want_max = !LABELS || !(r_thr > 0.f);        // with the fixed threshold the label pass is the only one
  // slot / present of classes c0 .. c0 + CH - 1; barriers on both sides, so every thread of the workgroup calls it
  auto build = [&](int c0) {
    __syncthreads();
    const int nc = min(CH, N - c0);
    for (int i = tid; i < nc * nwin; i += 256) slot[i] = -1;
    present[tid] = 0;
    __syncthreads();
    for (int k = tid; k < nwin; k += 256) {
      const int t = (iy0 + k / nwx) * p.nx + ix0 + k % nwx;
      // what the device table holds is clamped before anything is indexed with it
      int lo = tab[t], hi = tab[t + 1];
      lo = min(max(lo, 0), E_cap);
      hi = min(max(hi, lo), E_cap);
      for (int e = lo; e < hi; ++e) {
        const int c = min(max(cls[e], 0), N - 1) - c0;
        if (c >= 0 && c < nc) {
          slot[c * nwin + k] = e;
          present[c] = 1;
        }
      }
    }
    __syncthreads();
  };
  if (CH >= N) build(0);
  const size_t plane = (size_t)th * tw;
  const int q0 = cx0 >> 2, nq = ((cx1 + 3) >> 2) - q0;
  const int row_steps = (cy1 - cy0 + 4 * Z - 1) / (4 * Z), col_steps = (nq + 63) / 64;
  for (int rs = 0; rs < row_steps; ++rs)
    for (int cs = 0; cs < col_steps; ++cs) {                // the same trip count in every thread: build() has barriers
      const int y = cy0 + (rs * Z + (int)blockIdx.z) * 4 + (int)threadIdx.y;
      const int x4 = (q0 + cs * 64 + (int)threadIdx.x) * 4;
      const int j0 = max(cx0 - x4, 0), j1 = min(cx1 - x4, 4);      // this thread's pixels x4 + j0 .. x4 + j1 - 1
      const bool active = y < cy1 && j0 < j1;
      // W and its reciprocal per pixel: over ALL windows of the cell, whatever they list
      uint32_t W[4] = {0, 0, 0, 0}, rcp[4] = {0, 0, 0, 0};
      if (active) {
        for (int iy = iy0; iy <= iy1; ++iy) {
          const int dy = y - p.ys[iy];
          const uint32_t wy = (uint32_t)min(min(dy + 1, th - dy), ramp);
          for (int ix = ix0; ix <= ix1; ++ix) {
            const int dx0 = x4 - p.xs[ix];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int dx = dx0 + j;
              if (j >= j0 && j < j1) W[j] += wy * (uint32_t)min(min(dx + 1, tw - dx), ramp);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j >= j0 && j < j1) rcp[j] = 0xffffffffu / (2u * W[j]);   // W > 0: every window of the cell covers the pixel
      }
      float best[4] = {-1.f, -1.f, -1.f, -1.f};
      uint32_t lab[4] = {0u, 0u, 0u, 0u};
      for (int c0 = 0; c0 < N; c0 += CH) {
        if (CH < N) build(c0);
        if (!active) continue;
        const int nc = min(CH, N - c0);
        for (int cc = 0; cc < nc; ++cc) {
          if (!present[cc]) continue;
          uint32_t A[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
          const int32_t* sl = slot + cc * nwin;
          for (int iy = iy0, k = 0; iy <= iy1; ++iy) {
            const int dy = y - p.ys[iy];
            const uint32_t wy = (uint32_t)min(min(dy + 1, th - dy), ramp);
            for (int ix = ix0; ix <= ix1; ++ix, ++k) {
              const int e = sl[k];
              if (e < 0) continue;
              const int dx0 = x4 - p.xs[ix];
              uint32_t wt[4];
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int dx = dx0 + j;
                wt[j] = wy * (uint32_t)min(min(dx + 1, tw - dx), ramp);
              }
              const uint8_t* src = ent + (size_t)e * 3 * plane + (size_t)dy * tw + dx0;
              if (j0 == 0 && j1 == 4 && (((uintptr_t)src | plane) & 3) == 0) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                  const uint32_t v = *(const uint32_t*)(src + ch * plane);
#pragma unroll
                  for (int j = 0; j < 4; ++j) A[ch][j] += wt[j] * ((v >> (8 * j)) & 255u);
                }
              } else {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                  for (int j = 0; j < 4; ++j)
                    if (j >= j0 && j < j1) A[ch][j] += wt[j] * src[ch * plane + j];
              }
            }
          }
          const int c = c0 + cc;
          uint32_t m = 0u, nfg = 0u;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j < j0 || j >= j1) continue;
            const uint32_t d = 2u * W[j];
            uint32_t q[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              const uint32_t n = 2u * A[ch][j] + W[j];           // < 2^32: the host proved 511 * sum w fits
              uint32_t qq = __umulhi(n, rcp[j]);
              uint32_t r = n - qq * d;
              if (r >= d) { r -= d; ++qq; }
              if (r >= d) ++qq;
              q[ch] = qq;
              m = max(m, qq);
            }
            if (LABELS) {
              const float sc = ((lut[q[0]] + lut[q[1]]) + lut[q[2]]) / 3.0f;
              if (sc > thr[c]) {
                ++nfg;
                if (sc > best[j]) { best[j] = sc; lab[j] = (uint32_t)(c + 1); }
              }
            }
          }
          if (LABELS && area && nfg) atomicAdd(&ahist[c], nfg);
          if (want_max && m > lmax[c]) atomicMax(&lmax[c], m);
        }
      }
      if (!LABELS || !active) continue;
      uint8_t* dst = labels + (size_t)y * w + x4;
      if (j0 == 0 && j1 == 4 && ((uintptr_t)dst & 3) == 0) {
        *(uint32_t*)dst = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
      } else {
        for (int j = j0; j < j1; ++j) dst[j] = (uint8_t)lab[j];
      }
      for (int j = j0; j < j1; ++j) {
        if (area && lab[j]) atomicAdd(&ahist[256 + lab[j] - 1], 1u);
        if (gt) {
          const uint32_t g = gt[(size_t)y * w + x4 + j];
          if (g > (uint32_t)N) continue;   // 255 = ignore; N < g < 255 has no bin: dropped from every histogram too
          atomicAdd(&hist[NL + lab[j]], 1u);
          atomicAdd(&hist[2 * NL + g], 1u);
          if (lab[j] == g) atomicAdd(&hist[lab[j]], 1u);
        }
      }
    }
  __syncthreads();
  if (want_max && tid < N && lmax[tid]) atomicMax(mx + tid, lmax[tid]);
  if (!LABELS) return;
  if (gt) {
    for (int l = tid; l < NL; l += 256) {
      const unsigned in = hist[l], un = hist[NL + l] + hist[2 * NL + l] - in;
      if (in) atomicAdd(counts + l, (unsigned long long)in);
      if (un) atomicAdd(counts + NL + l, (unsigned long long)un);
    }
  }
  if (area && tid < N) {
    const unsigned fg = ahist[tid], won = ahist[256 + tid];
    if (fg) atomicAdd(area + 2 * (size_t)tid, (unsigned long long)fg);
    if (won) atomicAdd(area + 2 * (size_t)tid + 1, (unsigned long long)won);
  }
}

// The sorted, distinct origins and ends of one axis: b[0] = 0 .. b[n] = len; returns n, the number of cells.
static int tiles_axis_cells(const int32_t* o, int n, int tile, int32_t* b) {
  int m = 0, i = 0, j = 0;   // both o[] and o[] + tile ascend: a two-way merge
  while (i < n || j < n) {
    int v;
    if (i < n && o[i] <= o[j] + tile) v = o[i++];
    else v = o[j++] + tile;
    if (m == 0 || b[m - 1] != v) b[m++] = v;
  }
  return m - 1;
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
  if (int e = seg_zero_launch(st, mx, N, nullptr, 0)) return e;
  const dim3 grid((plan->img_w + 255) / 256, (3 * plan->img_h + 3) / 4, N);
  hipLaunchKernelGGL(tiles_merge_kernel, grid, dim3(64, 4), 0, st, *plan, win, out, mx);
  DFW_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfw_tiles_labels_cand(const dfw_tile_plan* plan, const uint8_t* ent, const int32_t* tab,
                                     const int32_t* tab_host, const uint8_t* gt, uint8_t* labels, uint32_t* mx,
                                     int64_t* counts, int64_t* area, int32_t E_cap, int32_t N, float r_threshold,
                                     float threshold, dfw_stream_t stream) {
  int cy, cx;
  if (!plan || !tab || !tab_host || !labels || !mx) return DFW_EINVAL;
  if (N < 1 || N > 254 || E_cap < 1) return DFW_EINVAL;
  if (counts && !gt) return DFW_EINVAL;
  if (!(r_threshold > 0.f) && !(threshold > 0.f)) return DFW_EINVAL;
  if (!tiles_plan_ok(plan, &cy, &cx)) return DFW_EINVAL;
  // the table's host mirror: offsets from 0, non-decreasing, at most E_cap; classes 0..N-1, strictly ascending per window
  const int T = plan->ny * plan->nx;
  if (tab_host[0] != 0) return DFW_EINVAL;
  for (int t = 0; t < T; ++t)
    if (tab_host[t + 1] < tab_host[t] || tab_host[t + 1] > E_cap) return DFW_EINVAL;
  const int E = tab_host[T];
  if (E > 0 && !ent) return DFW_EINVAL;
  for (int t = 0; t < T; ++t)
    for (int e = tab_host[t]; e < tab_host[t + 1]; ++e) {
      const int32_t c = tab_host[T + 1 + e];
      if (c < 0 || c >= N) return DFW_EINVAL;
      if (e > tab_host[t] && c <= tab_host[T + e]) return DFW_EINVAL;
    }
  if (plan->img_h > 65535) return DFW_ERANGE;        // dfw_tiles_merge's limit
  // dfw_tiles_merge's proof that 2 A + W fits 32 bits: absent pairs only make A smaller
  const uint64_t wsum = (uint64_t)cy * cx * (uint64_t)plan->ramp * (uint64_t)plan->ramp;
  if (wsum > 0xffffffffull / 511ull) return DFW_ERANGE;
  tiles_cells cells;
  cells.ncy = tiles_axis_cells(plan->ys, plan->ny, plan->tile_h, cells.by);
  cells.ncx = tiles_axis_cells(plan->xs, plan->nx, plan->tile_w, cells.bx);
  int tall = 1;
  for (int i = 0; i < cells.ncy; ++i) tall = cells.by[i + 1] - cells.by[i] > tall ? cells.by[i + 1] - cells.by[i] : tall;
  // shares of a cell's rows: enough workgroups for the chip (about 2048), none without a row in the tallest cell
  int Z = (2048 + cells.ncy * cells.ncx - 1) / (cells.ncy * cells.ncx);
  if (Z > (tall + 3) / 4) Z = (tall + 3) / 4;
  hipStream_t st = (hipStream_t)stream;
  const bool want_counts = gt && counts;
  if (int e = seg_zero_launch(st, mx, N, want_counts ? counts : nullptr, 2 * (N + 1), area, 2 * N)) return e;
  const dim3 grid(cells.ncx, cells.ncy, Z);
  const int cap = ent ? E_cap : 0;   // without entries the kernel sees every list empty, whatever the device table holds
  if (r_threshold > 0.f && E > 0) {
    hipLaunchKernelGGL(tiles_cand_kernel<false>, grid, dim3(64, 4), 0, st, *plan, cells, ent, tab, (const uint8_t*)nullptr,
                       (uint8_t*)nullptr, mx, (unsigned long long*)nullptr, (unsigned long long*)nullptr, cap, N,
                       r_threshold, threshold);
    DFW_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(tiles_cand_kernel<true>, grid, dim3(64, 4), 0, st, *plan, cells, ent, tab,
                     want_counts ? gt : (const uint8_t*)nullptr, labels, mx, (unsigned long long*)counts,
                     (unsigned long long*)area, cap, N, r_threshold, threshold);
  DFW_CHECK_LAUNCH();
  return 0;
}
