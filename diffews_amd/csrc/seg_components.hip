// Connected components of a label map (objects.label_objects): labels uint8 [B][H][W] -> ids int32 [B][H][W] numbered
// 1..n_b per image in row-major order of each component's first pixel, with per-object label / area / box rows, an
// optional minimum-area filter, the filtered label bytes, and seg_fuse.h's counts of the FILTERED bytes against a ground
// truth.  All integers: the result depends on no order of execution.
//
// Everything is a union-find over the pixel indices p = y * W + x of one image with the invariant parent[i] <= i, so the
// root of a set is its smallest index -- the component's first pixel.  The workspace is parent [B][HW] | area [B][HW] |
// blk [B][nblk][2], every word of it written before it is read (the caller initialises nothing).  Launches, a number fixed
// by the arguments (8, or 7 when the image is one tile), with no host readback in between:
//
//   0  seg_zero_launch       stats and counts (a library kernel, no memset node)
//   1  cc_tile_kernel        one workgroup per kCcTH x kCcTW tile: union-find of the tile in LDS.  Every pixel gets
//                            parent = its tile-local root (the tile-local component's smallest index, as a GLOBAL index; -1
//                            for background) and area = the tile-local component's pixel count at that local root, 0
//                            elsewhere.  Only local roots are ever linked from here on: a pixel is two hops from its root.
//   2  cc_merge_kernel       one thread per pixel on a tile's left column or top row: unions across the border with global
//                            atomicMin.  A pair that the pixel before it on the border already joins is skipped.
//   3  cc_flatten_kernel     every local root: parent = find (now the component's first pixel), and ONE atomicAdd of its
//                            tile-local count onto area[root] -- one atomic per (tile, local component), never per pixel
//   4  cc_count_kernel       per block of kCcTile consecutive pixels: roots, and roots with area >= min_area
//   5  cc_scan_kernel        one workgroup per image: exclusive scan of the block sums in place, n[b] = (kept, all)
//   6  cc_number_kernel      per block: the kept roots get id = offset + rank + 1, written over area[root] (0 for a removed
//                            root: the filter needs no cap); rows id <= cap of stats get label, area, the first pixel and
//                            that pixel as the initial box
//   7  cc_apply_kernel       one workgroup per tile: ids, filtered, the count histograms (seg_fuse.h's rule), and the box:
//                            x0 / y1 / x1 per tile-local component by LDS atomics, then one global atomicMin / atomicMax per
//                            (tile, local component) and field, only for ids <= cap (y0 is the first pixel's row)
//
// Launches 1 to 3, the grids' sizing and the argument why every loop ends are seg_unionfind.h's, shared with seg_holes.hip.
//
// keys (optional int32 [B][H][W], version 125): launches 1 and 2 are cc_tile_keyed_kernel / cc_merge_keyed_kernel, the same
// bodies comparing (byte, key) pairs; a pixel is a member by its byte alone, so numbering, filter, stats (the label column
// is the byte), counts, the launch count and the workspace are unchanged.
//
// seeds (version 125): the call is then the nearest-seed stage (validated here, launched by seg_nearest_launch, seg_boundary.hip) on map, seeds, nearest,
// dist, reach, passes and the workspace of dfw_seg_nearest_workspace_bytes; none of the launches above runs.
#include "common.h"
#include "seg_args.h"
#include "seg_fuse.h"
#include "seg_scan.h"
#include "seg_unionfind.h"

namespace dfw {

// id of the component of foreground pixel p once cc_number_kernel has run: a root holds it in area, a local root (area > 0)
// points at its root, every other pixel at its local root.
__device__ __forceinline__ int cc_id(const int32_t* parent, const int32_t* area, int p, int pa, int ar) {
  if (pa == p) return ar;
  if (ar != 0) return area[pa];
  return area[parent[pa]];
}

// The three union-find passes (seg_unionfind.h) on the label bytes themselves: equal non-zero bytes join.
__global__ __launch_bounds__(256) void cc_tile_kernel(const uint8_t* labels, int32_t* parent, int32_t* area, int H, int W,
                                                      int conn8) {
  cc_tile_body<cc_key_label>(labels, parent, area, H, W, conn8);
}

__global__ __launch_bounds__(256) void cc_merge_kernel(const uint8_t* labels, int32_t* parent, int H, int W, int ntx, int nty,
                                                       int conn8) {
  cc_merge_body<cc_key_label>(labels, parent, H, W, ntx, nty, conn8);
}

// ... and on (byte, key) pairs (version 125, `keys`): equal non-zero bytes with equal keys join.  Everything behind the
// merge reads parent and area only, so launches 3 to 7 are the keyless ones.
__global__ __launch_bounds__(256) void cc_tile_keyed_kernel(const uint8_t* labels, const int32_t* keys, int32_t* parent,
                                                            int32_t* area, int H, int W, int conn8) {
  cc_tile_body<cc_key_label, true>(labels, parent, area, H, W, conn8, keys);
}

__global__ __launch_bounds__(256) void cc_merge_keyed_kernel(const uint8_t* labels, const int32_t* keys, int32_t* parent, int H,
                                                             int W, int ntx, int nty, int conn8) {
  cc_merge_body<cc_key_label, true>(labels, parent, H, W, ntx, nty, conn8, keys);
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(int32_t* parent, int32_t* area, int HW) {
  cc_flatten_body(parent, area, HW);
}

// The 8 consecutive pixels of this thread in block blockIdx.x of the image: which are roots (bit j of *roots) and their
// areas.
__device__ __forceinline__ void cc_block_roots(const int32_t* P, const int32_t* A, int HW, int p0, unsigned* roots,
                                               int (&ar)[8]) {
  *roots = 0u;
  if (p0 + 8 <= HW && (((uintptr_t)(P + p0) | (uintptr_t)(A + p0)) & 15) == 0) {
    const i32x4 q0 = *(const i32x4*)(P + p0), q1 = *(const i32x4*)(P + p0 + 4);
    const int q[8] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3]};
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (q[j] == p0 + j) *roots |= 1u << j;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (p0 + j < HW && P[p0 + j] == p0 + j) *roots |= 1u << j;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) ar[j] = (*roots >> j) & 1u ? A[p0 + j] : 0;
}

__global__ __launch_bounds__(256) void cc_count_kernel(const int32_t* parent, const int32_t* area, int32_t* blk, int HW,
                                                       int min_area) {
  __shared__ int wk[4], wt[4];
  const size_t img = (size_t)blockIdx.y * HW;
  const int p0 = blockIdx.x * kCcTile + threadIdx.x * 8;
  unsigned roots;
  int ar[8];
  cc_block_roots(parent + img, area + img, HW, p0, &roots, ar);
  int kept = 0, all = __popc(roots);
#pragma unroll
  for (int j = 0; j < 8; ++j) kept += ((roots >> j) & 1u) && ar[j] >= min_area;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kept += __shfl_xor(kept, o, 64);
    all += __shfl_xor(all, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    wk[threadIdx.x >> 6] = kept;
    wt[threadIdx.x >> 6] = all;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t* o = blk + 2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
    o[0] = wk[0] + wk[1] + wk[2] + wk[3];
    o[1] = wt[0] + wt[1] + wt[2] + wt[3];
  }
}

// blk [b][nblk][2] = (kept, all) per block -> (kept before this block, all); n [b] = (kept, all) of the image
__global__ __launch_bounds__(256) void cc_scan_kernel(int32_t* blk, int32_t* n, int nblk) {
  __shared__ int wsum[4];
  int32_t* o = blk + 2 * (size_t)blockIdx.x * nblk;
  int ck = 0, ct = 0;
  for (int base = 0; base < nblk; base += 256) {
    const int i = base + threadIdx.x;
    const int k = i < nblk ? o[2 * i] : 0, t = i < nblk ? o[2 * i + 1] : 0;
    int sk, st;
    const int ek = block_scan(k, wsum, &sk);
    block_scan(t, wsum, &st);
    if (i < nblk) o[2 * i] = ck + ek;
    ck += sk;
    ct += st;
  }
  if (threadIdx.x == 0) {
    n[2 * blockIdx.x] = ck;
    n[2 * blockIdx.x + 1] = ct;
  }
}

__global__ __launch_bounds__(256) void cc_number_kernel(const uint8_t* labels, const int32_t* parent, int32_t* area,
                                                        const int32_t* blk, int32_t* stats, int HW, int W, int min_area,
                                                        int cap) {
  __shared__ int wsum[4];
  const size_t img = (size_t)blockIdx.y * HW;
  int32_t* A = area + img;
  const int p0 = blockIdx.x * kCcTile + threadIdx.x * 8;
  unsigned roots;
  int ar[8];
  cc_block_roots(parent + img, A, HW, p0, &roots, ar);
  int kept = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) kept += ((roots >> j) & 1u) && ar[j] >= min_area;
  int total;
  int id = blk[2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x)] + block_scan(kept, wsum, &total);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (!((roots >> j) & 1u)) continue;
    const int p = p0 + j;
    if (ar[j] < min_area) {
      A[p] = 0;
      continue;
    }
    A[p] = ++id;
    if (stats && id <= cap) {
      int32_t* row = stats + ((size_t)blockIdx.y * cap + (id - 1)) * 8;
      const int y = p / W, x = p - y * W;
      row[0] = labels[img + p];
      row[1] = ar[j];
      row[2] = y;
      row[3] = x;
      row[4] = y + 1;
      row[5] = x + 1;
      row[6] = p;
      row[7] = 0;
    }
  }
}

__global__ __launch_bounds__(256) void cc_apply_kernel(const uint8_t* labels, const int32_t* parent, const int32_t* area,
                                                       const uint8_t* gt, int32_t* ids, uint8_t* filtered, int32_t* stats,
                                                       unsigned long long* counts, int H, int W, int cap, int NLab) {
  __shared__ unsigned hist[3 * 256];     // seg_fuse_lds' [inter | pred | gt][label byte]
  __shared__ int bx0[kCcTile], by1[kCcTile], bx1[kCcTile];   // per tile-local root, tile coordinates; bx1 == 0: unused
  const int ty0 = blockIdx.y * kCcTH, tx0 = blockIdx.x * kCcTW;
  const size_t img = (size_t)blockIdx.z * H * W;
  const uint8_t* L = labels + img;
  const int32_t* P = parent + img;
  const int32_t* A = area + img;
  const uint8_t* G = gt ? gt + img : nullptr;
  int32_t* I = ids + img;
  uint8_t* F = filtered ? filtered + img : nullptr;
  int32_t* S = stats ? stats + (size_t)blockIdx.z * cap * 8 : nullptr;
  const bool vec = (W & 3) == 0 && (((uintptr_t)labels | (uintptr_t)filtered | (uintptr_t)gt) & 3) == 0 &&
                   (((uintptr_t)parent | (uintptr_t)area | (uintptr_t)ids) & 15) == 0;
  const seg_gt_byte map{NLab};
  for (int i = threadIdx.x; i < 3 * 256; i += 256) hist[i] = 0u;
  if (S)
    for (int i = threadIdx.x; i < kCcTile; i += 256) {
      bx0[i] = kCcTW;
      by1[i] = 0;
      bx1[i] = 0;
    }
  __syncthreads();
  const volatile int* vx0 = bx0;
  const volatile int* vy1 = by1;
  const volatile int* vx1 = bx1;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int w = threadIdx.x + 256 * k, ly = w >> 4, lx0 = (w & 15) * 4, y = ty0 + ly, x = tx0 + lx0;
    if (y >= H || x >= W) continue;
    const size_t o = (size_t)y * W + x;
    const int nj = vec ? 4 : min(4, W - x);
    uint32_t c4 = 0u, g4 = 0u;
    int pa[4] = {-1, -1, -1, -1}, ar[4] = {0, 0, 0, 0};
    if (vec) {
      c4 = *(const uint32_t*)(L + o);
      if (G) g4 = *(const uint32_t*)(G + o);
      const i32x4 q = *(const i32x4*)(P + o), a = *(const i32x4*)(A + o);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pa[j] = q[j];
        ar[j] = a[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nj) {
          c4 |= (uint32_t)L[o + j] << (8 * j);
          if (G) g4 |= (uint32_t)G[o + j] << (8 * j);
          pa[j] = P[o + j];
          ar[j] = A[o + j];
        }
    }
    int id[4];
    uint32_t f4 = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t c = (c4 >> (8 * j)) & 255u;
      const int p = (int)o + j;
      id[j] = (j < nj && c != 0u) ? cc_id(P, A, p, pa[j], ar[j]) : 0;
      const uint32_t f = id[j] ? c : 0u;
      f4 |= f << (8 * j);
      if (j < nj && G) {
        const int g = map((int)((g4 >> (8 * j)) & 255u));
        if (g >= 0) {
          atomicAdd(&hist[256 + f], 1u);
          atomicAdd(&hist[512 + g], 1u);
          if ((int)f == g) atomicAdd(&hist[f], 1u);
        }
      }
      if (S && id[j] >= 1 && id[j] <= cap) {
        // the slot of this pixel's tile-local root: the pixel itself when it is one, else its parent (inside the tile)
        int key = 4 * w + j;
        if (pa[j] != p && ar[j] == 0) {
          const int qy = pa[j] / W, qx = pa[j] - qy * W;
          key = (qy - ty0) * kCcTW + (qx - tx0);
        }
        if ((unsigned)key < (unsigned)kCcTile) {
          const int lx = lx0 + j;
          if (lx < vx0[key]) atomicMin(&bx0[key], lx);
          if (ly + 1 > vy1[key]) atomicMax(&by1[key], ly + 1);
          if (lx + 1 > vx1[key]) atomicMax(&bx1[key], lx + 1);
        }
      }
    }
    if (vec) {
      *(i32x4*)(I + o) = i32x4{id[0], id[1], id[2], id[3]};
      if (F) *(uint32_t*)(F + o) = f4;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nj) {
          I[o + j] = id[j];
          if (F) F[o + j] = (uint8_t)(f4 >> (8 * j));
        }
    }
  }
  __syncthreads();
  if (G) seg_flush_counts(hist, counts + (size_t)blockIdx.z * 2 * (NLab + 1), NLab + 1);
  if (S)
    for (int l = threadIdx.x; l < kCcTile; l += 256) {
      if (bx1[l] == 0) continue;
      const int p = (ty0 + (l >> 6)) * W + tx0 + (l & (kCcTW - 1));
      const int id = cc_id(P, A, p, P[p], A[p]);
      if (id < 1 || id > cap) continue;
      int32_t* row = S + (size_t)(id - 1) * 8;
      atomicMin(row + 3, tx0 + bx0[l]);
      atomicMax(row + 4, ty0 + by1[l]);
      atomicMax(row + 5, tx0 + bx1[l]);
    }
}

// cc_scan_kernel: 256 block sums a round, one workgroup per image.
inline int cc_scan_rounds(int nblk) { return (nblk + 255) / 256; }
inline int cc_grid_rounds(long long items, int gx) { return gx < 1 ? 0 : (int)((items + 256ll * gx - 1) / (256ll * gx)); }

}  // namespace dfw

using namespace dfw;

extern "C" size_t dfw_seg_components_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  const long long HW = (long long)H * W;
  return (size_t)B * ((size_t)HW * 8 + cc_blocks(HW) * 8);
}

extern "C" int dfw_seg_components_tile(int32_t* tile_h, int32_t* tile_w) {
  if (!tile_h || !tile_w) return DFW_EINVAL;
  *tile_h = kCcTH;
  *tile_w = kCcTW;
  return 0;
}

extern "C" int dfw_seg_components_rounds(int32_t B, int32_t H, int32_t W, const void* ws,
                                         dfw_seg_components_rounds_out* out) {
  if (!out || !ws) return DFW_EINVAL;
  if (int e = seg_map_size_error(B, H, W)) return e;
  if ((uintptr_t)ws & 3) return DFW_ESHAPE;
  const int HW = H * W, nblk = (int)cc_blocks(HW);
  const long long items = cc_merge_items(H, W);
  // the address of the area plane behind parent [B][HW]; ws is never dereferenced, so it is an integer here
  const uintptr_t area = (uintptr_t)ws + (uintptr_t)B * (uintptr_t)HW * 4;
  out->blocks = nblk;
  out->merge = cc_grid_rounds(items, items > 0 ? cc_merge_grid(items) : 0);
  out->flatten_vector = cc_flatten_vector(HW, area);
  out->flatten = cc_grid_rounds(out->flatten_vector ? HW / 4 : HW, cc_flatten_grid(HW));
  out->scan = cc_scan_rounds(nblk);
  return 0;
}

extern "C" int dfw_seg_components(const dfw_seg_components_args* a, dfw_stream_t stream) {
  if (a && a->seeds) {                                     // the nearest-seed stage: its own fields, its own checks
    if (!a->map || !a->nearest || !a->dist || !a->ws) return DFW_EINVAL;
    if (a->reach < 1 || a->reach > 254) return DFW_EINVAL;
    if (a->passes < 1 || a->passes > 8) return DFW_EINVAL;
    if (int e = seg_map_size_error(a->B, a->H, a->W)) return e;
    const size_t wsb = dfw_seg_nearest_workspace_bytes(a->B, a->H, a->W);
    if (a->ws_bytes < wsb) return DFW_EWORKSPACE;
    const size_t px = (size_t)a->B * a->H * a->W;
    const seg_buf bufs[] = {seg_in(a->map, px * 4, 4), seg_in(a->seeds, px * 4, 4), seg_out(a->dist, px * 2, 2),
                            seg_out(a->ws, wsb, 4), seg_out(a->nearest, px * 4, 4)};
    if (int e = seg_check_buffers(bufs)) return e;
    return seg_nearest_launch(a, stream);
  }
  if (!a || !a->labels || !a->ids || !a->n || !a->ws) return DFW_EINVAL;
  if (a->B < 1 || a->H < 1 || a->W < 1) return DFW_EINVAL;
  if (a->connectivity != 4 && a->connectivity != 8) return DFW_EINVAL;
  if (a->min_area < 0) return DFW_EINVAL;
  if (a->stats && a->cap < 1) return DFW_EINVAL;
  if (a->counts && !a->gt) return DFW_EINVAL;
  if (a->gt && (a->nlabels < 1 || a->nlabels > 254)) return DFW_EINVAL;
  if (a->nearest) return DFW_EINVAL;                       // nearest without seeds
  if (int e = seg_map_size_error(a->B, a->H, a->W)) return e;
  if (a->stats && (long long)a->B * a->cap * 8 > 0x7fffffffll) return DFW_ERANGE;   // seg_zero_launch counts in int
  if (a->ws_bytes < dfw_seg_components_workspace_bytes(a->B, a->H, a->W)) return DFW_EWORKSPACE;
  const int B = a->B, H = a->H, W = a->W, HW = H * W, conn8 = a->connectivity == 8;
  const size_t px = (size_t)B * HW;
  const seg_buf bufs[] = {seg_in(a->labels, px),
                          seg_in(a->counts ? a->gt : nullptr, px),
                          seg_out(a->ids, px * 4, 4),
                          seg_out(a->n, (size_t)B * 8, 4),
                          seg_out(a->filtered, px),
                          seg_out(a->stats, (size_t)B * a->cap * 32, 4),
                          seg_out(a->counts, (size_t)B * 2 * (a->nlabels + 1) * 8, 8),
                          seg_out(a->ws, dfw_seg_components_workspace_bytes(B, H, W), 4),
                          seg_in(a->keys, px * 4, 4)};
  if (int e = seg_check_buffers(bufs)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int ntx = (W + kCcTW - 1) / kCcTW, nty = (H + kCcTH - 1) / kCcTH, nblk = (int)cc_blocks(HW);
  int32_t* parent = (int32_t*)a->ws;
  int32_t* area = parent + (size_t)B * HW;
  int32_t* blk = area + (size_t)B * HW;
  const bool want_counts = a->gt && a->counts;
  if (int e = seg_zero_launch(st, (uint32_t*)a->stats, a->stats ? B * a->cap * 8 : 0, want_counts ? a->counts : nullptr,
                              want_counts ? B * 2 * (a->nlabels + 1) : 0))
    return e;
  if (a->keys)
    hipLaunchKernelGGL(cc_tile_keyed_kernel, dim3(ntx, nty, B), dim3(256), 0, st, a->labels, a->keys, parent, area, H, W,
                       conn8);
  else
    hipLaunchKernelGGL(cc_tile_kernel, dim3(ntx, nty, B), dim3(256), 0, st, a->labels, parent, area, H, W, conn8);
  DFW_CHECK_LAUNCH();
  const long long items = cc_merge_items(H, W);
  if (items > 0) {
    if (a->keys)
      hipLaunchKernelGGL(cc_merge_keyed_kernel, dim3(cc_merge_grid(items), B), dim3(256), 0, st, a->labels, a->keys, parent, H,
                         W, ntx, nty, conn8);
    else
      hipLaunchKernelGGL(cc_merge_kernel, dim3(cc_merge_grid(items), B), dim3(256), 0, st, a->labels, parent, H, W, ntx, nty,
                         conn8);
    DFW_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(cc_flatten_grid(HW), B), dim3(256), 0, st, parent, area, HW);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_count_kernel, dim3(nblk, B), dim3(256), 0, st, (const int32_t*)parent, (const int32_t*)area, blk, HW,
                     a->min_area);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_scan_kernel, dim3(B), dim3(256), 0, st, blk, a->n, nblk);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_number_kernel, dim3(nblk, B), dim3(256), 0, st, a->labels, (const int32_t*)parent, area,
                     (const int32_t*)blk, a->stats, HW, W, a->min_area, a->cap);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_apply_kernel, dim3(ntx, nty, B), dim3(256), 0, st, a->labels, (const int32_t*)parent,
                     (const int32_t*)area, want_counts ? a->gt : nullptr, a->ids, a->filtered, a->stats,
                     (unsigned long long*)a->counts, H, W, a->cap, a->nlabels);
  DFW_CHECK_LAUNCH();
  return 0;
}
