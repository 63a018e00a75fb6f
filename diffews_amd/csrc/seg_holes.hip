// Filling the holes of labelled objects (objects.fill_holes): labels uint8 [B][H][W] and ids int32 [B][H][W], normally
// dfw_seg_components' filtered and ids, -> labels_out / ids_out in which every background region that one object
// encloses has taken that object's id and label byte.  The definition is include/diffews_hip.h's.  All integers: the
// result depends on no order of execution.
//
// A hole is a connected component of the BACKGROUND under the dual connectivity hc (4 for objects joined over 8
// neighbours, 8 for objects joined over 4), so the three union-find passes of seg_unionfind.h run on the zero bytes
// (cc_key_zero).  The workspace is parent [B][HW] | area [B][HW], every word of it written before it is read (the caller
// initialises nothing).  Behind the flatten pass a background pixel is two hops from its region's first pixel, the root,
// and area[root] is the region's pixel count.  From there area[root] doubles as the region's state:
//
//   > 0          enclosed, and no reason against filling found so far: the area
//   kHoleOpen    the region touches the image frame
//   kHoleKept    enclosed, but not filled: owner < 1, a border pixel of another id, or an area above max_area
//
// Launches, a number fixed by the arguments (6, or 5 when the image is one tile), with no host readback in between:
//
//   0  sh_tile_kernel      seg_unionfind.h's tile pass on the zero bytes
//   1  sh_merge_kernel     its border merge
//   2  sh_flatten_kernel   its flatten pass
//   3  sh_prepare_kernel   one thread per frame pixel: a background pixel stores kHoleOpen at its root.  The same grid zeroes
//                          holes and counts and copies stats to stats_out (no memset node, no copy node)
//   4  sh_classify_kernel  one workgroup per tile.  Every background pixel of a region that launch 3 left enclosed -- decided
//                          BEFORE the owner is read: the first pixel of a region on column 0 has no left neighbour -- compares
//                          the ids of the non-background pixels in its hc-neighbourhood with the owner, ids[root - 1]; the
//                          root also checks owner >= 1 and area <= max_area.  Whoever finds a reason stores kHoleKept at the
//                          root: one value, from however many pixels, read in the next launch -- no atomic, no hand-off
//   5  sh_apply_kernel     one workgroup per tile: ids_out, labels_out, the count histograms (seg_fuse.h's rule) through LDS,
//                          the filled pixels per tile-local region in LDS and then one global atomicAdd per (tile, tile-local
//                          region) and field onto the owner's row of stats_out, and holes by one atomicAdd per tile and field
//
// No kernel of 3 to 5 loops over a capped grid.  Termination of 0 to 2: seg_unionfind.h.  No thread waits for another.
#include "common.h"
#include "seg_args.h"
#include "seg_fuse.h"
#include "seg_unionfind.h"

namespace dfw {

constexpr int kHoleOpen = -1, kHoleKept = -2;

__global__ __launch_bounds__(256) void sh_tile_kernel(const uint8_t* labels, int32_t* parent, int32_t* area, int H, int W,
                                                      int conn8) {
  cc_tile_body<cc_key_zero>(labels, parent, area, H, W, conn8);
}

__global__ __launch_bounds__(256) void sh_merge_kernel(const uint8_t* labels, int32_t* parent, int H, int W, int ntx, int nty,
                                                       int conn8) {
  cc_merge_body<cc_key_zero>(labels, parent, H, W, ntx, nty, conn8);
}

__global__ __launch_bounds__(256) void sh_flatten_kernel(int32_t* parent, int32_t* area, int HW) {
  cc_flatten_body(parent, area, HW);
}

// The root of background pixel p behind the flatten pass; pa = parent[p], ar = area[p], which is only looked at when p is
// no root (a root's area word is the region's state): a local root (ar > 0) points at the root, every other pixel at its
// local root.
__device__ __forceinline__ int sh_root(const int32_t* P, int p, int pa, int ar) {
  if (pa == p) return p;
  if (ar > 0) return pa;
  return P[pa];
}

// The slot of pixel p's tile-local root in its tile: the pixel itself when it is one (slot), else its parent.
__device__ __forceinline__ int sh_local_slot(int p, int pa, int ar, int slot, int W, int ty0, int tx0) {
  if (pa == p || ar > 0) return slot;
  const int qy = pa / W, qx = pa - qy * W;
  return (qy - ty0) * kCcTW + (qx - tx0);
}

// grid (max(frame, stats, counts items) / 256, B).  Frame items of an image: row 0, row H - 1, column 0, column W - 1
// (the corners twice: the store is idempotent).
__global__ __launch_bounds__(256) void sh_prepare_kernel(const uint8_t* labels, const int32_t* parent, int32_t* area,
                                                         const int32_t* stats, int32_t* stats_out, int32_t* holes,
                                                         unsigned long long* counts, int H, int W, int cap, int ncounts) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (t < 2) holes[2 * b + t] = 0;
  if (counts && t < ncounts) counts[(size_t)b * ncounts + t] = 0ull;
  if (stats_out && t < (long long)cap * 8) stats_out[(size_t)b * cap * 8 + t] = stats[(size_t)b * cap * 8 + t];
  if (t >= 2ll * W + 2ll * H) return;
  int y, x;
  if (t < W) {
    y = 0, x = (int)t;
  } else if (t < 2ll * W) {
    y = H - 1, x = (int)(t - W);
  } else if (t < 2ll * W + H) {
    y = (int)(t - 2ll * W), x = 0;
  } else {
    y = (int)(t - 2ll * W - H), x = W - 1;
  }
  const size_t img = (size_t)b * H * W;
  const int p = y * W + x;
  if (labels[img + p] != 0) return;
  const int32_t* P = parent + img;
  int32_t* A = area + img;
  const int pa = P[p];
  const int root = sh_root(P, p, pa, pa == p ? 0 : A[p]);
  A[root] = kHoleOpen;
}

__global__ __launch_bounds__(256) void sh_classify_kernel(const uint8_t* labels, const int32_t* ids, const int32_t* parent,
                                                          int32_t* area, int H, int W, int hc8, int max_area) {
  const int ty0 = blockIdx.y * kCcTH, tx0 = blockIdx.x * kCcTW;
  const size_t img = (size_t)blockIdx.z * H * W;
  const uint8_t* L = labels + img;
  const int32_t* I = ids + img;
  const int32_t* P = parent + img;
  int32_t* A = area + img;
  const bool vec = (W & 3) == 0 && ((uintptr_t)labels & 3) == 0 && (((uintptr_t)parent | (uintptr_t)area) & 15) == 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int w = threadIdx.x + 256 * k, y = ty0 + (w >> 4), x = tx0 + (w & 15) * 4;
    if (y >= H || x >= W) continue;
    const size_t o = (size_t)y * W + x;
    const int nj = vec ? 4 : min(4, W - x);
    uint32_t c4 = 0xffffffffu;
    int pa[4] = {-1, -1, -1, -1}, ar[4] = {0, 0, 0, 0};
    if (vec) {
      c4 = *(const uint32_t*)(L + o);
      if (cc_key_zero::word(c4) == 0u) continue;          // no background pixel among the four
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
          c4 = (c4 & ~(255u << (8 * j))) | ((uint32_t)L[o + j] << (8 * j));
          pa[j] = P[o + j];
          ar[j] = A[o + j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= nj || ((c4 >> (8 * j)) & 255u) != 0u) continue;
      const int xx = x + j, p = (int)o + j;
      // a pixel on the frame: its region is open, and it has no full neighbourhood
      if (y == 0 || y == H - 1 || xx == 0 || xx == W - 1) continue;
      const int root = sh_root(P, p, pa[j], ar[j]);
      const int state = root == p ? ar[j] : A[root];
      if (state < 0) continue;                            // open, or kept already
      // enclosed: the root is not on column 0, so root - 1 is its left neighbour, a pixel of an object
      int owner = 0;
      bool have = false, keep = false;
      if (root == p) {
        owner = I[root - 1];
        have = true;
        keep = owner < 1 || state > max_area;
      }
      auto look = [&](int q) {
        if (L[q] == 0) return;
        if (!have) {
          owner = I[root - 1];
          have = true;
        }
        keep = keep || I[q] != owner;
      };
      look(p - 1);
      look(p + 1);
      look(p - W);
      look(p + W);
      if (hc8) {
        look(p - W - 1);
        look(p - W + 1);
        look(p + W - 1);
        look(p + W + 1);
      }
      if (keep) A[root] = kHoleKept;
    }
  }
}

__global__ __launch_bounds__(256) void sh_apply_kernel(const uint8_t* labels, const int32_t* ids, const int32_t* parent,
                                                       const int32_t* area, const uint8_t* gt, int32_t* ids_out,
                                                       uint8_t* labels_out, int32_t* holes, int32_t* stats_out,
                                                       unsigned long long* counts, int H, int W, int cap, int NLab) {
  __shared__ unsigned hist[3 * 256];     // seg_fuse_lds' [inter | pred | gt][label byte]
  __shared__ int fill[kCcTile];          // filled pixels per tile-local root of a background region
  __shared__ int nholes[2];              // (filled, enclosed) roots of this tile
  const int ty0 = blockIdx.y * kCcTH, tx0 = blockIdx.x * kCcTW;
  const size_t img = (size_t)blockIdx.z * H * W;
  const uint8_t* L = labels + img;
  const int32_t* I = ids + img;
  const int32_t* P = parent + img;
  const int32_t* A = area + img;
  const uint8_t* G = gt ? gt + img : nullptr;
  int32_t* IO = ids_out + img;
  uint8_t* LO = labels_out + img;
  int32_t* S = stats_out ? stats_out + (size_t)blockIdx.z * cap * 8 : nullptr;
  const bool vec = (W & 3) == 0 && (((uintptr_t)labels | (uintptr_t)labels_out | (uintptr_t)gt) & 3) == 0 &&
                   (((uintptr_t)parent | (uintptr_t)area | (uintptr_t)ids | (uintptr_t)ids_out) & 15) == 0;
  const seg_gt_byte map{NLab};
  if (G)
    for (int i = threadIdx.x; i < 3 * 256; i += 256) hist[i] = 0u;
  if (S)
    for (int i = threadIdx.x; i < kCcTile; i += 256) fill[i] = 0;
  if (threadIdx.x < 2) nholes[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int w = threadIdx.x + 256 * k, y = ty0 + (w >> 4), x = tx0 + (w & 15) * 4;
    if (y >= H || x >= W) continue;
    const size_t o = (size_t)y * W + x;
    const int nj = vec ? 4 : min(4, W - x);
    uint32_t c4 = 0u, g4 = 0u;
    int id[4] = {0, 0, 0, 0}, pa[4] = {-1, -1, -1, -1}, ar[4] = {0, 0, 0, 0};
    if (vec) {
      c4 = *(const uint32_t*)(L + o);
      if (G) g4 = *(const uint32_t*)(G + o);
      const i32x4 v = *(const i32x4*)(I + o);
#pragma unroll
      for (int j = 0; j < 4; ++j) id[j] = v[j];
      if (cc_key_zero::word(c4) != 0u) {
        const i32x4 q = *(const i32x4*)(P + o), a = *(const i32x4*)(A + o);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          pa[j] = q[j];
          ar[j] = a[j];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nj) {
          c4 |= (uint32_t)L[o + j] << (8 * j);
          if (G) g4 |= (uint32_t)G[o + j] << (8 * j);
          id[j] = I[o + j];
          pa[j] = P[o + j];
          ar[j] = A[o + j];
        }
    }
    uint32_t f4 = c4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= nj) continue;
      uint32_t f = (c4 >> (8 * j)) & 255u;
      if (f == 0u) {
        const int p = (int)o + j;
        const int root = sh_root(P, p, pa[j], ar[j]);
        const int state = root == p ? ar[j] : A[root];
        if (root == p && state != kHoleOpen) {
          atomicAdd(&nholes[1], 1);
          if (state > 0) atomicAdd(&nholes[0], 1);
        }
        if (state > 0) {
          id[j] = I[root - 1];
          f = L[root - 1];
          f4 |= f << (8 * j);
          if (S && id[j] >= 1 && id[j] <= cap) {
            const int slot = sh_local_slot(p, pa[j], ar[j], 4 * w + j, W, ty0, tx0);
            if ((unsigned)slot < (unsigned)kCcTile) atomicAdd(&fill[slot], 1);
          }
        }
      }
      if (G) {
        const int g = map((int)((g4 >> (8 * j)) & 255u));
        if (g >= 0) {
          atomicAdd(&hist[256 + f], 1u);
          atomicAdd(&hist[512 + g], 1u);
          if ((int)f == g) atomicAdd(&hist[f], 1u);
        }
      }
    }
    if (vec) {
      *(i32x4*)(IO + o) = i32x4{id[0], id[1], id[2], id[3]};
      *(uint32_t*)(LO + o) = f4;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nj) {
          IO[o + j] = id[j];
          LO[o + j] = (uint8_t)(f4 >> (8 * j));
        }
    }
  }
  __syncthreads();
  if (G) seg_flush_counts(hist, counts + (size_t)blockIdx.z * 2 * (NLab + 1), NLab + 1);
  if (threadIdx.x < 2 && nholes[threadIdx.x] != 0) atomicAdd(holes + 2 * blockIdx.z + threadIdx.x, nholes[threadIdx.x]);
  if (S)
    for (int l = threadIdx.x; l < kCcTile; l += 256) {
      const int n = fill[l];
      if (n == 0) continue;
      // slot l is a tile-local root of a filled region: the root itself, or one hop from it
      const int p = (ty0 + (l >> 6)) * W + tx0 + (l & (kCcTW - 1));
      const int root = P[p];
      if (root < 1 || root > p) continue;
      const int id = I[root - 1];
      if (id < 1 || id > cap) continue;
      int32_t* row = S + (size_t)(id - 1) * 8;
      atomicAdd(row + 1, n);
      atomicAdd(row + 7, n);
    }
}

}  // namespace dfw

using namespace dfw;

extern "C" size_t dfw_seg_holes_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  if (seg_map_size_error(B, H, W)) return 0;
  return (size_t)B * (size_t)H * (size_t)W * 8;
}

extern "C" int dfw_seg_holes(const dfw_seg_holes_args* a, dfw_stream_t stream) {
  if (!a || !a->labels || !a->ids || !a->ids_out || !a->labels_out || !a->holes || !a->ws) return DFW_EINVAL;
  if (a->B < 1 || a->H < 1 || a->W < 1) return DFW_EINVAL;
  if (a->connectivity != 4 && a->connectivity != 8) return DFW_EINVAL;
  if (a->max_area < 0) return DFW_EINVAL;
  if (a->stats_out && (!a->stats || a->cap < 1)) return DFW_EINVAL;
  if (a->counts && !a->gt) return DFW_EINVAL;
  if (a->gt && (a->nlabels < 1 || a->nlabels > 254)) return DFW_EINVAL;
  if (int e = seg_map_size_error(a->B, a->H, a->W)) return e;
  if (a->stats_out && (long long)a->B * a->cap * 8 > 0x7fffffffll) return DFW_ERANGE;
  if (a->ws_bytes < dfw_seg_holes_workspace_bytes(a->B, a->H, a->W)) return DFW_EWORKSPACE;
  const int B = a->B, H = a->H, W = a->W, HW = H * W;
  const bool want_counts = a->gt && a->counts, want_stats = a->stats_out != nullptr;
  const size_t px = (size_t)B * HW, sb = want_stats ? (size_t)B * a->cap * 32 : 0;   // stats only with stats_out
  const seg_buf bufs[] = {seg_in(a->labels, px),
                          seg_in(a->ids, px * 4, 4),
                          seg_in(a->stats, sb, 4),
                          seg_in(a->gt, px),
                          seg_out(a->ids_out, px * 4, 4),
                          seg_out(a->labels_out, px),
                          seg_out(a->holes, (size_t)B * 8, 4),
                          seg_out(a->stats_out, sb, 4),
                          seg_out(a->counts, (size_t)B * 2 * (a->nlabels + 1) * 8, 8),
                          seg_out(a->ws, px * 8, 4)};
  if (int e = seg_check_buffers(bufs)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int hc8 = a->connectivity == 4;                  // the dual of the objects' connectivity
  const int ntx = (W + kCcTW - 1) / kCcTW, nty = (H + kCcTH - 1) / kCcTH;
  int32_t* parent = (int32_t*)a->ws;
  int32_t* area = parent + (size_t)B * HW;
  hipLaunchKernelGGL(sh_tile_kernel, dim3(ntx, nty, B), dim3(256), 0, st, a->labels, parent, area, H, W, hc8);
  DFW_CHECK_LAUNCH();
  const long long items = cc_merge_items(H, W);
  if (items > 0) {
    hipLaunchKernelGGL(sh_merge_kernel, dim3(cc_merge_grid(items), B), dim3(256), 0, st, a->labels, parent, H, W, ntx, nty,
                       hc8);
    DFW_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(sh_flatten_kernel, dim3(cc_flatten_grid(HW), B), dim3(256), 0, st, parent, area, HW);
  DFW_CHECK_LAUNCH();
  const int ncounts = want_counts ? 2 * (a->nlabels + 1) : 0;
  long long prep = 2ll * W + 2ll * H;
  if (want_stats && (long long)a->cap * 8 > prep) prep = (long long)a->cap * 8;
  if (ncounts > prep) prep = ncounts;
  hipLaunchKernelGGL(sh_prepare_kernel, dim3((unsigned)((prep + 255) / 256), B), dim3(256), 0, st, a->labels,
                     (const int32_t*)parent, area, want_stats ? a->stats : nullptr, a->stats_out, a->holes,
                     want_counts ? (unsigned long long*)a->counts : nullptr, H, W, a->cap, ncounts);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(sh_classify_kernel, dim3(ntx, nty, B), dim3(256), 0, st, a->labels, a->ids, (const int32_t*)parent, area,
                     H, W, hc8, a->max_area);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(sh_apply_kernel, dim3(ntx, nty, B), dim3(256), 0, st, a->labels, a->ids, (const int32_t*)parent,
                     (const int32_t*)area, want_counts ? a->gt : nullptr, a->ids_out, a->labels_out, a->holes, a->stats_out,
                     (unsigned long long*)a->counts, H, W, a->cap, a->nlabels);
  DFW_CHECK_LAUNCH();
  return 0;
}
