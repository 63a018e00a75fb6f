// The union-find over the pixels of an image that seg_components.hip (objects: equal non-zero bytes join) and
// seg_holes.hip (background regions: zero bytes join) share: the tile pass in LDS, the border merge by global atomicMin and
// the flatten pass, as bodies that the thin __global__ kernels of the two files call, with the grids' sizing and the size
// limits of both calls.
//
// What is joined is a Key: byte() maps a label byte to the byte the passes compare -- 0 = not a member of any set, equal
// non-zero keys join -- and word() does the same on four bytes of a 32-bit word.  cc_key_label is the identity;
// cc_key_zero gives 1 for a zero byte and 0 for every other one.  A pixel outside the image is never a member.
//
// Invariant: parent[i] <= i, so the root of a set is its smallest index -- the set's first pixel.  Behind the three passes
// parent is -1 for a pixel that is no member, a set's first pixel for every tile-local root, and the tile-local root for
// every other pixel: a pixel is two hops from its root.  area holds the set's pixel count at the root, the tile-local count
// (> 0) at every other tile-local root and 0 elsewhere.
//
// A second plane (template parameter K, seg_components with `keys`): int32 keys [B][H][W], compared for equality only.  Two
// neighbouring members then join when their bytes AND their keys are equal; membership is still the byte's alone.  The
// tile pass keeps the keys of its pixels in LDS (8 KB more).  The shortcut "upper diagonals only where the upper pixel
// differs" holds for the combined comparison as it stands: an upper pixel that is equal in both parts is joined to every
// diagonal neighbour that is equal to this pixel in both parts, by that neighbour's own left or this pixel's upper union.
// With K = false nothing of it is compiled: the bodies are the keyless ones.
//
// Termination: no thread waits for another thread or workgroup.  Every loop is a find, which reads strictly decreasing
// indices (it stops at any word that is not smaller than the index it was read at, so even a damaged workspace cannot send
// it round or outside), or a union's retry, where a failed atomicMin replaces the larger root by a strictly smaller index.
// A find may read a stale parent (another CU's L1, another XCD's L2): that is an older ancestor of the same set, and the
// atomicMin on the word itself returns the truth, so a stale read costs a round, never a wrong link.
#pragma once
#include "common.h"

namespace dfw {

constexpr int kCcTH = 32, kCcTW = 64, kCcTile = kCcTH * kCcTW;   // 2048 pixels, 8 per thread of 256
constexpr int kCcWords = kCcTile / 4;

struct cc_key_label {
  static __device__ __forceinline__ uint8_t byte(uint8_t c) { return c; }
  static __device__ __forceinline__ uint32_t word(uint32_t v) { return v; }
};
struct cc_key_zero {
  static __device__ __forceinline__ uint8_t byte(uint8_t c) { return c == 0; }
  // 0x01 in every byte of v that is zero: bit 7 of (low seven bits + 0x7f) | v is clear only for a zero byte
  static __device__ __forceinline__ uint32_t word(uint32_t v) {
    return (~(((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v | 0x7f7f7f7fu)) >> 7;
  }
};

// ---- union-find in LDS ----
__device__ __forceinline__ int lds_find(const volatile int* par, int i) {
  for (;;) {
    const int p = par[i];
    if ((unsigned)p >= (unsigned)i) return i;
    i = p;
  }
}
__device__ __forceinline__ void lds_union(int* par, int a, int b) {
  for (;;) {
    a = lds_find(par, a);
    b = lds_find(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&par[a], b);
    if (old == a) return;
    a = old;                             // somebody linked a first: old < a, go on from there
  }
}

// ---- union-find in global memory ----
__device__ __forceinline__ int g_find(const int32_t* par, int i) {
  for (;;) {
    const int p = __hip_atomic_load(par + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((unsigned)p >= (unsigned)i) return i;
    i = p;
  }
}
__device__ __forceinline__ void g_union(int32_t* par, int a, int b) {
  for (;;) {
    a = g_find(par, a);
    b = g_find(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&par[a], b);
    if (old == a) return;
    a = old;
  }
}

// One workgroup of 256 per kCcTH x kCcTW tile, grid (ntx, nty, B): union-find of the tile in LDS.  Every pixel gets parent
// = its tile-local root (the tile-local set's smallest index, as a GLOBAL index; -1 for a pixel that is no member) and area
// = the tile-local set's pixel count at that local root, 0 elsewhere.
template <class Key, bool K = false>
__device__ __forceinline__ void cc_tile_body(const uint8_t* labels, int32_t* parent, int32_t* area, int H, int W, int conn8,
                                             const int32_t* keys = nullptr) {
  __shared__ uint32_t lab4[kCcWords];
  __shared__ int par[kCcTile];
  __shared__ int cnt[kCcTile];
  __shared__ __attribute__((aligned(16))) int kk[K ? kCcTile : 4];   // the keys of the tile's pixels, K only
  const uint8_t* lab = (const uint8_t*)lab4;
  const int ty0 = blockIdx.y * kCcTH, tx0 = blockIdx.x * kCcTW;
  const size_t img = (size_t)blockIdx.z * H * W;
  const uint8_t* L = labels + img;
  int32_t* P = parent + img;
  int32_t* A = area + img;
  const bool vec = (W & 3) == 0 && ((uintptr_t)labels & 3) == 0 && (((uintptr_t)parent | (uintptr_t)area) & 15) == 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int w = threadIdx.x + 256 * k, y = ty0 + (w >> 4), x = tx0 + (w & 15) * 4;
    uint32_t v = 0u;
    if (y < H) {
      const size_t o = (size_t)y * W + x;
      if (vec) {
        if (x < W) v = Key::word(*(const uint32_t*)(L + o));
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x + j < W) v |= (uint32_t)Key::byte(L[o + j]) << (8 * j);
      }
    }
    lab4[w] = v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      par[4 * w + j] = 4 * w + j;
      cnt[4 * w + j] = 0;
    }
    if constexpr (K) {
      const int32_t* Q = keys + img;
      const size_t o = (size_t)y * W + x;
      if (y < H && x < W && vec && ((uintptr_t)keys & 15) == 0) {
        *(i32x4*)(kk + 4 * w) = *(const i32x4*)(Q + o);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) kk[4 * w + j] = (y < H && x + j < W) ? Q[o + j] : 0;
      }
    }
  }
  __syncthreads();
  // equal in the byte (c, this pixel's, non-zero) and, with keys, in the key
  auto same = [&](int l, int m, uint8_t c) -> bool {
    if constexpr (K) return lab[m] == c && kk[m] == kk[l];
    else return lab[m] == c;
  };
  // a pixel joins its left and upper neighbour; with 8 neighbours the two upper diagonals only where the upper one is
  // another byte, or another key (else they reach this pixel through it)
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int w = threadIdx.x + 256 * k, ly = w >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int l = 4 * w + j, lx = l & (kCcTW - 1);
      const uint8_t c = lab[l];
      if (c == 0) continue;
      if (lx > 0 && same(l, l - 1, c)) lds_union(par, l, l - 1);
      if (ly > 0) {
        if (same(l, l - kCcTW, c)) {
          lds_union(par, l, l - kCcTW);
        } else if (conn8) {
          if (lx > 0 && same(l, l - kCcTW - 1, c)) lds_union(par, l, l - kCcTW - 1);
          if (lx < kCcTW - 1 && same(l, l - kCcTW + 1, c)) lds_union(par, l, l - kCcTW + 1);
        }
      }
    }
  }
  __syncthreads();
  int root[2][4];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int w = threadIdx.x + 256 * k;
#pragma unroll
    for (int j = 0; j < 4; ++j) root[k][j] = lab[4 * w + j] ? lds_find(par, 4 * w + j) : -1;
    // one LDS atomic per run of equal roots among the four
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (root[k][j] < 0 || (j > 0 && root[k][j - 1] == root[k][j])) continue;
      int n = 1;
      bool run = true;
#pragma unroll
      for (int i = 1; i < 4; ++i)
        if (j + i < 4) {
          run = run && root[k][j + i] == root[k][j];
          n += run;
        }
      atomicAdd(&cnt[root[k][j]], n);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int w = threadIdx.x + 256 * k, y = ty0 + (w >> 4), x = tx0 + (w & 15) * 4;
    if (y >= H || x >= W) continue;
    int gp[4], ga[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = root[k][j];
      gp[j] = r < 0 ? -1 : (ty0 + (r >> 6)) * W + tx0 + (r & (kCcTW - 1));
      ga[j] = r == 4 * w + j ? cnt[r] : 0;
    }
    const size_t o = (size_t)y * W + x;
    if (vec) {
      *(i32x4*)(P + o) = i32x4{gp[0], gp[1], gp[2], gp[3]};
      *(i32x4*)(A + o) = i32x4{ga[0], ga[1], ga[2], ga[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x + j < W) {
          P[o + j] = gp[j];
          A[o + j] = ga[j];
        }
    }
  }
}

// One thread per pixel on a tile's left column or top row, grid (cc_merge_grid, B): unions across the border with global
// atomicMin.  A pair that the pixel before it on the border already joins is skipped.  Items of an image: (ntx - 1) * H
// pixels on the left column of a tile (not the image's), then (nty - 1) * W on a top row.
template <class Key, bool K = false>
__device__ __forceinline__ void cc_merge_body(const uint8_t* labels, int32_t* parent, int H, int W, int ntx, int nty,
                                              int conn8, const int32_t* keys = nullptr) {
  const size_t img = (size_t)blockIdx.y * H * W;
  const uint8_t* L = labels + img;
  int32_t* P = parent + img;
  // pixel m equals pixel a, whose byte la is non-zero, in the byte and, with keys, in the key
  auto same = [&](int a, int m, uint8_t la) -> bool {
    if constexpr (K) return Key::byte(L[m]) == la && keys[img + m] == keys[img + a];
    else return Key::byte(L[m]) == la;
  };
  const long long nv = (long long)(ntx - 1) * H, total = nv + (long long)(nty - 1) * W;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    if (t < nv) {
      const int c = (int)(t / H), y = (int)(t - (long long)c * H), x = (c + 1) * kCcTW;
      const int a = y * W + x;
      const uint8_t la = Key::byte(L[a]);
      if (la == 0) continue;
      if (same(a, a - 1, la)) {
        // the pixel above joins the same two tile-local components
        const bool dup = (y % kCcTH) != 0 && same(a, a - W, la) && same(a, a - W - 1, la);
        if (!dup) g_union(P, a, a - 1);
      } else if (conn8) {
        if (y > 0 && same(a, a - W - 1, la)) g_union(P, a, a - W - 1);
        if (y + 1 < H && same(a, a + W - 1, la)) g_union(P, a, a + W - 1);
      }
    } else {
      const long long u = t - nv;
      const int r = (int)(u / W), x = (int)(u - (long long)r * W), y = (r + 1) * kCcTH;
      const int a = y * W + x, up = a - W;
      const uint8_t la = Key::byte(L[a]);
      if (la == 0) continue;
      if (same(a, up, la)) {
        const bool dup = (x % kCcTW) != 0 && same(a, a - 1, la) && same(a, up - 1, la);
        if (!dup) g_union(P, a, up);
      } else if (conn8) {
        if (x > 0 && same(a, up - 1, la)) g_union(P, a, up - 1);
        if (x + 1 < W && same(a, up + 1, la)) g_union(P, a, up + 1);
      }
    }
  }
}

// Every local root, grid (cc_flatten_grid, B): parent = find (now the set's first pixel), and ONE atomicAdd of its
// tile-local count onto area[root] -- one atomic per (tile, local set), never per pixel.
__device__ __forceinline__ void cc_flatten_body(int32_t* parent, int32_t* area, int HW) {
  const size_t img = (size_t)blockIdx.y * HW;
  int32_t* P = parent + img;
  int32_t* A = area + img;
  auto one = [&](int p, int a) {
    if (a <= 0) return;                  // not a local root
    const int r = g_find(P, p);
    if (r == p) return;
    P[p] = r;
    atomicAdd(&A[r], a);
  };
  if ((HW & 3) == 0 && ((uintptr_t)area & 15) == 0) {
    const int n4 = HW >> 2;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n4; e += gridDim.x * 256) {
      const i32x4 a = *(const i32x4*)(A + 4 * (size_t)e);
#pragma unroll
      for (int j = 0; j < 4; ++j) one(4 * e + j, a[j]);
    }
  } else {
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) one(p, A[p]);
  }
}

inline size_t cc_blocks(long long HW) { return (size_t)((HW + kCcTile - 1) / kCcTile); }

// One inline function per launch whose kernel loops: the grid, and with it the trips of the loop.
constexpr int kCcGridCap = 4096;
// the merge: one thread per item, grid-stride behind the cap.
inline long long cc_merge_items(int H, int W) {
  const int ntx = (W + kCcTW - 1) / kCcTW, nty = (H + kCcTH - 1) / kCcTH;
  return (long long)(ntx - 1) * H + (long long)(nty - 1) * W;
}
inline int cc_merge_grid(long long items) {
  return (int)((items + 255) / 256 > kCcGridCap ? kCcGridCap : (items + 255) / 256);
}
// the flatten: the grid is sized for four pixels a thread; the kernel takes that path when HW is a multiple of four and
// area is 16-byte aligned, else one pixel a thread over the same grid.  cc_flatten_vector repeats the kernel's own test
// for the query (the kernel decides on the device; the launcher never asks): keep the two in step.
inline int cc_flatten_grid(int HW) {
  const int per = (HW + 3) / 4;
  return (per + 255) / 256 > kCcGridCap ? kCcGridCap : (per + 255) / 256;
}
inline bool cc_flatten_vector(int HW, uintptr_t area) { return (HW & 3) == 0 && (area & 15) == 0; }

}  // namespace dfw
