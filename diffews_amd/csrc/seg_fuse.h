// The one label-fusion body of the segmentation output side, and the threshold / count tails its callers share.
//
// seg_fuse: K planes-of-3 of quantised masks (plane c at p0 + c * stride, channels HW bytes apart) -> one label byte per
// pixel.  Per pixel and plane the score is the fp32 mean ((u0/255 + u1/255) + u2/255) / 3 through a 256-entry table, the
// plane is foreground when score > thr[c], and the label is 0 with no foreground plane, else lbl[c] of the foreground plane
// with the largest score: planes are visited in ascending order and only a strictly larger score takes over, so the
// earliest plane wins a tie.  With ground truth, a functor maps every id to a histogram bin or to "dropped" (negative), and
// the workgroup keeps pred / gt / intersection histograms in LDS, indexed by label byte; with AREA also two per-plane
// histograms (foreground on its own, won the label).  4 pixels per thread through 32-bit words when HW % 4 == 0, stride % 4
// == 0 and the three pointers are word-aligned; a scalar path otherwise.  The flushes issue one 64-bit atomic per non-zero
// cell.
//
// The callers are thin __global__ kernels (seg_labels_kernel, seg_cand_kernel, native_labels_kernel,
// native_labels_cand_kernel): each declares the LDS, fills thr / lbl (and clamps what it reads from a device table) in its
// prologue, calls seg_fuse and flushes.
#pragma once
#include "common.h"

namespace dfw {

constexpr int kSegCandMax = 254;   // planes of one image or query: a label byte, 0 = background, 255 = ignore

// The histograms come first: with the byte table at offset 0 and the histograms behind it, seg_cand_kernel measured 10 %
// slower on the same instruction stream (profiles/seg_fuse_timing.md).
template <bool AREA> struct seg_fuse_lds {
  unsigned hist[3 * 256];              // [inter | pred | gt][label byte]
  float lut[256];
  float thr[256];                      // per plane, set by the caller
  uint32_t lbl[256];                   // per plane, set by the caller
  unsigned ahist[AREA ? 2 * 256 : 1];  // [foreground | won][plane]
};

struct seg_planes {
  const uint8_t* p0;   // plane 0 of this image / query (not dereferenced when K == 0)
  size_t stride;       // bytes between two planes
  int K, HW;
};

// r_thr > 0: dynamic threshold max * r_threshold (main_oss.py:129-132) with the maximum mc[b] of this image or (batch_max)
// of mc[0 .. B), the whole batch tensor, as `pred_mask.max()` literally does; else the fixed `--threshold`
// (main_oss.py:134-135).
__device__ __forceinline__ float seg_threshold(const uint32_t* mc, int b, int B, float r_thr, float fixed_thr,
                                               int batch_max) {
  if (!(r_thr > 0.f)) return fixed_thr;
  uint32_t m = mc[b];
  if (batch_max)
    for (int i = 0; i < B; ++i) m = max(m, mc[i]);
  return ((float)m / 255.0f) * r_thr;
}

// ---- ground truth id -> histogram bin, negative = dropped from every histogram ----
// bytes: the id is the label, 255 = ignore, n < id < 255 has no bin
struct seg_gt_byte {
  int n;
  __device__ __forceinline__ int operator()(int id) const { return id > n ? -1 : id; }
};
// native size, no id table: the item's ignore_value dropped, the id is the label, ids outside 0..n have no bin
struct seg_gt_plain {
  int ign, n;
  __device__ __forceinline__ int operator()(int id) const { return (ign >= 0 && id == ign) || id < 0 || id > n ? -1 : id; }
};
// native size, class_ids [n]: 1 + the lowest c with ids[c] == id, every other id is background.  Ids 0..255 go through
// idmap, an LDS table that fill() builds once per workgroup (a barrier before the first use).
struct seg_gt_classes {
  int ign, n;
  const int32_t* ids;
  int* idmap;
  __device__ __forceinline__ int find(int id) const {
    int g = 0;
    for (int c = n - 1; c >= 0; --c)
      if (ids[c] == id) g = c + 1;   // descending: the lowest c stays
    return g;
  }
  __device__ __forceinline__ void fill() const { idmap[threadIdx.x] = find((int)threadIdx.x); }
  __device__ __forceinline__ int operator()(int id) const {
    if (ign >= 0 && id == ign) return -1;
    return (unsigned)id < 256u ? idmap[id] : find(id);
  }
};
// native size, entry_ids of the query's n entries: lbl[k] of the earliest entry with ids[k] == id, else background.
// fill() reads lbl: a barrier between the caller's writes of lbl and fill().
struct seg_gt_entries {
  int ign, n;
  const int32_t* ids;
  const uint32_t* lbl;
  int* idmap;
  __device__ __forceinline__ int find(int id) const {
    int g = 0;
    for (int k = n - 1; k >= 0; --k)
      if (ids[k] == id) g = (int)lbl[k];   // descending: the earliest entry stays
    return g;
  }
  __device__ __forceinline__ void fill() const { idmap[threadIdx.x] = find((int)threadIdx.x); }
  __device__ __forceinline__ int operator()(int id) const {
    if (ign >= 0 && id == ign) return -1;
    return (unsigned)id < 256u ? idmap[id] : find(id);
  }
};

// Workgroup of 256, grid x strides over the pixels.  s.thr / s.lbl [0, K) are the caller's (written before the call, no
// barrier needed in between); labels lb [HW]; ground truth gt [HW] of uint8 or (wide) int32, null: no histograms; `area`
// (only with AREA): keep the per-plane histograms.  Ends with a barrier: the histograms are complete on return.
template <bool AREA, class GtMap>
__device__ __forceinline__ void seg_fuse(seg_fuse_lds<AREA>& s, const seg_planes pl, uint8_t* lb, const uint8_t* gt,
                                         bool wide, bool area, const GtMap map) {
  s.lut[threadIdx.x] = (float)threadIdx.x / 255.0f;
  for (int i = threadIdx.x; i < 3 * 256; i += 256) s.hist[i] = 0u;
  if (AREA)
    for (int i = threadIdx.x; i < 2 * 256; i += 256) s.ahist[i] = 0u;
  __syncthreads();
  const int HW = pl.HW, K = pl.K;
  const size_t stride = pl.stride;
  const int32_t* g32 = (const int32_t*)gt;
  const bool keep = AREA && area;
  auto score = [&](uint32_t u0, uint32_t u1, uint32_t u2) { return ((s.lut[u0] + s.lut[u1]) + s.lut[u2]) / 3.0f; };
  auto count = [&](uint32_t l, int id) {
    const int g = map(id);
    if (g < 0) return;
    atomicAdd(&s.hist[256 + l], 1u);
    atomicAdd(&s.hist[512 + g], 1u);
    if ((int)l == g) atomicAdd(&s.hist[l], 1u);
  };
  if ((HW & 3) == 0 && (stride & 3) == 0 && (((uintptr_t)pl.p0 | (uintptr_t)lb | (uintptr_t)gt) & 3) == 0) {
    const int n4 = HW >> 2;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n4; e += gridDim.x * 256) {
      const size_t o = 4 * (size_t)e;
      float best[4] = {-1.f, -1.f, -1.f, -1.f};
      uint32_t lab[4] = {0u, 0u, 0u, 0u};
      int win[4] = {-1, -1, -1, -1};
      const uint8_t* uc = pl.p0 + o;
      for (int c = 0; c < K; ++c, uc += stride) {
        const uint32_t w0 = *(const uint32_t*)uc, w1 = *(const uint32_t*)(uc + HW), w2 = *(const uint32_t*)(uc + 2 * (size_t)HW);
        const float t = s.thr[c];
        const uint32_t l = s.lbl[c];
        unsigned nfg = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float sc = score((w0 >> (8 * k)) & 255u, (w1 >> (8 * k)) & 255u, (w2 >> (8 * k)) & 255u);
          if (sc > t) {
            ++nfg;
            if (sc > best[k]) { best[k] = sc; lab[k] = l; win[k] = c; }
          }
        }
        if (keep && nfg) atomicAdd(&s.ahist[c], nfg);
      }
      *(uint32_t*)(lb + o) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
      if (keep) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (win[k] >= 0) atomicAdd(&s.ahist[256 + win[k]], 1u);
      }
      if (gt) {
        if (wide) {
#pragma unroll
          for (int k = 0; k < 4; ++k) count(lab[k], g32[o + k]);
        } else {
          const uint32_t wg = *(const uint32_t*)(gt + o);
#pragma unroll
          for (int k = 0; k < 4; ++k) count(lab[k], (int)((wg >> (8 * k)) & 255u));
        }
      }
    }
  } else {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < HW; e += gridDim.x * 256) {
      float best = -1.f;
      uint32_t lab = 0u;
      int win = -1;
      const uint8_t* uc = pl.p0 + e;
      for (int c = 0; c < K; ++c, uc += stride) {
        const float sc = score(uc[0], uc[HW], uc[2 * (size_t)HW]);
        if (sc > s.thr[c]) {
          if (keep) atomicAdd(&s.ahist[c], 1u);
          if (sc > best) { best = sc; lab = s.lbl[c]; win = c; }
        }
      }
      lb[e] = (uint8_t)lab;
      if (keep && win >= 0) atomicAdd(&s.ahist[256 + win], 1u);
      if (gt) count(lab, wide ? g32[e] : (int)gt[e]);
    }
  }
  __syncthreads();
}

// hist -> cb [2][NB] = intersections, unions (pred + gt - inter)
__device__ __forceinline__ void seg_flush_counts(const unsigned* hist, unsigned long long* cb, int NB) {
  for (int l = threadIdx.x; l < NB; l += 256) {
    const unsigned in = hist[l], un = hist[256 + l] + hist[512 + l] - in;
    if (in) atomicAdd(cb + l, (unsigned long long)in);
    if (un) atomicAdd(cb + NB + l, (unsigned long long)un);
  }
}

// ahist -> area [K][2] of the query's entries = foreground, won
__device__ __forceinline__ void seg_flush_area(const unsigned* ahist, unsigned long long* area, int K) {
  for (int c = threadIdx.x; c < K; c += 256) {
    const unsigned fg = ahist[c], won = ahist[256 + c];
    if (fg) atomicAdd(area + 2 * (size_t)c, (unsigned long long)fg);
    if (won) atomicAdd(area + 2 * (size_t)c + 1, (unsigned long long)won);
  }
}

// The tail of the two binary count kernels.  c = {inter0, inter1, pred0, pred1, gt0, gt1} of this thread; wave reduce,
// then one set of integer atomics per workgroup of 256: cb = {inter0, inter1, union0, union1}, union = pred + gt - inter.
__device__ __forceinline__ void seg_count_reduce(unsigned (&c)[6], long long* cb) {
  __shared__ unsigned wc[4][6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    unsigned v = c[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    c[k] = v;
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) wc[threadIdx.x >> 6][k] = c[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) t[k] = wc[0][k] + wc[1][k] + wc[2][k] + wc[3][k];
    atomicAdd((unsigned long long*)(cb + 0), (unsigned long long)t[0]);
    atomicAdd((unsigned long long*)(cb + 1), (unsigned long long)t[1]);
    atomicAdd((unsigned long long*)(cb + 2), (unsigned long long)(t[2] + t[4] - t[0]));
    atomicAdd((unsigned long long*)(cb + 3), (unsigned long long)(t[3] + t[5] - t[1]));
  }
}

}  // namespace dfw
