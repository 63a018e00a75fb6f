// Candidate classes per query (pipeline.segment_candidates): every query is run against a handful of the library's
// classes, a different handful per query, and the masks are fused into ONE label map per query.  The quantised masks
// arrive ENTRY-major -- seg_u8 [E_cap][3][H][W], entry e one (query, candidate class) pair, a query's entries adjacent --
// with the per-entry maxima mx [E_cap] that a gt-less dfw_seg_postprocess_ex leaves.  Which entries belong to which query
// and which label byte each carries stands in a DEVICE table
//
//   tab = off[0 .. B] | lab[0 .. E_cap)        int32, query q owns entries [off[q], off[q + 1])
//
// that the kernel reads when it RUNS, as the routed attention reads its rows: a captured launch follows whatever the table
// holds at each replay, so one graph serves every choice of candidates of a shape.
//
// seg_cand_kernel is misc.hip's seg_labels_kernel with "entry of the query" where that one has "class": the same fp32
// score ((u0/255 + u1/255) + u2/255) / 3 through the same 256-entry table, foreground when score > the entry's threshold,
// label 0 with no foreground entry, else lab[e] of the foreground entry with the largest score -- entries in ascending
// order, only a strictly larger score takes over, so the earliest entry wins a tie.  No batch_max form.  The pred / gt /
// intersection histograms live in LDS, indexed by label byte (256 bins each), plus two per-entry histograms for `area`
// (foreground on its own, won the label); one 64-bit atomic per non-zero cell at the end.  4 pixels per thread through
// 32-bit words when HW % 4 == 0 and every pointer is word-aligned; a scalar path otherwise.
//
// The host validates the table's mirror before any launch.  What the kernel reads from the device table it clamps before
// use (0 <= lo <= hi <= E_cap, hi - lo <= 254, label & 255): a bad table written between replays gives wrong numbers,
// never a read outside seg_u8 / mx / tab or a bin outside the histograms.
#include "common.h"

namespace dfw {

constexpr int kCandMax = 254;   // entries of one query

// counts and area of dfw_seg_labels_cand: a library kernel, not a memset node (see seg_zero_kernel in misc.hip)
__global__ void seg_cand_zero_kernel(unsigned long long* counts, int nc, unsigned long long* area, int na) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (counts && e < nc) counts[e] = 0ull;
  if (area && e < na) area[e] = 0ull;
}

__global__ __launch_bounds__(256) void seg_cand_kernel(const uint8_t* u8, const uint32_t* mx, const int32_t* tab,
                                                       const uint8_t* gt, uint8_t* labels, unsigned long long* counts,
                                                       unsigned long long* area, int E_cap, int NLab, int HW, float r_thr,
                                                       float fixed_thr) {
  __shared__ float lut[256];
  __shared__ float thr[256];
  __shared__ uint32_t lbl[256];
  __shared__ unsigned hist[3 * 256];    // [inter | pred | gt][label byte]
  __shared__ unsigned ahist[2 * 256];   // [foreground | won][entry of this query]
  const int q = blockIdx.y, B = gridDim.y;
  // the query's range: two loads at a uniform address, clamped before anything is indexed with them
  int lo = tab[q], hi = tab[q + 1];
  lo = min(max(lo, 0), E_cap);
  hi = min(max(hi, lo), E_cap);
  hi = min(hi, lo + kCandMax);
  const int K = hi - lo;
  const int32_t* labt = tab + B + 1;
  lut[threadIdx.x] = (float)threadIdx.x / 255.0f;
  if ((int)threadIdx.x < K) {
    float t = fixed_thr;
    if (r_thr > 0.f) t = ((float)mx[lo + threadIdx.x] / 255.0f) * r_thr;
    thr[threadIdx.x] = t;
    lbl[threadIdx.x] = (uint32_t)labt[lo + threadIdx.x] & 255u;
  }
  for (int i = threadIdx.x; i < 3 * 256; i += 256) hist[i] = 0u;
  for (int i = threadIdx.x; i < 2 * 256; i += 256) ahist[i] = 0u;
  __syncthreads();
  const size_t ent = (size_t)3 * HW;                       // bytes between two entries
  const uint8_t* ub = u8 + (size_t)lo * ent;               // the query's first entry (not dereferenced when K == 0)
  const uint8_t* gb = gt ? gt + (size_t)q * HW : nullptr;
  uint8_t* lb = labels + (size_t)q * HW;
  const uint32_t NL = (uint32_t)NLab;
  auto count = [&](uint32_t l, uint32_t g) {
    if (g > NL) return;   // 255 = ignore; nlabels < g < 255 has no bin: dropped from every histogram too
    atomicAdd(&hist[256 + l], 1u);
    atomicAdd(&hist[512 + g], 1u);
    if (l == g) atomicAdd(&hist[l], 1u);
  };
  if ((HW & 3) == 0 && (((uintptr_t)u8 | (uintptr_t)gb | (uintptr_t)lb) & 3) == 0) {
    const int n4 = HW >> 2;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n4; e += gridDim.x * 256) {
      float best[4] = {-1.f, -1.f, -1.f, -1.f};
      uint32_t lab[4] = {0u, 0u, 0u, 0u};
      int win[4] = {-1, -1, -1, -1};
      const uint8_t* uc = ub + 4 * (size_t)e;
      for (int c = 0; c < K; ++c, uc += ent) {
        const uint32_t w0 = *(const uint32_t*)uc, w1 = *(const uint32_t*)(uc + HW), w2 = *(const uint32_t*)(uc + 2 * (size_t)HW);
        const float t = thr[c];
        const uint32_t l = lbl[c];
        unsigned nfg = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float sc = ((lut[(w0 >> (8 * k)) & 255u] + lut[(w1 >> (8 * k)) & 255u]) + lut[(w2 >> (8 * k)) & 255u]) / 3.0f;
          if (sc > t) {
            ++nfg;
            if (sc > best[k]) { best[k] = sc; lab[k] = l; win[k] = c; }
          }
        }
        if (area && nfg) atomicAdd(&ahist[c], nfg);
      }
      *(uint32_t*)(lb + 4 * (size_t)e) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
      if (area) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (win[k] >= 0) atomicAdd(&ahist[256 + win[k]], 1u);
      }
      if (gb) {
        const uint32_t wg = *(const uint32_t*)(gb + 4 * (size_t)e);
#pragma unroll
        for (int k = 0; k < 4; ++k) count(lab[k], (wg >> (8 * k)) & 255u);
      }
    }
  } else {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < HW; e += gridDim.x * 256) {
      float best = -1.f;
      uint32_t lab = 0u;
      int win = -1;
      const uint8_t* uc = ub + e;
      for (int c = 0; c < K; ++c, uc += ent) {
        const float sc = ((lut[uc[0]] + lut[uc[HW]]) + lut[uc[2 * (size_t)HW]]) / 3.0f;
        if (sc > thr[c]) {
          if (area) atomicAdd(&ahist[c], 1u);
          if (sc > best) { best = sc; lab = lbl[c]; win = c; }
        }
      }
      lb[e] = (uint8_t)lab;
      if (area && win >= 0) atomicAdd(&ahist[256 + win], 1u);
      if (gb) count(lab, gb[e]);
    }
  }
  if (!gb && !area) return;
  __syncthreads();
  if (gb) {
    const int NB = NLab + 1;
    unsigned long long* cb = counts + (size_t)q * 2 * NB;
    for (int l = threadIdx.x; l < NB; l += 256) {
      const unsigned in = hist[l], un = hist[256 + l] + hist[512 + l] - in;
      if (in) atomicAdd(cb + l, (unsigned long long)in);
      if (un) atomicAdd(cb + NB + l, (unsigned long long)un);
    }
  }
  if (area) {
    for (int c = threadIdx.x; c < K; c += 256) {
      const unsigned fg = ahist[c], won = ahist[256 + c];
      if (fg) atomicAdd(area + 2 * (size_t)(lo + c), (unsigned long long)fg);
      if (won) atomicAdd(area + 2 * (size_t)(lo + c) + 1, (unsigned long long)won);
    }
  }
}

}  // namespace dfw

using namespace dfw;

extern "C" int dfw_seg_labels_cand(const uint8_t* seg_u8, const uint32_t* mx, const int32_t* tab, const int32_t* tab_host,
                                   const uint8_t* gt, uint8_t* labels, int64_t* counts, int64_t* area, int32_t B,
                                   int32_t E_cap, int32_t nlabels, int32_t H, int32_t Wd, float r_threshold,
                                   float threshold, dfw_stream_t stream) {
  if (!seg_u8 || !tab || !tab_host || !labels) return DFW_EINVAL;
  if (B < 1 || H < 1 || Wd < 1 || E_cap < 1 || nlabels < 1 || nlabels > 254) return DFW_EINVAL;
  if (counts && !gt) return DFW_EINVAL;
  if (r_threshold > 0.f && !mx) return DFW_EINVAL;
  if (!(r_threshold > 0.f) && !(threshold > 0.f)) return DFW_EINVAL;
  // before the table is read: it is B + 1 + E_cap words
  if (B > 65535 || E_cap > (1 << 24) || (long long)H * Wd > (1ll << 30)) return DFW_ERANGE;
  // the table's host mirror: offsets from 0, non-decreasing, at most E_cap, at most 254 entries a query; labels 1..nlabels
  if (tab_host[0] != 0) return DFW_EINVAL;
  for (int q = 0; q < B; ++q) {
    const int32_t a = tab_host[q], b = tab_host[q + 1];
    if (b < a || b > E_cap || b - a > kCandMax) return DFW_EINVAL;
  }
  const int E = tab_host[B];
  for (int e = 0; e < E; ++e) {
    const int32_t l = tab_host[B + 1 + e];
    if (l < 1 || l > nlabels) return DFW_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * Wd;
  const bool want_counts = gt && counts;
  if (want_counts || area) {
    const int nc = want_counts ? B * 2 * (nlabels + 1) : 0, na = area ? 2 * E_cap : 0;
    const int n = nc > na ? nc : na;
    hipLaunchKernelGGL(seg_cand_zero_kernel, dim3((n + 255) / 256), dim3(256), 0, st,
                       (unsigned long long*)(want_counts ? counts : nullptr), nc, (unsigned long long*)area, na);
    DFW_CHECK_LAUNCH();
  }
  int cx = (HW / 4 + 255) / 256;
  if (cx > 64) cx = 64;
  if (cx < 1) cx = 1;
  hipLaunchKernelGGL(seg_cand_kernel, dim3(cx, B), dim3(256), 0, st, seg_u8, mx, tab, want_counts ? gt : nullptr, labels,
                     (unsigned long long*)counts, (unsigned long long*)area, E_cap, nlabels, HW, r_threshold, threshold);
  DFW_CHECK_LAUNCH();
  return 0;
}
