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
// seg_cand_kernel is seg_fuse (seg_fuse.h) over the entries of a query: its prologue takes the query's range from the
// table, each entry's threshold from mx[e] (no batch_max form) and its label byte from the table, and it keeps the
// per-entry `area` histograms.
//
// The host validates the table's mirror before any launch.  What the kernel reads from the device table it clamps before
// use (0 <= lo <= hi <= E_cap, hi - lo <= 254, label & 255): a bad table written between replays gives wrong numbers,
// never a read outside seg_u8 / mx / tab or a bin outside the histograms.
#include "common.h"
#include "seg_fuse.h"

namespace dfw {

__global__ __launch_bounds__(256) void seg_cand_kernel(const uint8_t* u8, const uint32_t* mx, const int32_t* tab,
                                                       const uint8_t* gt, uint8_t* labels, unsigned long long* counts,
                                                       unsigned long long* area, int E_cap, int NLab, int HW, float r_thr,
                                                       float fixed_thr) {
  __shared__ seg_fuse_lds<true> s;
  const int q = blockIdx.y, B = gridDim.y;
  // the query's range: two loads at a uniform address, clamped before anything is indexed with them
  int lo = tab[q], hi = tab[q + 1];
  lo = min(max(lo, 0), E_cap);
  hi = min(max(hi, lo), E_cap);
  hi = min(hi, lo + kSegCandMax);
  const int K = hi - lo;
  const int32_t* labt = tab + B + 1;
  if ((int)threadIdx.x < K) {
    s.thr[threadIdx.x] = seg_threshold(mx + lo + threadIdx.x, 0, 1, r_thr, fixed_thr, 0);
    s.lbl[threadIdx.x] = (uint32_t)labt[lo + threadIdx.x] & 255u;
  }
  const size_t ent = (size_t)3 * HW;                       // bytes between two entries
  const seg_planes pl = {u8 + (size_t)lo * ent, ent, K, HW};
  seg_fuse<true>(s, pl, labels + (size_t)q * HW, gt ? gt + (size_t)q * HW : nullptr, false, area != nullptr,
                 seg_gt_byte{NLab});
  if (gt) seg_flush_counts(s.hist, counts + (size_t)q * 2 * (NLab + 1), NLab + 1);
  if (area) seg_flush_area(s.ahist, area + 2 * (size_t)lo, K);
}

int cand_table_check(const int32_t* tab_host, int B, int E_cap, int nlabels, int* K, int* E) {
  if (tab_host[0] != 0) return DFW_EINVAL;
  *K = 0;
  for (int q = 0; q < B; ++q) {
    const int32_t lo = tab_host[q], hi = tab_host[q + 1];
    if (hi < lo || hi > E_cap || hi - lo > kSegCandMax) return DFW_EINVAL;
    *K = hi - lo > *K ? hi - lo : *K;
  }
  *E = tab_host[B];
  for (int e = 0; e < *E; ++e) {
    const int32_t l = tab_host[B + 1 + e];
    if (l < 1 || l > nlabels) return DFW_EINVAL;
  }
  return 0;
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
  int K, E;
  if (int e = cand_table_check(tab_host, B, E_cap, nlabels, &K, &E)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * Wd;
  const bool want_counts = gt && counts;
  if (int e = seg_zero_launch(st, nullptr, 0, want_counts ? counts : nullptr, B * 2 * (nlabels + 1), area, 2 * E_cap)) return e;
  int cx = (HW / 4 + 255) / 256;
  if (cx > 64) cx = 64;
  if (cx < 1) cx = 1;
  hipLaunchKernelGGL(seg_cand_kernel, dim3(cx, B), dim3(256), 0, st, seg_u8, mx, tab, want_counts ? gt : nullptr, labels,
                     (unsigned long long*)counts, (unsigned long long*)area, E_cap, nlabels, HW, r_threshold, threshold);
  DFW_CHECK_LAUNCH();
  return 0;
}
