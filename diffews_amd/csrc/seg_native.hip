// Native-size masks and scores (the launcher's --use_original_imgsize, main_oss.py:128-155): the output-side counterpart
// of inputs.hip.  The reference resizes the uint8 prediction back to the query's own size with
// `Image.fromarray(hwc).resize((W, H))` (marigold_pipeline_rgb_latent_noise.py:539 -- Pillow's default filter, BICUBIC)
// and then thresholds and scores it on the host.  Here that is four launches for a whole RAGGED batch, however many
// images it holds: zero, horizontal pass, vertical pass + per-image maximum, threshold + count.  Grid z runs over the
// images, x / y are sized for the largest one and blocks beyond an image's extent exit; everything per image (size,
// where its weights, scratch, outputs and ground truth lie) comes from one device-resident table, dfw_native_item[B].
//
// Arithmetic: resample_h_kernel's (Pillow's ImagingResample, 8 bits per channel): 2^21 + sum tap * weight, arithmetic
// shift by 22, clamp to 0..255, uint8 intermediate between the passes; planar, since a 3-channel resize is three
// single-channel ones.  Bicubic overshoots (a 0/200 block image reaches 225), so the dynamic threshold uses the maximum
// of the RESIZED image, taken in the vertical pass.  Threshold and count tail are seg_count_kernel's (seg_fuse.h).
//
// dfw_seg_labels_native is the same for N classes (seg_u8 [N][B][3][Hs][Ws], pipeline.segment_classes): the two resize
// kernels run over N * B planes-of-3 (grid z = c * B + i, one item per image, a byte stride per class), the fourth launch
// is seg_fuse (seg_fuse.h) on the resized bytes.
//
// dfw_seg_labels_cand_native is the same for the ENTRIES of seg_candidates.hip (seg_u8 [E_cap][3][Hs][Ws], one entry per
// (query, candidate class) pair): the two resize kernels run over E planes-of-3 (grid z = e; the entry's query is looked up
// in the device table, its position k in the query's list takes the part of the class above, so the scratch is K strides
// with K the longest list), the fourth launch is seg_fuse over the query's entries, with area.
//
// What the label kernels add to seg_fuse here: planes, labels and ground truth are placed by the image's item, not by
// H * W, and the ground truth is read in place at native size -- uint8 or int32 per image, the item's ignore_value
// dropped, ids mapped through class_ids / entry_ids where given (native_fuse).  All three entry points check the items'
// host mirror with one validator (native_items_check) before any launch.
//
// Byte work bound by HBM / L2: a thread produces 4 adjacent bytes of one channel row, one 32-bit store where the
// address is 4-byte aligned (row starts are when w % 4 == 0: every offset of the table is 16-byte aligned), byte stores
// otherwise.
#include "common.h"
#include "resample_host.h"
#include "seg_fuse.h"

namespace dfw {

constexpr int kNativeBits = kResamplePrecisionBits;

__device__ __forceinline__ uint32_t native_clip8(int acc) { return (uint32_t)min(max(acc >> kNativeBits, 0), 255); }

__device__ __forceinline__ void native_store4(uint8_t* dst, uint32_t word, int nx) {
  if (nx == 4 && ((uintptr_t)dst & 3) == 0) {
    *(uint32_t*)dst = word;
  } else {
    for (int j = 0; j < nx; ++j) dst[j] = (uint8_t)(word >> (8 * j));
  }
}

// horizontal: seg_u8 [B][3][Hs][Ws] -> tmp[i] = [3][Hs][w_i].  Block (64, 4): x -> 4 adjacent output columns,
// y -> row of the flat 3 * Hs rows of the image's planes.  With classes (dfw_seg_labels_native) seg_u8 is [N][B][3][Hs][Ws]
// and grid z = c * B + i: class c of image i uses item i, its intermediates lie tmp_cls bytes after class c - 1's.  The
// binary path launches B planes with tmp_cls = 0.
//
// One copy of the arithmetic for both forms: `cls` is the plane's position among its item's planes (class c, or position k
// in a query's candidate list), `item` the index of its item; both are workgroup-uniform.
__device__ __forceinline__ void native_h_body(const uint8_t* __restrict__ seg_u8,
                                              const dfw_native_item* __restrict__ items, uint32_t item, int cls,
                                              const uint8_t* __restrict__ weights, uint8_t* __restrict__ tmp, int Hs,
                                              int Ws, size_t tmp_cls) {
  const dfw_native_item it = items[item];
  const int w = it.w;
  const int x4 = (blockIdx.x * 64 + threadIdx.x) * 4;
  const int row = blockIdx.y * 4 + threadIdx.y;
  if (x4 >= w || row >= 3 * Hs) return;
  const int32_t* bounds = (const int32_t*)(weights + it.xb_off);
  const int32_t* coef = (const int32_t*)(weights + it.xc_off);
  const uint8_t* src = seg_u8 + ((size_t)blockIdx.z * 3 * Hs + row) * Ws;
  const int nx = min(4, w - x4);
  uint32_t word = 0;
  for (int j = 0; j < nx; ++j) {
    const int xo = x4 + j;
    const int x0 = bounds[2 * xo], n = bounds[2 * xo + 1];
    const int32_t* k = coef + (size_t)xo * it.xk;
    int acc = 1 << (kNativeBits - 1);
    for (int x = 0; x < n; ++x) acc += (int)src[x0 + x] * k[x];
    word |= native_clip8(acc) << (8 * j);
  }
  native_store4(tmp + cls * tmp_cls + it.tmp_off + (size_t)row * w + x4, word, nx);
}

__global__ __launch_bounds__(256) void native_h_kernel(const uint8_t* __restrict__ seg_u8,
                                                       const dfw_native_item* __restrict__ items,
                                                       const uint8_t* __restrict__ weights, uint8_t* __restrict__ tmp,
                                                       int Hs, int Ws, int B, size_t tmp_cls) {
  const int cls = blockIdx.z / B;
  native_h_body(seg_u8, items, blockIdx.z - cls * B, cls, weights, tmp, Hs, Ws, tmp_cls);
}

// The candidate form (dfw_seg_labels_cand_native): seg_u8 is ENTRY-major [E_cap][3][Hs][Ws] and grid z = e, one plane-of-3
// per entry.  Which query q owns entry e is searched in the device table's offsets -- the largest q in [0, B) with
// off[q] <= e, a bisection at workgroup-uniform addresses that ends whatever the table holds -- and k = e - off[q] is the
// entry's position in q's list, clamped to [0, Kcap) (the longest list of the host mirror, what the workspace was
// validated for): a table rewritten after the call was made gives wrong numbers, never a byte outside the workspace.
__device__ __forceinline__ void native_cand_plane(const int32_t* __restrict__ tab, int B, int Kcap, int e, int& q, int& k) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid] <= e) lo = mid; else hi = mid - 1;
  }
  q = lo;
  k = min(max(e - tab[lo], 0), Kcap - 1);
}

__global__ __launch_bounds__(256) void native_h_cand_kernel(const uint8_t* __restrict__ seg_u8,
                                                            const dfw_native_item* __restrict__ items,
                                                            const int32_t* __restrict__ tab,
                                                            const uint8_t* __restrict__ weights,
                                                            uint8_t* __restrict__ tmp, int Hs, int Ws, int B, int Kcap,
                                                            size_t tmp_cls) {
  int q, k;
  native_cand_plane(tab, B, Kcap, (int)blockIdx.z, q, k);
  native_h_body(seg_u8, items, q, k, weights, tmp, Hs, Ws, tmp_cls);
}

// vertical + maximum: tmp[i] -> res + u8_off = [3][h_i][w_i] (res may be null: maximum only).  Block (64, 4) over
// (4 adjacent columns, row of the flat 3 * h_i output rows).  One atomicMax per workgroup, as seg_u8_kernel does.
// Grid z = c * B + i as in native_h_kernel: mx is [N][B], class c's resized bytes lie res_cls bytes after class c - 1's.
__device__ __forceinline__ void native_v_body(const dfw_native_item* __restrict__ items, uint32_t item, int cls,
                                              const uint8_t* __restrict__ weights, const uint8_t* __restrict__ tmp,
                                              uint8_t* __restrict__ res, uint32_t* mx, int Hs, size_t tmp_cls,
                                              size_t res_cls, uint32_t* wmax) {
  const dfw_native_item it = items[item];
  const int w = it.w, h = it.h;
  if ((int)blockIdx.x * 256 >= w || (int)blockIdx.y * 4 >= 3 * h) return;   // whole block beyond this image
  const int x4 = (blockIdx.x * 64 + threadIdx.x) * 4;
  const int row = blockIdx.y * 4 + threadIdx.y;
  uint32_t m = 0;
  if (x4 < w && row < 3 * h) {
    const int c = row / h, yo = row - c * h;
    const int32_t* bounds = (const int32_t*)(weights + it.yb_off);
    const int32_t* k = (const int32_t*)(weights + it.yc_off) + (size_t)yo * it.yk;
    const int y0 = bounds[2 * yo], n = bounds[2 * yo + 1];
    const uint8_t* col = tmp + cls * tmp_cls + it.tmp_off + ((size_t)c * Hs + y0) * w + x4;
    const int nx = min(4, w - x4);
    int acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = 1 << (kNativeBits - 1);
    if (nx == 4 && (w & 3) == 0 && ((uintptr_t)col & 3) == 0) {
      for (int y = 0; y < n; ++y) {
        const uint32_t v = *(const uint32_t*)(col + (size_t)y * w);
        const int kv = k[y];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += (int)((v >> (8 * j)) & 255u) * kv;
      }
    } else {
      for (int y = 0; y < n; ++y) {
        const uint8_t* px = col + (size_t)y * w;
        const int kv = k[y];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < nx) acc[j] += (int)px[j] * kv;
      }
    }
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nx) {
        const uint32_t q = native_clip8(acc[j]);
        word |= q << (8 * j);
        m = max(m, q);
      }
    if (res) native_store4(res + cls * res_cls + it.u8_off + (size_t)row * w + x4, word, nx);
  }
  if (!mx) return;   // kernel argument: uniform
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  const int tid = threadIdx.y * 64 + threadIdx.x;   // wmax: the kernel's own 4 words of LDS
  if ((tid & 63) == 0) wmax[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) atomicMax(mx + blockIdx.z, max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3])));
}

__global__ __launch_bounds__(256) void native_v_kernel(const dfw_native_item* __restrict__ items,
                                                       const uint8_t* __restrict__ weights,
                                                       const uint8_t* __restrict__ tmp, uint8_t* __restrict__ res,
                                                       uint32_t* mx, int Hs, int B, size_t tmp_cls, size_t res_cls) {
  __shared__ uint32_t wmax[4];
  const int cls = blockIdx.z / B;
  native_v_body(items, blockIdx.z - cls * B, cls, weights, tmp, res, mx, Hs, tmp_cls, res_cls, wmax);
}

// The candidate form: grid z = e as in native_h_cand_kernel, mx is [E_cap].
__global__ __launch_bounds__(256) void native_v_cand_kernel(const dfw_native_item* __restrict__ items,
                                                            const int32_t* __restrict__ tab,
                                                            const uint8_t* __restrict__ weights,
                                                            const uint8_t* __restrict__ tmp, uint8_t* __restrict__ res,
                                                            uint32_t* mx, int Hs, int B, int Kcap, size_t tmp_cls,
                                                            size_t res_cls) {
  __shared__ uint32_t wmax[4];
  int q, k;
  native_cand_plane(tab, B, Kcap, (int)blockIdx.z, q, k);
  native_v_body(items, q, k, weights, tmp, res, mx, Hs, tmp_cls, res_cls, wmax);
}

// threshold + counts per image over h_i * w_i: seg_count_kernel's expressions and reduction, the ground truth read in
// place at native size (uint8 or int32 class ids, per image).
__global__ __launch_bounds__(256) void native_count_kernel(const dfw_native_item* __restrict__ items,
                                                           const uint8_t* __restrict__ res, const uint8_t* gt,
                                                           const uint32_t* mx, uint8_t* pred, long long* counts,
                                                           float r_thr, float fixed_thr, int batch_max) {
  __shared__ float lut[256];
  lut[threadIdx.x] = (float)threadIdx.x / 255.0f;
  __syncthreads();
  const int b = blockIdx.y;
  const dfw_native_item it = items[b];
  const int HW = it.h * it.w;
  const float thr = seg_threshold(mx, b, gridDim.y, r_thr, fixed_thr, batch_max);
  // kept pixels, pred1, gt1, inter0, inter1 (scalars: a histogram indexed by pr would be spilled to LDS per thread);
  // pred0 = kept - pred1, gt0 = kept - gt1
  unsigned n_kept = 0, n_p1 = 0, n_g1 = 0, n_i0 = 0, n_i1 = 0;
  const uint8_t* ub = res + it.u8_off;
  uint8_t* pb = pred ? pred + it.pred_off : nullptr;
  const uint8_t* g8 = counts ? gt + it.gt_off : nullptr;
  const int32_t* g32 = (const int32_t*)g8;
  const bool wide = it.gt_elem == 4;
  const int cls = it.class_value, ign = it.ignore_value;
  auto predict = [&](uint32_t u0, uint32_t u1, uint32_t u2) {
    const float mean = ((lut[u0] + lut[u1]) + lut[u2]) / 3.0f;
    return mean > thr ? 1 : 0;
  };
  auto tally = [&](int pr, int id) {
    if (ign >= 0 && id == ign) return;  // ignore value: dropped from every histogram
    const int g = id == cls ? 1 : 0;
    n_kept++;
    n_p1 += pr;
    n_g1 += g;
    n_i1 += pr & g;
    n_i0 += (pr | g) ^ 1;
  };
  if ((HW & 3) == 0 && (((uintptr_t)ub | (uintptr_t)pb | (uintptr_t)g8) & 3) == 0) {
    const int n4 = HW >> 2;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n4; e += gridDim.x * 256) {
      const size_t o = 4 * (size_t)e;
      const uint32_t w0 = *(const uint32_t*)(ub + o), w1 = *(const uint32_t*)(ub + HW + o);
      const uint32_t w2 = *(const uint32_t*)(ub + 2 * (size_t)HW + o);
      uint32_t pw = 0;
      int pr[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        pr[k] = predict((w0 >> (8 * k)) & 255u, (w1 >> (8 * k)) & 255u, (w2 >> (8 * k)) & 255u);
        pw |= (uint32_t)pr[k] << (8 * k);
      }
      if (pb) *(uint32_t*)(pb + o) = pw;
      if (g8) {
        if (wide) {
#pragma unroll
          for (int k = 0; k < 4; ++k) tally(pr[k], g32[o + k]);
        } else {
          const uint32_t wg = *(const uint32_t*)(g8 + o);
#pragma unroll
          for (int k = 0; k < 4; ++k) tally(pr[k], (int)((wg >> (8 * k)) & 255u));
        }
      }
    }
  } else {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < HW; e += gridDim.x * 256) {
      const int pr = predict(ub[e], ub[HW + e], ub[2 * (size_t)HW + e]);
      if (pb) pb[e] = (uint8_t)pr;
      if (g8) tally(pr, wide ? g32[e] : (int)g8[e]);
    }
  }
  if (!counts) return;   // kernel argument: uniform
  // inter0, inter1, pred0, pred1, gt0, gt1
  unsigned c[6] = {n_i0, n_i1, n_kept - n_p1, n_p1, n_kept - n_g1, n_g1};
  seg_count_reduce(c, counts + 4 * b);
}

// What both label kernels take from the image's item: where its labels and ground truth lie (gt null: no counts), and
// seg_fuse with the ground-truth rule that the id tables select -- class_ids, else entry_ids, else the plain ids 0..NLab.
// The functors' id maps are built here, behind a barrier: entry_ids reads s.lbl, which the caller has just written.
template <bool AREA>
__device__ __forceinline__ void native_fuse(seg_fuse_lds<AREA>& s, const dfw_native_item& it, const seg_planes pl,
                                            uint8_t* labels, const uint8_t* gt, bool area, int NLab,
                                            const int32_t* class_ids, const int32_t* entry_ids) {
  __shared__ int idmap[256];   // ground-truth id 0..255 -> label
  uint8_t* lb = labels + it.pred_off;
  const uint8_t* g8 = gt ? gt + it.gt_off : nullptr;
  const bool wide = it.gt_elem == 4;
  const int ign = it.ignore_value;
  if (class_ids) {
    const seg_gt_classes map = {ign, NLab, class_ids, idmap};
    map.fill();
    seg_fuse<AREA>(s, pl, lb, g8, wide, area, map);
  } else if (entry_ids) {
    const seg_gt_entries map = {ign, pl.K, entry_ids, s.lbl, idmap};
    __syncthreads();
    map.fill();
    seg_fuse<AREA>(s, pl, lb, g8, wide, area, map);
  } else {
    seg_fuse<AREA>(s, pl, lb, g8, wide, area, seg_gt_plain{ign, NLab});
  }
}

// label + counts per image over h_i * w_i, N classes: seg_fuse on the RESIZED bytes -- class c of image b at
// res + c * res_cls + u8_off, label c + 1 -- with the thresholds from mx [N][B], the maxima of the resized planes, and the
// ground truth read in place at native size (uint8 or int32 per image): counts [B][2][N+1].
__global__ __launch_bounds__(256) void native_labels_kernel(const dfw_native_item* __restrict__ items,
                                                            const uint8_t* __restrict__ res, size_t res_cls,
                                                            const uint8_t* gt, const uint32_t* mx,
                                                            const int32_t* class_ids, uint8_t* labels,
                                                            unsigned long long* counts, int N, float r_thr,
                                                            float fixed_thr, int batch_max) {
  __shared__ seg_fuse_lds<false> s;
  const int b = blockIdx.y, B = gridDim.y;
  const dfw_native_item it = items[b];
  if ((int)threadIdx.x < N) {
    s.thr[threadIdx.x] = seg_threshold(mx + (size_t)threadIdx.x * B, b, B, r_thr, fixed_thr, batch_max);
    s.lbl[threadIdx.x] = threadIdx.x + 1;
  }
  const seg_planes pl = {res + it.u8_off, res_cls, N, it.h * it.w};
  native_fuse<false>(s, it, pl, labels, counts ? gt : nullptr, false, N, class_ids, nullptr);
  if (counts) seg_flush_counts(s.hist, counts + (size_t)b * 2 * (N + 1), N + 1);
}

// label + counts + area per query over h_q * w_q (dfw_seg_labels_cand_native): seg_cand_kernel's prologue at native size.
// Entry e = lo + k of query q lies at res + k * res_cls + u8_off (the resized bytes), its threshold comes from mx[e], the
// maximum of ITS resized planes, and its label byte from the table.  The range is clamped as seg_cand_kernel clamps it and
// to Kcap, the longest list the workspace was validated for.  entry_ids [E_cap] names the ground-truth id of each entry.
__global__ __launch_bounds__(256) void native_labels_cand_kernel(const dfw_native_item* __restrict__ items,
                                                                 const uint8_t* __restrict__ res, size_t res_cls,
                                                                 const uint8_t* gt, const uint32_t* mx,
                                                                 const int32_t* tab, const int32_t* class_ids,
                                                                 const int32_t* entry_ids, uint8_t* labels,
                                                                 unsigned long long* counts, unsigned long long* area,
                                                                 int E_cap, int Kcap, int NLab, float r_thr,
                                                                 float fixed_thr) {
  __shared__ seg_fuse_lds<true> s;
  const int q = blockIdx.y, B = gridDim.y;
  const dfw_native_item it = items[q];
  // the query's range: two loads at a uniform address, clamped before anything is indexed with them
  int lo = tab[q], hi = tab[q + 1];
  lo = min(max(lo, 0), E_cap);
  hi = min(max(hi, lo), E_cap);
  hi = min(hi, lo + min(Kcap, kSegCandMax));
  const int K = hi - lo;
  const int32_t* labt = tab + B + 1;
  if ((int)threadIdx.x < K) {
    s.thr[threadIdx.x] = seg_threshold(mx + lo + threadIdx.x, 0, 1, r_thr, fixed_thr, 0);
    s.lbl[threadIdx.x] = (uint32_t)labt[lo + threadIdx.x] & 255u;
  }
  const seg_planes pl = {res + it.u8_off, res_cls, K, it.h * it.w};
  native_fuse<true>(s, it, pl, labels, counts ? gt : nullptr, area != nullptr, NLab, class_ids,
                    entry_ids ? entry_ids + lo : nullptr);
  if (counts) seg_flush_counts(s.hist, counts + (size_t)q * 2 * (NLab + 1), NLab + 1);
  if (area) seg_flush_area(s.ahist, area + 2 * (size_t)lo, K);
}

}  // namespace dfw

using namespace dfw;

extern "C" int32_t dfw_resample_ksize_ex(int32_t in_size, int32_t out_size, int32_t filter) {
  resample_filter_fn fn;
  double support;
  if (!resample_filter(filter, &fn, &support)) return 0;
  return resample_ksize_host(in_size, out_size, support);
}

extern "C" int dfw_resample_coeffs_ex(int32_t in_size, int32_t out_size, int32_t filter, int32_t* bounds,
                                      int32_t* coeffs) {
  resample_filter_fn fn;
  double support;
  if (!resample_filter(filter, &fn, &support)) return DFW_EINVAL;
  return resample_coeffs_host(in_size, out_size, fn, support, bounds, coeffs);
}

// What the items of one call are checked against: how many bytes each buffer holds, and which buffers the call uses.
struct native_caps {
  size_t weights_bytes, tmp_cap;   // tmp_cap: the horizontal intermediates' part of tmp
  bool need_res;                   // the resized bytes are written
  size_t res_cap;
  bool need_pred;                  // pred / labels are written
  size_t pred_bytes;
  bool counts;                     // the ground truth is read
  size_t gt_bytes;
};
// What the launches are sized by, and the extent of one plane-of-3 in tmp / in the resized bytes.
struct native_extents {
  int max_h = 0, max_w = 0;
  long long max_hw = 0;
  uint64_t tmp_ext = 0, res_ext = 0;
};

// The host mirror of the items, checked before any launch.  Returns the error.
static int native_items_check(const void* items_host, int B, int Hs, int Ws, const native_caps& c, native_extents* x) {
  const dfw_native_item* it = (const dfw_native_item*)items_host;
  for (int i = 0; i < B; ++i) {
    const dfw_native_item& t = it[i];
    if (t.h <= 0 || t.w <= 0) return DFW_EINVAL;
    if (t.h > 65535 || t.w > 65535) return DFW_ERANGE;
    if (c.counts && t.gt_elem != 1 && t.gt_elem != 4) return DFW_EINVAL;
    if (t.xk != dfw_resample_ksize_ex(Ws, t.w, DFW_FILTER_BICUBIC) || t.yk != dfw_resample_ksize_ex(Hs, t.h, DFW_FILTER_BICUBIC))
      return DFW_ESHAPE;
    if (((t.xb_off | t.xc_off | t.yb_off | t.yc_off) & 3) != 0) return DFW_ESHAPE;
    const uint64_t hw = (uint64_t)t.h * t.w;
    if (!extent_fits(t.xb_off, 8ull * t.w, c.weights_bytes) || !extent_fits(t.xc_off, 4ull * t.w * t.xk, c.weights_bytes) ||
        !extent_fits(t.yb_off, 8ull * t.h, c.weights_bytes) || !extent_fits(t.yc_off, 4ull * t.h * t.yk, c.weights_bytes))
      return DFW_EWORKSPACE;
    if (!extent_fits(t.tmp_off, 3ull * Hs * t.w, c.tmp_cap)) return DFW_EWORKSPACE;
    if (c.need_res && !extent_fits(t.u8_off, 3ull * hw, c.res_cap)) return DFW_EWORKSPACE;
    if (c.need_pred && !extent_fits(t.pred_off, hw, c.pred_bytes)) return DFW_EWORKSPACE;
    if (c.counts) {
      if (t.gt_elem == 4 && (t.gt_off & 3) != 0) return DFW_ESHAPE;
      if (!extent_fits(t.gt_off, hw * t.gt_elem, c.gt_bytes)) return DFW_EWORKSPACE;
    }
    const uint64_t te = (uint64_t)t.tmp_off + 3ull * Hs * t.w, re = (uint64_t)t.u8_off + 3ull * hw;
    x->tmp_ext = te > x->tmp_ext ? te : x->tmp_ext;
    x->res_ext = re > x->res_ext ? re : x->res_ext;
    x->max_h = t.h > x->max_h ? t.h : x->max_h;
    x->max_w = t.w > x->max_w ? t.w : x->max_w;
    x->max_hw = (long long)hw > x->max_hw ? (long long)hw : x->max_hw;
  }
  return 0;
}

// `planes` planes-of-3 per item (classes, or positions of the longest candidate list), plane p lying p strides after
// plane 0: a stride holds one plane, and the last plane ends inside its buffer.
static int native_strides_check(int planes, size_t tmp_stride, size_t res_stride, const native_caps& c,
                                const native_extents& x) {
  const uint64_t more = planes > 1 ? (uint64_t)(planes - 1) : 0;
  if (tmp_stride < x.tmp_ext || res_stride < x.res_ext) return DFW_EWORKSPACE;
  if (more && (tmp_stride > (c.tmp_cap - x.tmp_ext) / more || res_stride > (c.res_cap - x.res_ext) / more))
    return DFW_EWORKSPACE;
  return 0;
}

// grid x of the count / label kernels: 4 pixels a thread, at most 64 workgroups an image
static int native_count_blocks(long long max_hw) {
  const long long cx = (max_hw / 4 + 255) / 256;
  return cx > 64 ? 64 : (cx < 1 ? 1 : (int)cx);
}

extern "C" int dfw_seg_native(const dfw_seg_native_args* a, dfw_stream_t stream) {
  if (!a || !a->seg_u8 || !a->items || !a->items_host || !a->weights || !a->tmp) return DFW_EINVAL;
  if (a->B <= 0 || a->Hs <= 0 || a->Ws <= 0) return DFW_EINVAL;
  const bool count_stage = a->pred || a->counts;
  if (!a->out_u8 && !a->mx && !count_stage) return DFW_EINVAL;   // nothing to produce
  if (a->counts && !a->gt) return DFW_EINVAL;
  if (count_stage && a->r_threshold > 0.f && !a->mx) return DFW_EINVAL;
  // as dfw_seg_postprocess_ex: with neither flag > 0 the reference leaves the mask un-thresholded
  if (count_stage && !(a->r_threshold > 0.f) && !(a->threshold > 0.f)) return DFW_EINVAL;
  if (a->B > 65535 || a->Hs > 65535 || a->Ws > 65535) return DFW_ERANGE;
  // the resized bytes go to out_u8, or (where a later stage needs them) behind the horizontal intermediates in tmp
  const bool need_res = a->out_u8 || count_stage, in_tmp = !a->out_u8 && need_res;
  uint8_t* res = a->out_u8 ? a->out_u8 : (need_res ? a->tmp + a->tmp_res_off : nullptr);
  if (in_tmp && a->tmp_res_off > a->tmp_bytes) return DFW_EWORKSPACE;
  const native_caps caps = {a->weights_bytes, in_tmp ? a->tmp_res_off : a->tmp_bytes,
                            need_res, a->out_u8 ? a->out_u8_bytes : a->tmp_bytes - (in_tmp ? a->tmp_res_off : 0),
                            a->pred != nullptr, a->pred_bytes, a->counts != nullptr, a->gt_bytes};
  native_extents x;
  if (int e = native_items_check(a->items_host, a->B, a->Hs, a->Ws, caps, &x)) return e;
  hipStream_t st = (hipStream_t)stream;
  const dfw_native_item* items = (const dfw_native_item*)a->items;
  const int B = a->B;
  if (int e = seg_zero_launch(st, a->mx, B, a->counts, 4 * B)) return e;
  const dim3 blk(64, 4);
  hipLaunchKernelGGL(native_h_kernel, dim3((x.max_w + 255) / 256, (3 * a->Hs + 3) / 4, B), blk, 0, st, a->seg_u8, items,
                     a->weights, a->tmp, a->Hs, a->Ws, B, (size_t)0);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(native_v_kernel, dim3((x.max_w + 255) / 256, (3 * x.max_h + 3) / 4, B), blk, 0, st, items, a->weights,
                     (const uint8_t*)a->tmp, res, a->mx, a->Hs, B, (size_t)0, (size_t)0);
  DFW_CHECK_LAUNCH();
  if (count_stage) {
    hipLaunchKernelGGL(native_count_kernel, dim3(native_count_blocks(x.max_hw), B), dim3(256), 0, st, items,
                       (const uint8_t*)res, a->gt, (const uint32_t*)a->mx, a->pred, (long long*)a->counts, a->r_threshold,
                       a->threshold, a->batch_max ? 1 : 0);
    DFW_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int dfw_seg_labels_native(const dfw_seg_labels_native_args* a, dfw_stream_t stream) {
  if (!a || !a->seg_u8 || !a->items || !a->items_host || !a->weights || !a->tmp || !a->labels) return DFW_EINVAL;
  if (a->N < 1 || a->N > 254 || a->B <= 0 || a->Hs <= 0 || a->Ws <= 0) return DFW_EINVAL;
  if (a->counts && !a->gt) return DFW_EINVAL;
  if (a->r_threshold > 0.f && !a->mx) return DFW_EINVAL;
  if (!(a->r_threshold > 0.f) && !(a->threshold > 0.f)) return DFW_EINVAL;   // as dfw_seg_native
  if (a->B > 65535 || a->Hs > 65535 || a->Ws > 65535) return DFW_ERANGE;
  if ((long long)a->N * a->B > 65535) return DFW_ERANGE;                    // grid z = N * B
  // the resized bytes of every class are materialised (the thresholds need each plane's maximum first): in out_u8, or
  // behind the horizontal intermediates at tmp + tmp_res_off
  if (!a->out_u8 && a->tmp_res_off > a->tmp_bytes) return DFW_EWORKSPACE;
  uint8_t* res = a->out_u8 ? a->out_u8 : a->tmp + a->tmp_res_off;
  const native_caps caps = {a->weights_bytes, a->out_u8 ? a->tmp_bytes : a->tmp_res_off,
                            true, a->out_u8 ? a->out_u8_bytes : a->tmp_bytes - a->tmp_res_off,
                            true, a->labels_bytes, a->counts != nullptr, a->gt_bytes};
  native_extents x;
  if (int e = native_items_check(a->items_host, a->B, a->Hs, a->Ws, caps, &x)) return e;
  if (int e = native_strides_check(a->N, a->tmp_cls_stride, a->u8_cls_stride, caps, x)) return e;
  hipStream_t st = (hipStream_t)stream;
  const dfw_native_item* items = (const dfw_native_item*)a->items;
  const int N = a->N, B = a->B;
  if (int e = seg_zero_launch(st, a->mx, N * B, a->counts, B * 2 * (N + 1))) return e;
  const dim3 blk(64, 4);
  hipLaunchKernelGGL(native_h_kernel, dim3((x.max_w + 255) / 256, (3 * a->Hs + 3) / 4, N * B), blk, 0, st, a->seg_u8, items,
                     a->weights, a->tmp, a->Hs, a->Ws, B, a->tmp_cls_stride);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(native_v_kernel, dim3((x.max_w + 255) / 256, (3 * x.max_h + 3) / 4, N * B), blk, 0, st, items,
                     a->weights, (const uint8_t*)a->tmp, res, a->mx, a->Hs, B, a->tmp_cls_stride, a->u8_cls_stride);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(native_labels_kernel, dim3(native_count_blocks(x.max_hw), B), dim3(256), 0, st, items,
                     (const uint8_t*)res, a->u8_cls_stride, a->gt, (const uint32_t*)a->mx, a->class_ids, a->labels,
                     (unsigned long long*)a->counts, N, a->r_threshold, a->threshold, a->batch_max ? 1 : 0);
  DFW_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfw_seg_labels_cand_native(const dfw_seg_labels_cand_native_args* a, dfw_stream_t stream) {
  if (!a || !a->seg_u8 || !a->tab || !a->tab_host || !a->items || !a->items_host || !a->weights || !a->tmp || !a->labels)
    return DFW_EINVAL;
  if (a->B < 1 || a->E_cap < 1 || a->Hs < 1 || a->Ws < 1 || a->nlabels < 1 || a->nlabels > 254) return DFW_EINVAL;
  if (a->counts && !a->gt) return DFW_EINVAL;
  if (a->class_ids && a->entry_ids) return DFW_EINVAL;
  if (a->r_threshold > 0.f && !a->mx) return DFW_EINVAL;
  if (!(a->r_threshold > 0.f) && !(a->threshold > 0.f)) return DFW_EINVAL;
  // before the table is read: it is B + 1 + E_cap words
  if (a->B > 65535 || a->Hs > 65535 || a->Ws > 65535 || a->E_cap > (1 << 24)) return DFW_ERANGE;
  int K, E;   // the longest list: the planes of the workspace; the entries: grid z
  if (int e = cand_table_check(a->tab_host, a->B, a->E_cap, a->nlabels, &K, &E)) return e;
  if (E > 65535) return DFW_ERANGE;
  if (!a->out_u8 && a->tmp_res_off > a->tmp_bytes) return DFW_EWORKSPACE;
  uint8_t* res = a->out_u8 ? a->out_u8 : a->tmp + a->tmp_res_off;
  const native_caps caps = {a->weights_bytes, a->out_u8 ? a->tmp_bytes : a->tmp_res_off,
                            true, a->out_u8 ? a->out_u8_bytes : a->tmp_bytes - a->tmp_res_off,
                            true, a->labels_bytes, a->counts != nullptr, a->gt_bytes};
  native_extents x;
  if (int e = native_items_check(a->items_host, a->B, a->Hs, a->Ws, caps, &x)) return e;
  if (int e = native_strides_check(K, a->tmp_cls_stride, a->u8_cls_stride, caps, x)) return e;
  hipStream_t st = (hipStream_t)stream;
  const dfw_native_item* items = (const dfw_native_item*)a->items;
  const int B = a->B;
  if (int e = seg_zero_launch(st, a->mx, a->E_cap, a->counts, B * 2 * (a->nlabels + 1), a->area, 2 * a->E_cap)) return e;
  if (E > 0) {   // K >= 1
    const dim3 blk(64, 4);
    hipLaunchKernelGGL(native_h_cand_kernel, dim3((x.max_w + 255) / 256, (3 * a->Hs + 3) / 4, E), blk, 0, st, a->seg_u8,
                       items, a->tab, a->weights, a->tmp, a->Hs, a->Ws, B, K, a->tmp_cls_stride);
    DFW_CHECK_LAUNCH();
    hipLaunchKernelGGL(native_v_cand_kernel, dim3((x.max_w + 255) / 256, (3 * x.max_h + 3) / 4, E), blk, 0, st, items,
                       a->tab, a->weights, (const uint8_t*)a->tmp, res, a->mx, a->Hs, B, K, a->tmp_cls_stride,
                       a->u8_cls_stride);
    DFW_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(native_labels_cand_kernel, dim3(native_count_blocks(x.max_hw), B), dim3(256), 0, st, items,
                     (const uint8_t*)res, a->u8_cls_stride, a->gt, (const uint32_t*)a->mx, a->tab, a->class_ids,
                     a->entry_ids, a->labels, (unsigned long long*)a->counts, (unsigned long long*)a->area, a->E_cap, K,
                     a->nlabels, a->r_threshold, a->threshold);
  DFW_CHECK_LAUNCH();
  return 0;
}
