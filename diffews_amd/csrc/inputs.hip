// Input transform on the GPU: what evaluation_util/data/dataset.py:36-40 and coco.py:36-46 do on
// the host per image -- PIL bilinear Resize((S,S)) -> ToTensor -> Normalize(0.5, 0.5), and nearest resize of the
// binarised class mask -- as three small integer stages, bit-exact with Pillow's ImagingResample (8 bits per channel) and
// ATen's nearest.  The output-side counterpart is seg_native.hip.
//
// Pillow's resize is separable with a uint8 intermediate [H][out_w][3]: horizontal pass, then vertical, each output
// sample = clip8((2^21 + sum_x pixel[xmin + x] * k[x]) >> 22) with fixed-point weights k = int(0.5 + w * 2^22) of a
// triangle filter whose support scales with the reduction factor.  The weights are computed on the host in double exactly
// as Resample.c does (dfw_resample_coeffs, resample_host.h) and travel with the image bytes in one H2D copy; ToTensor +
// Normalize of a byte is a 256-entry table supplied by the caller (computed by torch itself -> same bits).  The nearest
// index is min((int)floorf((float)o * scale), size - 1) with scale = (float)in / out in float (ATen
// compute_scales_value<float>).  HBM-bound integer/byte work: a 640x480 JPEG is 0.9 MB in, 3 MB out.
//
// Each stage's arithmetic exists ONCE, as a __device__ function over resolved pointers.  Two sets of thin __global__
// wrappers feed it: the per-item entry points (dfw_image_to_tensor / dfw_mask_to_tensor) pass their arguments through;
// the ragged-batch entry point (dfw_inputs_to_tensor) resolves them from dfw_input_image_item[n_img] /
// dfw_input_mask_item[n_mask] -- grid z = item, x / y sized for the largest one, threads beyond an item's own rows exit:
// three launches whatever the batch holds.  The host mirrors of both tables are validated before the first launch.
#include "common.h"
#include "resample_host.h"
#include <math.h>

namespace dfw {

__device__ __forceinline__ int input_clip8(int acc) { return min(max(acc >> kResamplePrecisionBits, 0), 255); }

// horizontal: thread = (row y, output column xo), 3 interleaved channels
__device__ __forceinline__ void input_h(const uint8_t* __restrict__ src, uint8_t* __restrict__ tmp,
                                        const int32_t* __restrict__ bounds, const int32_t* __restrict__ coef, int ksize,
                                        int W, int out_w, int xo, int y) {
  if (xo >= out_w) return;
  const int x0 = bounds[2 * xo], n = bounds[2 * xo + 1];
  const int32_t* k = coef + (size_t)xo * ksize;
  int a0 = 1 << (kResamplePrecisionBits - 1), a1 = a0, a2 = a0;
  const uint8_t* row = src + ((size_t)y * W + x0) * 3;
  for (int x = 0; x < n; ++x) {
    const int kv = k[x];
    a0 += row[3 * x] * kv;
    a1 += row[3 * x + 1] * kv;
    a2 += row[3 * x + 2] * kv;
  }
  uint8_t* o = tmp + ((size_t)y * out_w + xo) * 3;
  o[0] = (uint8_t)input_clip8(a0);
  o[1] = (uint8_t)input_clip8(a1);
  o[2] = (uint8_t)input_clip8(a2);
}

// vertical + ToTensor/Normalize table: thread = (output row yo, output column xo), planar fp32 out
__device__ __forceinline__ void input_v(const uint8_t* __restrict__ tmp, float* __restrict__ dst,
                                        const int32_t* __restrict__ bounds, const int32_t* __restrict__ coef, int ksize,
                                        int out_h, int out_w, const float* __restrict__ lut, int xo, int yo) {
  if (xo >= out_w) return;
  const int y0 = bounds[2 * yo], n = bounds[2 * yo + 1];
  const int32_t* k = coef + (size_t)yo * ksize;
  int a0 = 1 << (kResamplePrecisionBits - 1), a1 = a0, a2 = a0;
  const uint8_t* col = tmp + ((size_t)y0 * out_w + xo) * 3;
  for (int y = 0; y < n; ++y) {
    const uint8_t* px = col + (size_t)y * out_w * 3;
    const int kv = k[y];
    a0 += px[0] * kv;
    a1 += px[1] * kv;
    a2 += px[2] * kv;
  }
  const size_t plane = (size_t)out_h * out_w, o = (size_t)yo * out_w + xo;
  dst[o] = lut[input_clip8(a0)];
  dst[plane + o] = lut[input_clip8(a1)];
  dst[2 * plane + o] = lut[input_clip8(a2)];
}

// class-id map -> binary (== class_value) -> nearest resize; +-1 on three planes (pm1) and/or 0/1 bytes (bin)
__device__ __forceinline__ void input_mask(const uint8_t* __restrict__ src, int elem, int H, int W, int class_value,
                                           int out_h, int out_w, float* __restrict__ pm1, uint8_t* __restrict__ bin,
                                           int xo, int yo) {
  if (xo >= out_w) return;
  const float sy = (float)H / out_h, sx = (float)W / out_w;   // ATen compute_scales_value<float>
  const int iy = min((int)floorf((float)yo * sy), H - 1), ix = min((int)floorf((float)xo * sx), W - 1);
  const size_t e = (size_t)iy * W + ix;
  const int id = elem == 4 ? ((const int32_t*)src)[e] : (int)src[e];
  const int on = id == class_value;
  const size_t plane = (size_t)out_h * out_w, o = (size_t)yo * out_w + xo;
  if (bin) bin[o] = (uint8_t)on;
  if (pm1) {
    const float v = on ? 1.f : -1.f;
    pm1[o] = v;
    pm1[plane + o] = v;
    pm1[2 * plane + o] = v;
  }
}

// ---- one item per launch: the arguments are the pointers
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ tmp,
                                                         const int32_t* __restrict__ bounds,
                                                         const int32_t* __restrict__ coef, int ksize, int W, int out_w) {
  input_h(src, tmp, bounds, coef, ksize, W, out_w, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t* __restrict__ tmp, float* __restrict__ dst,
                                                         const int32_t* __restrict__ bounds,
                                                         const int32_t* __restrict__ coef, int ksize, int out_h,
                                                         int out_w, const float* __restrict__ lut) {
  input_v(tmp, dst, bounds, coef, ksize, out_h, out_w, lut, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(256) void mask_nearest_kernel(const uint8_t* __restrict__ mask, int elem, int H, int W,
                                                           int class_value, int out_h, int out_w,
                                                           float* __restrict__ pm1, uint8_t* __restrict__ bin) {
  input_mask(mask, elem, H, W, class_value, out_h, out_w, pm1, bin, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

// ---- a ragged batch per launch: item blockIdx.z of a device table says where its bytes lie
__global__ __launch_bounds__(256) void inputs_h_kernel(const dfw_input_image_item* __restrict__ items,
                                                       const uint8_t* __restrict__ staged, uint8_t* __restrict__ tmp,
                                                       int out_w) {
  const dfw_input_image_item it = items[blockIdx.z];
  if (blockIdx.y >= it.H) return;   // grid y is the tallest image's
  input_h(staged + it.src_off, tmp + it.tmp_off, (const int32_t*)(staged + it.xb_off),
          (const int32_t*)(staged + it.xc_off), it.xk, it.W, out_w, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(256) void inputs_v_kernel(const dfw_input_image_item* __restrict__ items,
                                                       const uint8_t* __restrict__ staged,
                                                       const uint8_t* __restrict__ tmp, uint8_t* __restrict__ dst_base,
                                                       int out_h, int out_w, const float* __restrict__ lut) {
  const dfw_input_image_item it = items[blockIdx.z];
  input_v(tmp + it.tmp_off, (float*)(dst_base + it.dst_off), (const int32_t*)(staged + it.yb_off),
          (const int32_t*)(staged + it.yc_off), it.yk, out_h, out_w, lut, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(256) void inputs_mask_kernel(const dfw_input_mask_item* __restrict__ items,
                                                          const uint8_t* __restrict__ staged,
                                                          uint8_t* __restrict__ pm1_base, uint8_t* __restrict__ bin_base,
                                                          int out_h, int out_w) {
  const dfw_input_mask_item it = items[blockIdx.z];
  input_mask(staged + it.src_off, it.elem, it.H, it.W, it.class_value, out_h, out_w,
             it.pm1_off >= 0 ? (float*)(pm1_base + it.pm1_off) : nullptr,
             it.bin_off >= 0 ? bin_base + it.bin_off : nullptr, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

}  // namespace dfw

using namespace dfw;

// ---- host: Pillow's precompute_coeffs + normalize_coeffs_8bpc for the BILINEAR filter, whole-image box
// (the weight loop itself is resample_host.h's, shared with the output side's bicubic weights)
extern "C" int32_t dfw_resample_ksize(int32_t in_size, int32_t out_size) {
  return resample_ksize_host(in_size, out_size, 1.0);
}

extern "C" int dfw_resample_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coeffs) {
  return resample_coeffs_host(in_size, out_size, resample_bilinear, 1.0, bounds, coeffs);
}

extern "C" int dfw_image_to_tensor(const dfw_image_args* a, dfw_stream_t stream) {
  if (!a || !a->src || !a->tmp || !a->dst || !a->lut) return DFW_EINVAL;
  if (!a->xbounds || !a->xcoef || !a->ybounds || !a->ycoef) return DFW_EINVAL;
  if (a->H <= 0 || a->W <= 0 || a->out_h <= 0 || a->out_w <= 0) return DFW_EINVAL;
  if (a->xk != dfw_resample_ksize(a->W, a->out_w) || a->yk != dfw_resample_ksize(a->H, a->out_h)) return DFW_ESHAPE;
  if (a->H > 65535 || a->out_h > 65535) return DFW_ERANGE;
  hipStream_t st = (hipStream_t)stream;
  const dim3 gh((a->out_w + 255) / 256, a->H), gv((a->out_w + 255) / 256, a->out_h);
  hipLaunchKernelGGL(resample_h_kernel, gh, dim3(256), 0, st, a->src, a->tmp, a->xbounds, a->xcoef, a->xk, a->W,
                     a->out_w);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(resample_v_kernel, gv, dim3(256), 0, st, (const uint8_t*)a->tmp, a->dst, a->ybounds, a->ycoef,
                     a->yk, a->out_h, a->out_w, a->lut);
  DFW_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfw_mask_to_tensor(const void* mask, int32_t elem_bytes, int32_t H, int32_t W, int32_t class_value,
                                  int32_t out_h, int32_t out_w, float* dst_pm1, uint8_t* dst_bin,
                                  dfw_stream_t stream) {
  if (!mask || (!dst_pm1 && !dst_bin) || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0) return DFW_EINVAL;
  if (elem_bytes != 1 && elem_bytes != 4) return DFW_EINVAL;
  if (out_h > 65535) return DFW_ERANGE;
  hipLaunchKernelGGL(mask_nearest_kernel, dim3((out_w + 255) / 256, out_h), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)mask, elem_bytes, H, W, class_value, out_h, out_w, dst_pm1, dst_bin);
  DFW_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfw_inputs_to_tensor(const dfw_inputs_args* a, dfw_stream_t stream) {
  if (!a || a->n_img < 0 || a->n_mask < 0 || a->n_img + (int64_t)a->n_mask == 0) return DFW_EINVAL;   // nothing to do
  if (a->out_h <= 0 || a->out_w <= 0 || !a->staged) return DFW_EINVAL;
  if (a->n_img > 0 && (!a->image_items || !a->image_items_host || !a->tmp || !a->dst || !a->lut)) return DFW_EINVAL;
  if (a->n_mask > 0 && (!a->mask_items || !a->mask_items_host)) return DFW_EINVAL;
  if (a->n_img > 65535 || a->n_mask > 65535 || a->out_h > 65535) return DFW_ERANGE;   // grid y / z
  const uint64_t plane = (uint64_t)a->out_h * (uint64_t)a->out_w;
  const dfw_input_image_item* im = (const dfw_input_image_item*)a->image_items_host;
  int max_h = 0;
  for (int i = 0; i < a->n_img; ++i) {
    const dfw_input_image_item& t = im[i];
    if (t.H <= 0 || t.W <= 0) return DFW_EINVAL;
    if (t.H > 65535) return DFW_ERANGE;
    if (t.xk != dfw_resample_ksize(t.W, a->out_w) || t.yk != dfw_resample_ksize(t.H, a->out_h)) return DFW_ESHAPE;
    if (((t.xb_off | t.xc_off | t.yb_off | t.yc_off | t.dst_off) & 3) != 0) return DFW_ESHAPE;
    if (!extent_fits(t.src_off, 3ull * t.H * t.W, a->staged_bytes) ||
        !extent_fits(t.xb_off, 8ull * a->out_w, a->staged_bytes) ||
        !extent_fits(t.xc_off, 4ull * a->out_w * t.xk, a->staged_bytes) ||
        !extent_fits(t.yb_off, 8ull * a->out_h, a->staged_bytes) ||
        !extent_fits(t.yc_off, 4ull * a->out_h * t.yk, a->staged_bytes))
      return DFW_EWORKSPACE;
    if (!extent_fits(t.tmp_off, 3ull * t.H * a->out_w, a->tmp_bytes)) return DFW_EWORKSPACE;
    if (!extent_fits(t.dst_off, 12ull * plane, a->dst_bytes)) return DFW_EWORKSPACE;
    max_h = t.H > max_h ? t.H : max_h;
  }
  const dfw_input_mask_item* mk = (const dfw_input_mask_item*)a->mask_items_host;
  for (int i = 0; i < a->n_mask; ++i) {
    const dfw_input_mask_item& t = mk[i];
    if (t.H <= 0 || t.W <= 0) return DFW_EINVAL;
    if (t.elem != 1 && t.elem != 4) return DFW_EINVAL;
    const bool has_pm1 = t.pm1_off != -1, has_bin = t.bin_off != -1;
    if (!has_pm1 && !has_bin) return DFW_EINVAL;          // a mask with neither destination
    if ((has_pm1 && !a->pm1) || (has_bin && !a->bin)) return DFW_EINVAL;
    if (t.elem == 4 && (t.src_off & 3) != 0) return DFW_ESHAPE;
    if (has_pm1 && (t.pm1_off & 3) != 0) return DFW_ESHAPE;
    if (!extent_fits(t.src_off, (uint64_t)t.H * t.W * t.elem, a->staged_bytes)) return DFW_EWORKSPACE;
    if (has_pm1 && !extent_fits(t.pm1_off, 12ull * plane, a->pm1_bytes)) return DFW_EWORKSPACE;
    if (has_bin && !extent_fits(t.bin_off, plane, a->bin_bytes)) return DFW_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const unsigned gx = (unsigned)((a->out_w + 255) / 256);
  if (a->n_img > 0) {
    const dfw_input_image_item* items = (const dfw_input_image_item*)a->image_items;
    hipLaunchKernelGGL(inputs_h_kernel, dim3(gx, max_h, a->n_img), dim3(256), 0, st, items, a->staged, a->tmp, a->out_w);
    DFW_CHECK_LAUNCH();
    hipLaunchKernelGGL(inputs_v_kernel, dim3(gx, a->out_h, a->n_img), dim3(256), 0, st, items, a->staged,
                       (const uint8_t*)a->tmp, (uint8_t*)a->dst, a->out_h, a->out_w, a->lut);
    DFW_CHECK_LAUNCH();
  }
  if (a->n_mask > 0) {
    hipLaunchKernelGGL(inputs_mask_kernel, dim3(gx, a->out_h, a->n_mask), dim3(256), 0, st,
                       (const dfw_input_mask_item*)a->mask_items, a->staged, (uint8_t*)a->pm1, a->bin, a->out_h,
                       a->out_w);
    DFW_CHECK_LAUNCH();
  }
  return 0;
}
