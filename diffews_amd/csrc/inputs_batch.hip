// Input transform of a whole RAGGED batch: preprocess.hip's three kernels -- Pillow's 8-bit two-pass
// BILINEAR resize + ToTensor / Normalize table, and ATen's nearest resize of the binarised class map -- driven by two
// device-resident tables instead of one launch train per image.  Three launches whatever the batch holds: horizontal pass
// and vertical pass + table lookup over all images (grid z = image, x / y sized for the largest one, threads beyond an
// image's own rows exit), one more over all masks (grid z = mask).  Everything per item (size, where its bytes, weights,
// scratch and outputs lie) comes from dfw_input_image_item[n_img] / dfw_input_mask_item[n_mask]; the host mirrors of
// both are validated before the first launch.  The output-side counterpart is seg_native.hip.
//
// Arithmetic is exactly resample_h_kernel / resample_v_kernel / mask_nearest_kernel's: 2^21 + sum tap * weight,
// arithmetic shift by 22, clamp to 0..255, a uint8 intermediate [H][out_w][3] between the passes; the nearest index is
// min((int)floorf((float)o * scale), size - 1) with scale = (float)in / out computed in float (ATen
// compute_scales_value<float>).  Those kernels and their entry points are untouched.
#include "common.h"
#include "resample_host.h"
#include <math.h>

namespace dfw {

constexpr int kInputBits = kResamplePrecisionBits;

__device__ __forceinline__ uint8_t input_clip8(int acc) { return (uint8_t)min(max(acc >> kInputBits, 0), 255); }

// horizontal: thread = (row y of image z, output column xo), 3 interleaved channels
__global__ __launch_bounds__(256) void inputs_h_kernel(const dfw_input_image_item* __restrict__ items,
                                                       const uint8_t* __restrict__ staged, uint8_t* __restrict__ tmp,
                                                       int out_w) {
  const dfw_input_image_item it = items[blockIdx.z];
  const int xo = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (y >= it.H || xo >= out_w) return;   // grid y is the tallest image's
  const int32_t* bounds = (const int32_t*)(staged + it.xb_off);
  const int x0 = bounds[2 * xo], n = bounds[2 * xo + 1];
  const int32_t* k = (const int32_t*)(staged + it.xc_off) + (size_t)xo * it.xk;
  int a0 = 1 << (kInputBits - 1), a1 = a0, a2 = a0;
  const uint8_t* row = staged + it.src_off + ((size_t)y * it.W + x0) * 3;
  for (int x = 0; x < n; ++x) {
    const int kv = k[x];
    a0 += row[3 * x] * kv;
    a1 += row[3 * x + 1] * kv;
    a2 += row[3 * x + 2] * kv;
  }
  uint8_t* o = tmp + it.tmp_off + ((size_t)y * out_w + xo) * 3;
  o[0] = input_clip8(a0);
  o[1] = input_clip8(a1);
  o[2] = input_clip8(a2);
}

// vertical + ToTensor/Normalize table: thread = (output row yo, output column xo) of image z, planar fp32 out
__global__ __launch_bounds__(256) void inputs_v_kernel(const dfw_input_image_item* __restrict__ items,
                                                       const uint8_t* __restrict__ staged,
                                                       const uint8_t* __restrict__ tmp, uint8_t* __restrict__ dst_base,
                                                       int out_h, int out_w, const float* __restrict__ lut) {
  const dfw_input_image_item it = items[blockIdx.z];
  const int xo = blockIdx.x * 256 + threadIdx.x, yo = blockIdx.y;
  if (xo >= out_w) return;
  const int32_t* bounds = (const int32_t*)(staged + it.yb_off);
  const int y0 = bounds[2 * yo], n = bounds[2 * yo + 1];
  const int32_t* k = (const int32_t*)(staged + it.yc_off) + (size_t)yo * it.yk;
  int a0 = 1 << (kInputBits - 1), a1 = a0, a2 = a0;
  const uint8_t* col = tmp + it.tmp_off + ((size_t)y0 * out_w + xo) * 3;
  for (int y = 0; y < n; ++y) {
    const uint8_t* px = col + (size_t)y * out_w * 3;
    const int kv = k[y];
    a0 += px[0] * kv;
    a1 += px[1] * kv;
    a2 += px[2] * kv;
  }
  float* dst = (float*)(dst_base + it.dst_off);
  const size_t plane = (size_t)out_h * out_w, o = (size_t)yo * out_w + xo;
  dst[o] = lut[min(max(a0 >> kInputBits, 0), 255)];
  dst[plane + o] = lut[min(max(a1 >> kInputBits, 0), 255)];
  dst[2 * plane + o] = lut[min(max(a2 >> kInputBits, 0), 255)];
}

// class-id map z -> binary (== class_value) -> nearest resize; +-1 on three planes and/or 0/1 bytes
__global__ __launch_bounds__(256) void inputs_mask_kernel(const dfw_input_mask_item* __restrict__ items,
                                                          const uint8_t* __restrict__ staged,
                                                          uint8_t* __restrict__ pm1_base, uint8_t* __restrict__ bin_base,
                                                          int out_h, int out_w) {
  const dfw_input_mask_item it = items[blockIdx.z];
  const int xo = blockIdx.x * 256 + threadIdx.x, yo = blockIdx.y;
  if (xo >= out_w) return;
  const float sy = (float)it.H / out_h, sx = (float)it.W / out_w;   // ATen compute_scales_value<float>
  const int iy = min((int)floorf((float)yo * sy), it.H - 1), ix = min((int)floorf((float)xo * sx), it.W - 1);
  const size_t e = (size_t)iy * it.W + ix;
  const uint8_t* src = staged + it.src_off;
  const int id = it.elem == 4 ? ((const int32_t*)src)[e] : (int)src[e];
  const int on = id == it.class_value;
  const size_t plane = (size_t)out_h * out_w, o = (size_t)yo * out_w + xo;
  if (it.bin_off >= 0) bin_base[it.bin_off + o] = (uint8_t)on;
  if (it.pm1_off >= 0) {
    float* pm1 = (float*)(pm1_base + it.pm1_off);
    const float v = on ? 1.f : -1.f;
    pm1[o] = v;
    pm1[plane + o] = v;
    pm1[2 * plane + o] = v;
  }
}

}  // namespace dfw

using namespace dfw;

// [off, off + bytes) inside a buffer of `cap` bytes
static bool inputs_fits(int64_t off, uint64_t bytes, size_t cap) {
  return off >= 0 && (uint64_t)off <= (uint64_t)cap && bytes <= (uint64_t)cap - (uint64_t)off;
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
    if (!inputs_fits(t.src_off, 3ull * t.H * t.W, a->staged_bytes) ||
        !inputs_fits(t.xb_off, 8ull * a->out_w, a->staged_bytes) ||
        !inputs_fits(t.xc_off, 4ull * a->out_w * t.xk, a->staged_bytes) ||
        !inputs_fits(t.yb_off, 8ull * a->out_h, a->staged_bytes) ||
        !inputs_fits(t.yc_off, 4ull * a->out_h * t.yk, a->staged_bytes))
      return DFW_EWORKSPACE;
    if (!inputs_fits(t.tmp_off, 3ull * t.H * a->out_w, a->tmp_bytes)) return DFW_EWORKSPACE;
    if (!inputs_fits(t.dst_off, 12ull * plane, a->dst_bytes)) return DFW_EWORKSPACE;
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
    if (!inputs_fits(t.src_off, (uint64_t)t.H * t.W * t.elem, a->staged_bytes)) return DFW_EWORKSPACE;
    if (has_pm1 && !inputs_fits(t.pm1_off, 12ull * plane, a->pm1_bytes)) return DFW_EWORKSPACE;
    if (has_bin && !inputs_fits(t.bin_off, plane, a->bin_bytes)) return DFW_EWORKSPACE;
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
