// Host-only: Pillow's precompute_coeffs + normalize_coeffs_8bpc (Resample.c) for one axis and a whole-image box,
// parametrised by the filter function and its support.  inputs.hip (input side, bilinear) and seg_native.hip
// (output side, bicubic) both get their fixed-point weights here, so the two sides cannot drift apart.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/diffews_hip.h"

namespace dfw {

constexpr int kResamplePrecisionBits = 32 - 8 - 2;

// Resample.c bilinear_filter / bicubic_filter (a = -0.5), in double as Pillow evaluates them
inline double resample_bilinear(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}
inline double resample_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// [off, off + bytes) inside a buffer of `cap` bytes: how both sides validate an item table's offsets
inline bool extent_fits(int64_t off, uint64_t bytes, size_t cap) {
  return off >= 0 && (uint64_t)off <= (uint64_t)cap && bytes <= (uint64_t)cap - (uint64_t)off;
}

typedef double (*resample_filter_fn)(double);

// filter id (DFW_FILTER_*) -> function and support; false for an unknown id
inline bool resample_filter(int32_t filter, resample_filter_fn* fn, double* support) {
  if (filter == DFW_FILTER_BILINEAR) { *fn = resample_bilinear; *support = 1.0; return true; }
  if (filter == DFW_FILTER_BICUBIC) { *fn = resample_bicubic; *support = 2.0; return true; }
  return false;
}

inline int32_t resample_ksize_host(int32_t in_size, int32_t out_size, double filter_support) {
  if (in_size <= 0 || out_size <= 0) return 0;
  double filterscale = (double)in_size / (double)out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = filter_support * filterscale;
  return (int32_t)ceil(support) * 2 + 1;
}

// bounds [out_size][2] = (first input index, tap count), coeffs [out_size][ksize]
inline int resample_coeffs_host(int32_t in_size, int32_t out_size, resample_filter_fn filter, double filter_support,
                                int32_t* bounds, int32_t* coeffs) {
  if (in_size <= 0 || out_size <= 0 || !bounds || !coeffs) return DFW_EINVAL;
  const double scale = (double)in_size / (double)out_size;
  double filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = filter_support * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  const double ss = 1.0 / filterscale;
  double* w = (double*)malloc(sizeof(double) * ksize);
  if (!w) return DFW_EINVAL;
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) {
      w[x] = filter((x + xmin - center + 0.5) * ss);
      ww += w[x];
    }
    for (int x = 0; x < xmax; ++x)
      if (ww != 0.0) w[x] /= ww;
    for (int x = xmax; x < ksize; ++x) w[x] = 0.0;
    int32_t* k = coeffs + (size_t)xx * ksize;
    for (int x = 0; x < ksize; ++x)
      k[x] = w[x] < 0 ? (int32_t)(-0.5 + w[x] * (1 << kResamplePrecisionBits))
                      : (int32_t)(0.5 + w[x] * (1 << kResamplePrecisionBits));
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  free(w);
  return 0;
}

}  // namespace dfw
