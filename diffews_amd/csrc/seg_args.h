// Argument checks shared by the object stages behind a label map (seg_components, seg_holes, seg_rle, seg_contours,
// seg_match, seg_scores, seg_boundary): the size rule of a map, and one table of a call's device buffers with one checker
// over it.  Host code only, nothing here touches the device.
//
// An entry point checks null pointers, scalars, sizes and the workspace itself, in that order, then lists every device
// buffer the call uses in a seg_buf table and returns what seg_check_buffers says: overlap (DFW_EINVAL) before alignment
// (DFW_ESHAPE).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/diffews_hip.h"

namespace dfw {

// The sizes every stage over a [B, H, W] map refuses: DFW_EINVAL before DFW_ERANGE.  Grid y or z carries B and the rows'
// tiles; H * W <= 2^30 keeps every position of an image, HW itself and the padded block counts in an int.
inline int seg_map_size_error(long long B, long long H, long long W) {
  if (B < 1 || H < 1 || W < 1) return DFW_EINVAL;
  if (H > 65535 || W > 65535 || H * W > (1ll << 30) || B > 65535) return DFW_ERANGE;
  return 0;
}

// Two byte ranges [p, p + pn) and [q, q + qn) share a byte; a null or an empty one shares none.
inline bool seg_overlap(const void* p, size_t pn, const void* q, size_t qn) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p && q && pn && qn && a < b + qn && b < a + pn;
}

// One device buffer of a call.  A null pointer or zero bytes: absent, it takes part in nothing.  align 0 or 1: any address.
// The workspace is a written buffer of the bytes the stage's query returns, whatever ws_bytes says.
struct seg_buf {
  const void* p;
  size_t bytes;
  size_t align;
  bool written;
};
inline seg_buf seg_in(const void* p, size_t bytes, size_t align = 1) { return {p, bytes, align, false}; }
inline seg_buf seg_out(const void* p, size_t bytes, size_t align = 1) { return {p, bytes, align, true}; }

// DFW_EINVAL when a written buffer shares a byte with any other buffer of the table (two inputs may alias each other);
// only then DFW_ESHAPE when a present pointer is off its alignment.
template <int N>
inline int seg_check_buffers(const seg_buf (&t)[N]) {
  for (int i = 0; i < N; ++i)
    for (int j = i + 1; j < N; ++j)
      if ((t[i].written || t[j].written) && seg_overlap(t[i].p, t[i].bytes, t[j].p, t[j].bytes)) return DFW_EINVAL;
  for (int i = 0; i < N; ++i)
    if (t[i].p && t[i].bytes && t[i].align > 1 && ((uintptr_t)t[i].p & (t[i].align - 1))) return DFW_ESHAPE;
  return 0;
}

// The launches of dfw_seg_components' nearest-seed stage (seeds non-null), in seg_boundary.hip, whose pair of passes they
// are.  The entry point has validated a; nothing is checked there.
int seg_nearest_launch(const dfw_seg_components_args* a, void* stream);

}  // namespace dfw
