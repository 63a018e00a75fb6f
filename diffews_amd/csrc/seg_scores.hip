// Per-object confidence (objects.object_scores): the decoder's uint8 mask planes reduced over an id map, per object and
// exact.  ids int32 [B][H][W], labels uint8 [B][H][W], seg_u8 uint8 [P][3][H][W], planes int32 [B][nlabels + 1] ->
// scores int64 [B][cap][4] = (sum, counted pixels, min, max) of s = u0 + u1 + u2 over the counted pixels of every object.
// All integers: the result depends on no order of execution.
//
// A pixel at q = y * W + x is COUNTED when 1 <= id <= cap, l = labels[q] lies in 1..nlabels and g = planes[b][l] lies in
// 0..P-1; its value is the sum of the three bytes of plane group g at q (0..765).  Its KEY is its id when counted and 0
// otherwise; a PIECE is a maximal interval of equal non-zero keys inside one block of kSegPix positions.  The piece is
// the unit that reaches global memory: one set of integer atomics (64-bit add of the sum, 32-bit add of the count, 32-bit
// max of 765 - s and of s) into the accumulators of its object, never one per pixel.  A 4096 x 4096 map that is one object
// issues 8192 sets, not 16.8 M.  The minimum is accumulated as the maximum of 765 - s, so that zero is the identity of all
// four fields and a row nobody added to needs no special value.
//
// The workspace is sum [B * cap] (64-bit, at the first 8-byte boundary of ws) | cnt | inv | mx [B * cap] (32-bit each).
// Launches, three whatever the image holds, no host readback in between:
//
//   0  scores_init_kernel     zeroes the accumulators (a library kernel, no memset node)
//   1  scores_reduce_kernel   per block of kSegPix positions, 8 per thread of 256:
//                               - the image's row of the plane table goes to LDS, clamped: an entry outside 0..P-1 is -1
//                               - ids as two 16-byte loads, labels and (when the thread's counted pixels share one plane
//                                 group) the three plane rows as 8-byte loads, where the addresses allow; else by element
//                               - a thread folds its equal neighbouring keys.  A piece with both ends inside the thread
//                                 is complete and goes out at once; the piece at its first position (HEAD) and the one at
//                                 its last (TAIL) may go on in the neighbours.  A thread of one key is all tail
//                               - a wave64 segmented inclusive scan of the tails (shuffles; a tail joins the one before it
//                                 when its thread is of one key and that key is the previous thread's last), then the
//                                 carry across the four waves through LDS
//                               - a tail that the next thread does not continue goes out; a head takes the scanned tail
//                                 of the previous thread when the keys agree, and goes out
//   2  scores_finish_kernel   row = (sum, cnt, cnt ? 765 - inv : 0, mx): every row 0..cap-1 of every image is written
//
// Termination: no thread waits for another thread or workgroup; every loop has a trip count fixed at compile time.  Any
// grid is correct at any residency.
#include "seg_args.h"
#include "seg_sort.h"

namespace dfw {

constexpr int kScoreMax = 765;   // 3 * 255

using u32x2 = unsigned __attribute__((ext_vector_type(2)));

// (sum, count, max of 765 - s, max of s) of a set of counted pixels; zeros for the empty set.
struct score_acc {
  int sum, n, inv, mx;
};
__device__ __forceinline__ score_acc score_join(score_acc a, score_acc b) {
  return {a.sum + b.sum, a.n + b.n, max(a.inv, b.inv), max(a.mx, b.mx)};
}
__device__ __forceinline__ score_acc score_shfl_up(score_acc a, int d) {
  return {__shfl_up(a.sum, d, 64), __shfl_up(a.n, d, 64), __shfl_up(a.inv, d, 64), __shfl_up(a.mx, d, 64)};
}

struct score_ws {
  unsigned long long* sum;   // [B * cap]
  uint32_t *cnt, *inv, *mx;  // [B * cap] each
};
__host__ __device__ __forceinline__ score_ws score_split(void* ws, size_t rows) {
  score_ws w;
  w.sum = (unsigned long long*)(((uintptr_t)ws + 7) & ~(uintptr_t)7);
  w.cnt = (uint32_t*)(w.sum + rows);
  w.inv = w.cnt + rows;
  w.mx = w.inv + rows;
  return w;
}

// One piece of object `key` (1..cap, so the row exists) of image b.
__device__ __forceinline__ void score_flush(const score_ws& w, size_t row0, int key, score_acc a) {
  const size_t r = row0 + key - 1;
  atomicAdd(&w.sum[r], (unsigned long long)a.sum);
  atomicAdd(&w.cnt[r], (uint32_t)a.n);
  atomicMax(&w.inv[r], (uint32_t)a.inv);
  atomicMax(&w.mx[r], (uint32_t)a.mx);
}

__global__ __launch_bounds__(256) void scores_init_kernel(uint32_t* words, int n) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) words[e] = 0u;
}

__global__ __launch_bounds__(256) void scores_reduce_kernel(const int32_t* ids, const uint8_t* labels, const uint8_t* u8,
                                                            const int32_t* planes, void* ws, int HW, int cap, int nlabels,
                                                            int P) {
  __shared__ int tab[256];          // label byte -> plane group, -1 for "not counted"
  __shared__ int kfirst[256], klast[256];
  __shared__ int tails[256][4];     // the scanned tail of every thread
  __shared__ int wtail[4][4];       // the scanned tail of every wave's last lane
  __shared__ int wopen[4];          // that wave is one segment that goes on from the wave before
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.y;
  const int p0 = blockIdx.x * kSegPix + t * 8;
  {
    int g = -1;
    if (t >= 1 && t <= nlabels) {
      g = planes[(size_t)b * (nlabels + 1) + t];
      if ((unsigned)g >= (unsigned)P) g = -1;
    }
    tab[t] = g;
  }
  const int32_t* idp = ids + (size_t)b * HW + p0;
  const uint8_t* lp = labels + (size_t)b * HW + p0;
  const bool full = p0 + 8 <= HW;
  int id[8], lab[8];
  if (full && ((uintptr_t)idp & 15) == 0) {
    const i32x4 q0 = *(const i32x4*)idp, q1 = *(const i32x4*)(idp + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) id[j] = q0[j], id[4 + j] = q1[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) id[j] = p0 + j < HW ? idp[j] : 0;
  }
  if (full && ((uintptr_t)lp & 7) == 0) {
    const u32x2 q = *(const u32x2*)lp;
#pragma unroll
    for (int j = 0; j < 4; ++j) lab[j] = (q[0] >> (8 * j)) & 255, lab[4 + j] = (q[1] >> (8 * j)) & 255;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) lab[j] = p0 + j < HW ? lp[j] : 0;
  }
  __syncthreads();                  // tab
  // the plane group of every counted pixel, -1 for the others; `one` = the counted pixels share a group (g1)
  int g[8], g1 = -1;
  bool one = true;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    g[j] = (id[j] >= 1 && id[j] <= cap) ? tab[lab[j]] : -1;   // lab 0 and lab > nlabels hold -1; outside HW id is 0
    if (g[j] >= 0) {
      if (g1 < 0) g1 = g[j];
      one = one && g[j] == g1;
    }
  }
  int s[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = 0;
  if (g1 >= 0) {
    const uint8_t* u1 = u8 + (size_t)g1 * 3 * HW + p0;
    if (one && full && ((((uintptr_t)u1) | (uintptr_t)HW) & 7) == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const u32x2 q = *(const u32x2*)(u1 + (size_t)c * HW);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += (q[0] >> (8 * j)) & 255, s[4 + j] += (q[1] >> (8 * j)) & 255;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (g[j] >= 0) {               // counted, so p0 + j < HW and g[j] < P
          const uint8_t* u = u8 + (size_t)g[j] * 3 * HW + p0 + j;
          s[j] = u[0] + u[HW] + u[2 * (size_t)HW];
        }
    }
  }
  int key[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) key[j] = g[j] >= 0 ? id[j] : 0;

  const score_ws w = score_split(ws, (size_t)gridDim.y * cap);
  const size_t row0 = (size_t)b * cap;
  // the thread's pieces: the first one is kept as the head, the last one as the tail, the others are complete
  score_acc cur = {s[0], key[0] != 0, kScoreMax - s[0], s[0]}, head = {0, 0, 0, 0};
  if (key[0] == 0) cur = {0, 0, 0, 0};
  bool uniform = true;
#pragma unroll
  for (int j = 1; j < 8; ++j) {
    if (key[j] != key[j - 1]) {
      if (uniform) head = cur;
      else if (key[j - 1] != 0) score_flush(w, row0, key[j - 1], cur);
      uniform = false;
      cur = {0, 0, 0, 0};
    }
    if (key[j] != 0) cur = score_join(cur, {s[j], 1, kScoreMax - s[j], s[j]});
  }
  kfirst[t] = key[0];
  klast[t] = key[7];
  __syncthreads();
  const int kprev = t > 0 ? klast[t - 1] : -1, knext = t < 255 ? kfirst[t + 1] : -1;   // -1 is no key
  // a tail starts a segment unless its thread is of one key and goes on from the thread before
  int flag = !(uniform && key[0] == kprev);
  score_acc v = cur;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const score_acc up = score_shfl_up(v, d);
    const int upf = __shfl_up(flag, d, 64);
    if (lane >= d && !flag) {
      v = score_join(up, v);
      flag = upf;
    }
  }
  // flag == 0 now: no segment starts in lanes 0..lane, the tail goes on from the wave before
  if (lane == 63) {
    wtail[wave][0] = v.sum, wtail[wave][1] = v.n, wtail[wave][2] = v.inv, wtail[wave][3] = v.mx;
    wopen[wave] = !flag;
  }
  __syncthreads();
  if (!flag) {                       // wave >= 1: thread 0 always starts a segment
    score_acc carry = {0, 0, 0, 0};
    bool open = true;
#pragma unroll
    for (int u = 2; u >= 0; --u)     // the waves before, the nearest first; stop behind the first one that is not open
      if (u < wave && open) {
        carry = score_join({wtail[u][0], wtail[u][1], wtail[u][2], wtail[u][3]}, carry);
        open = wopen[u] != 0;
      }
    v = score_join(carry, v);
  }
  tails[t][0] = v.sum, tails[t][1] = v.n, tails[t][2] = v.inv, tails[t][3] = v.mx;
  __syncthreads();
  if (key[7] != 0 && knext != key[7]) score_flush(w, row0, key[7], v);
  if (!uniform && key[0] != 0) {
    if (key[0] == kprev) head = score_join({tails[t - 1][0], tails[t - 1][1], tails[t - 1][2], tails[t - 1][3]}, head);
    score_flush(w, row0, key[0], head);
  }
}

__global__ __launch_bounds__(256) void scores_finish_kernel(const void* ws, long long* scores, int rows) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const score_ws w = score_split(const_cast<void*>(ws), (size_t)rows);
  const long long n = w.cnt[r];
  long long* o = scores + 4 * (size_t)r;
  o[0] = (long long)w.sum[r];
  o[1] = n;
  o[2] = n ? kScoreMax - (long long)w.inv[r] : 0;
  o[3] = w.mx[r];
}

// The sizes dfw_seg_scores refuses: DFW_EINVAL before DFW_ERANGE.
static int scores_size_error(long long B, long long H, long long W, long long cap, long long nlabels, long long P) {
  if (B < 1 || H < 1 || W < 1 || cap < 1 || P < 1) return DFW_EINVAL;
  if (nlabels < 1 || nlabels > 254) return DFW_EINVAL;
  if (int e = seg_map_size_error(B, H, W)) return e;
  // seg_u8 is addressed in size_t: P * 3 * H * W must stay below 2^63, which int32 arguments cannot break (2^31 * 3 *
  // 2^30); the test is here for the day a size widens
  if (P > (0x7fffffffffffffffll / 3) / (H * W)) return DFW_ERANGE;
  // the init kernel counts the accumulators' 5 * B * cap words, and the finish kernel the B * cap rows, in an int; the
  // B * cap * 4 words of scores are addressed in size_t
  if (B * cap * 5 > 0x7fffffffll) return DFW_ERANGE;
  return 0;
}

}  // namespace dfw

using namespace dfw;

extern "C" size_t dfw_seg_scores_workspace_bytes(int32_t B, int32_t cap) {
  if (B < 1 || cap < 1 || B > 65535 || (long long)B * cap * 5 > 0x7fffffffll) return 0;
  return (size_t)B * cap * 20 + 8;   // 8 + 3 * 4 bytes a row, and the way to the first 8-byte boundary
}

extern "C" int dfw_seg_scores_block(int32_t* pixels) {
  if (!pixels) return DFW_EINVAL;
  *pixels = kSegPix;
  return 0;
}

extern "C" int dfw_seg_scores(const dfw_seg_scores_args* a, dfw_stream_t stream) {
  if (!a || !a->ids || !a->labels || !a->seg_u8 || !a->planes || !a->planes_host || !a->scores || !a->ws) return DFW_EINVAL;
  if (int e = scores_size_error(a->B, a->H, a->W, a->cap, a->nlabels, a->P)) return e;
  for (size_t i = 0, n = (size_t)a->B * (a->nlabels + 1); i < n; ++i)
    if (i % (a->nlabels + 1) != 0 && (a->planes_host[i] < -1 || a->planes_host[i] > a->P - 1)) return DFW_EINVAL;
  const size_t wsb = dfw_seg_scores_workspace_bytes(a->B, a->cap);
  if (a->ws_bytes < wsb) return DFW_EWORKSPACE;
  const size_t HW = (size_t)a->H * a->W, rows = (size_t)a->B * a->cap;
  const seg_buf bufs[] = {seg_in(a->ids, a->B * HW * 4, 4),
                          seg_in(a->labels, a->B * HW),
                          seg_in(a->seg_u8, (size_t)a->P * 3 * HW),
                          seg_in(a->planes, (size_t)a->B * (a->nlabels + 1) * 4, 4),   // planes_host is host memory
                          seg_out(a->scores, rows * 32, 8),
                          seg_out(a->ws, wsb, 4)};
  if (int e = seg_check_buffers(bufs)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int iHW = a->H * a->W, irows = a->B * a->cap;
  const score_ws w = score_split(a->ws, rows);
  hipLaunchKernelGGL(scores_init_kernel, dim3((5 * irows + 255) / 256), dim3(256), 0, st, (uint32_t*)w.sum, 5 * irows);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(scores_reduce_kernel, dim3((iHW + kSegPix - 1) / kSegPix, a->B), dim3(256), 0, st, a->ids, a->labels,
                     a->seg_u8, a->planes, a->ws, iHW, a->cap, a->nlabels, a->P);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(scores_finish_kernel, dim3((irows + 255) / 256), dim3(256), 0, st, (const void*)a->ws,
                     (long long*)a->scores, irows);
  DFW_CHECK_LAUNCH();
  return 0;
}
