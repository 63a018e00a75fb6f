// Boundary bands (objects.boundary_bands): the capped chessboard distance of every pixel of a label map (uint8) or an id
// map (int32) to its own contour, and the per-class counts of two such bands.  map [B][H][W] -> dist uint8 [B][H][W]:
// 0 where map == 0, else min(D, dmax + 1), D the smallest max(|dy|, |dx|) to a position that lies outside the image or
// holds another value; optionally band [B][H][W] of the map's type, the value where 1 <= dist <= d and 0 elsewhere.
// Values are compared for equality only.  All integers: the result depends on no order of execution.
//
// The exact two-pass form.  h(y, x) = min(x - run_start + 1, run_end - x) is the distance along the row to the nearest
// position that is outside the row or holds another value; then
//   D(y, x) = min(y + 1, H - y, min over dy of c(dy)),  c(dy) = max(|dy|, h(y + dy, x)) while map[y + dy][x] == v,
//                                                       c(dy) = |dy| at the first row where it differs,
// and nothing beyond that row, or beyond |dy| >= the best so far, can be smaller.  h is capped at dmax + 1 as well, which
// changes no capped D: min(max(a, min(h, c)), c) == min(max(a, h), c).
//
// Launches, two whatever the image holds, no host readback in between:
//
//   0  boundary_row_kernel<T>     per block of kBndPos consecutive positions y * W + x of one image: the window of
//                                 kBndPos + 2 * kBndHalo positions goes to LDS (16-byte / 4-byte loads of four elements where
//                                 the address allows and the four lie inside the image, else by element; outside the image
//                                 reads nothing).  A position is a BREAK when it lies outside the image, starts a row or
//                                 holds another value than its predecessor.  Each thread owns 10 positions of the window;
//                                 the last break at or before a position is an inclusive max-scan of break positions and
//                                 the next break behind it an exclusive min-scan from the right (wave64 shuffles, the four
//                                 waves through LDS).  The halo of kBndHalo >= 254 + 1 positions a side makes every capped
//                                 distance of the block's own positions final.  h goes to the workspace, one byte a pixel,
//                                 as 8-byte stores where the address allows.
//   1  boundary_col_kernel<T, V>  per tile of kBndRows x kBndCols pixels: a thread owns V pixels side by side (V = 4
//                                 through one 32-bit word of h and of a uint8 map, or 16 bytes of an int32 map, when W % 4
//                                 == 0 and every pointer is aligned for it; V = 1 otherwise) and walks dy = 1, 2, ... up
//                                 and down the column while dy < the largest best-so-far of its pixels.  The walk stays
//                                 inside the image by itself: best <= min(y + 1, H - y) from the start.  dist and band
//                                 come out of the same pass.
//
// Why plain column reads through the caches and not an LDS tile with halo: the walk of a pixel ends after D steps, so only
// the pixels deep inside an object go the whole dmax rows; at dmax = 116 a tile needs a 232-row halo, i.e. (16 + 232) x 64
// x (1 + 4) bytes = 79 KB for an id map, above the 64 KB of static LDS, and a taller tile only moves the ratio from 15x to
// 5x re-read.  A row of a tile is 64 consecutive bytes of h (one cache line) and the 15 neighbouring tile rows read the
// same lines, so the re-reads are L1 / L2 hits; profiles/object_boundaries_timing.md holds the measured cost.
//
// dfw_seg_boundary_counts: per pixel, dropped when gt > nlabels (seg_gt_byte's rule); l = pred if 1 <= pdist <= d else 0,
// g = gt if 1 <= gdist <= d else 0; pred[l]++, gt[g]++, inter[l]++ when l == g, in LDS histograms per workgroup of
// kBndCountPix positions, flushed by seg_flush_counts (seg_fuse.h) into counts [B][2][nlabels + 1] = (intersections,
// unions).  Pixels in neither band, the bulk of an image, are counted in a register and reach the histogram once per wave.
// Two launches: a library kernel zeroes counts (no memset node), then the count.  dist_elem = 2: both dist maps are the
// uint16 squared ones and the rule is 1 <= dist <= d * d (boundary_counts_kernel<uint16_t>).
//
// The Euclidean metric (metric = 1): dist is uint16 [B][H][W], 0 where map == 0, else min(D2, (dmax + 1)^2), D2 the smallest
// dy^2 + dx^2 to a position outside the image or of another value; band holds the value where 1 <= dist <= d^2.  The row
// pass and the workspace are the same, h is all the state there is:
//   D2(y, x) = min(min(y + 1, H - y)^2, min over dy of c(dy)),  c(0) = h(y, x)^2,
//   c(dy) = dy^2 + h(y + dy, x)^2 while map[y + dy][x] == v, c(dy) = dy^2 at the first row where it differs.
// Every candidate is the squared distance to a real differing position, and for a nearest one (y', x') either the column
// holds v from y to y', so that h(y', x) reaches a differing position no farther along than x', or the column differs at a
// nearer row.  A capped h only removes candidates above (dmax + 1)^2.
//
//   1' boundary_col2_kernel<T, V, P>  the tile, the V = 4 / V = 1 split and the vector condition of boundary_col_kernel (dist
//                                 aligned to four uint16), walking while dy^2 < the largest best-so-far.  P: peaks int64
//                                 [B][cap] of an id map, row k - 1 = max over the pixels of id k of (dist << 32) | (2^32 - 1
//                                 - (y * W + x)); boundary_zero_kernel clears it first (three launches then) and
//                                 bnd_peaks_wave reduces it with one atomicMax per piece of equal id of a wave's lanes, none
//                                 when the row already holds as much.
//
// The nearest seed inside the object (seg_nearest_launch, reached through dfw_seg_components with `seeds`; it lives here because
// it is this file's pair of passes): per pixel of an int32 map the seed with the smallest (dy^2 + dx^2, value) that an L path
// on the pixel's value reaches, the column first.  A row pass and a column pass of their own, described where they stand
// below, 2 * passes launches; the workspace holds a value (int32) beside h.
//
//   0" seeds_row_kernel           boundary_row_kernel's window and scans, and the same scans over the seed positions
//   1" seeds_col_kernel<V, LATER> boundary_col2_kernel's tile and V rule; walks each direction while the column holds the
//                                 value and dy^2 <= the best so far; LATER (passes 2..) keeps what a pixel already holds
//
// Termination: in dfw_seg_boundary no thread waits for another thread or workgroup and, without peaks, no atomics are
// used; every loop but the column walk has a trip count fixed at compile time, and the walk ends after at most dmax steps.
// The peaks and the counts use global (and LDS) integer atomics, order-free, and wait for nothing.  Any grid is correct at
// any residency.
#include "seg_args.h"
#include "seg_fuse.h"

namespace dfw {

constexpr int kBndPos = 2048;                          // positions a workgroup of the row pass covers
constexpr int kBndHalo = 256;                          // >= dmax + 1 for every dmax <= 254, a multiple of 16
constexpr int kBndWin = kBndPos + 2 * kBndHalo;        // 2560 = 256 threads x 10
constexpr int kBndOwn = kBndWin / 256;
constexpr int kBndRows = 16, kBndCols = 64;            // the tile of the column pass
constexpr int kBndCountPix = 4096;                     // positions a workgroup of the counts covers, 16 per thread
static_assert(kBndOwn * 256 == kBndWin && kBndHalo >= 255 && kBndPos == 256 * 8, "the row pass's layout");

using u32x2 = unsigned __attribute__((ext_vector_type(2)));

// V neighbouring elements -> ints
template <typename T, int V> __device__ __forceinline__ void bnd_load(const T* p, int (&o)[V]) {
  if constexpr (V == 1) {
    o[0] = (int)p[0];
  } else if constexpr (sizeof(T) == 1) {
    const uint32_t w = *(const uint32_t*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (int)((w >> (8 * k)) & 255u);
  } else {
    const i32x4 w = *(const i32x4*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = w[k];
  }
}
template <typename T, int V> __device__ __forceinline__ void bnd_store(T* p, const int (&o)[V]) {
  if constexpr (V == 1) {
    p[0] = (T)o[0];
  } else if constexpr (sizeof(T) == 1) {
    *(uint32_t*)p = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
  } else {
    i32x4 w;
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = o[k];
    *(i32x4*)p = w;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void boundary_row_kernel(const T* map, uint8_t* hrow, int HW, int W, int cap) {
  __shared__ __attribute__((aligned(16))) int val[kBndWin];
  __shared__ __attribute__((aligned(8))) uint8_t hb[kBndPos];
  __shared__ int wlast[4], wfirst[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int p0 = blockIdx.x * kBndPos, w0 = p0 - kBndHalo;   // the window's first position, negative in block 0
  const T* mp = map + (size_t)blockIdx.y * HW;
#pragma unroll
  for (int r = 0; r < (kBndWin / 4 + 255) / 256; ++r) {
    const int c = r * 256 + t;
    if (c < kBndWin / 4) {
      const int q = w0 + 4 * c;
      int v[4];
      if (q >= 0 && q + 4 <= HW && ((uintptr_t)(mp + q) & (4 * sizeof(T) - 1)) == 0) {
        bnd_load<T, 4>(mp + q, v);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (q + k >= 0 && q + k < HW) ? (int)mp[q + k] : 0;
      }
      i32x4 w;
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = v[k];
      *(i32x4*)(val + 4 * c) = w;
    }
  }
  __syncthreads();
  const int i0 = kBndOwn * t, q0 = w0 + i0;
  int v[kBndOwn + 1];
  v[0] = t ? val[i0 - 1] : 0;
#pragma unroll
  for (int j = 0; j < kBndOwn; ++j) v[j + 1] = val[i0 + j];
  // breaks: the window's first position is one as well, which no position of the block itself can see (kBndHalo > cap)
  int x = q0 >= 0 ? q0 % W : 0;
  int last = -1, first = kBndWin, L[kBndOwn];
  unsigned brk = 0u;
#pragma unroll
  for (int j = 0; j < kBndOwn; ++j) {
    const int q = q0 + j;
    if (q < 0 || q >= HW || x == 0 || v[j + 1] != v[j] || i0 + j == 0) {
      brk |= 1u << j;
      last = i0 + j;
      if (first == kBndWin) first = i0 + j;
    }
    L[j] = last;
    if (q >= 0 && ++x == W) x = 0;
  }
  int ls = last, fs = first;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int a = __shfl_up(ls, o, 64), c = __shfl_down(fs, o, 64);
    if (lane >= o) ls = max(ls, a);
    if (lane + o < 64) fs = min(fs, c);
  }
  if (lane == 63) wlast[wave] = ls;
  if (lane == 0) wfirst[wave] = fs;
  int before = __shfl_up(ls, 1, 64), behind = __shfl_down(fs, 1, 64);
  if (lane == 0) before = -1;
  if (lane == 63) behind = kBndWin;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (u < wave) before = max(before, wlast[u]);
    if (u > wave) behind = min(behind, wfirst[u]);
  }
  int nb = behind;
#pragma unroll
  for (int j = kBndOwn - 1; j >= 0; --j) {
    const int i = i0 + j;
    const int h = min(min(i - max(L[j], before) + 1, nb - i), cap);
    if (i >= kBndHalo && i < kBndHalo + kBndPos) hb[i - kBndHalo] = (uint8_t)h;
    if (brk & (1u << j)) nb = i;
  }
  __syncthreads();
  const int p = p0 + 8 * t;
  uint8_t* hp = hrow + (size_t)blockIdx.y * HW;
  if (p + 8 <= HW && ((uintptr_t)(hp + p) & 7) == 0) {
    *(u32x2*)(hp + p) = *(const u32x2*)(hb + 8 * t);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (p + k < HW) hp[p + k] = hb[8 * t + k];
  }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void boundary_col_kernel(const T* map, const uint8_t* hrow, uint8_t* dist, T* band, int H,
                                                           int W, int cap, int d) {
  constexpr int TX = kBndCols / V, TY = 256 / TX;   // threads along a tile row, rows a round
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
  const int x = blockIdx.x * kBndCols + tx * V;
  if (x >= W) return;                               // V == 4 only with W % 4 == 0: x < W covers x + 3
  const size_t img = (size_t)blockIdx.z * H * W;
#pragma unroll
  for (int r = 0; r < kBndRows / TY; ++r) {
    const int y = blockIdx.y * kBndRows + r * TY + ty;
    if (y >= H) return;
    const size_t o = img + (size_t)y * W + x;
    int v[V], best[V];
    bnd_load<T, V>(map + o, v);
    bnd_load<uint8_t, V>(hrow + o, best);
    const int edge = min(min(y + 1, H - y), cap);
    int far = 0;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      best[k] = v[k] ? min(best[k], edge) : 0;
      far = max(far, best[k]);
    }
    // dy < far <= min(y + 1, H - y): rows y - dy and y + dy exist.  A pixel with best <= dy takes nothing from this round:
    // both candidates are >= dy
    for (int dy = 1; dy < far; ++dy) {
      const size_t s = (size_t)dy * W;
      int mu[V], hu[V], md[V], hd[V];
      bnd_load<T, V>(map + o - s, mu);
      bnd_load<uint8_t, V>(hrow + o - s, hu);
      bnd_load<T, V>(map + o + s, md);
      bnd_load<uint8_t, V>(hrow + o + s, hd);
      far = 0;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const int cu = mu[k] == v[k] ? max(dy, hu[k]) : dy, cd = md[k] == v[k] ? max(dy, hd[k]) : dy;
        best[k] = min(best[k], min(cu, cd));
        far = max(far, best[k]);
      }
    }
    bnd_store<uint8_t, V>(dist + o, best);
    if (band) {
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] = best[k] <= d ? v[k] : 0;   // best == 0 only where v == 0
      bnd_store<T, V>(band + o, v);
    }
  }
}

// V neighbouring squared distances -> uint16
template <int V> __device__ __forceinline__ void bnd_store16(uint16_t* p, const int (&o)[V]) {
  if constexpr (V == 1) {
    p[0] = (uint16_t)o[0];
  } else {
    u32x2 w;
    w[0] = (uint32_t)o[0] | ((uint32_t)o[1] << 16), w[1] = (uint32_t)o[2] | ((uint32_t)o[3] << 16);
    *(u32x2*)p = w;
  }
}

// One piece of the peaks reduction goes out: the row only grows, so a key that a relaxed load already finds there, or a
// larger one, needs no atomic.
__device__ __forceinline__ void bnd_peak_out(unsigned long long* row, unsigned long long key) {
  if (__hip_atomic_load(row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(row, key);
}

// The peaks of one round of a wave: every lane holds V pixels side by side, id[k] in 1..pcap or 0 (not counted, inactive
// lanes included) and key[k].  A thread folds its runs of equal id into the run's last pixel; the run at a thread's end
// (its tail) goes on in the next lane when that lane starts with the same id, through all of that lane when it holds one
// id only.  A wave64 segmented max-scan over the tails folds every such chain, the chain's last lane sends it out, and the
// runs that end inside a thread go out by themselves.  All 64 lanes must arrive.
template <int V>
__device__ __forceinline__ void bnd_peaks_wave(unsigned long long* rows, const int (&idv)[V], unsigned long long (&key)[V]) {
  const int lane = threadIdx.x & 63;
  bool uniform = true;
#pragma unroll
  for (int k = 1; k < V; ++k) {
    if (idv[k] == idv[k - 1]) key[k] = max(key[k], key[k - 1]);
    else uniform = false;
  }
  int lead = 0;                                       // the last pixel of the thread's first run
#pragma unroll
  for (int k = V - 1; k > 0; --k)
    if (idv[k] != idv[k - 1]) lead = k - 1;
  if (uniform) lead = V - 1;
  const int tid = idv[V - 1];
  unsigned long long tkey = key[V - 1];
  // a first run that is not the whole thread joins the tail of the lane before it
  int lid = idv[0];
  unsigned long long lkey = key[0];
#pragma unroll
  for (int k = 1; k < V; ++k)
    if (k == lead) lkey = key[k];
  const int nlid = __shfl_down(lid, 1, 64), nuni = __shfl_down((int)uniform, 1, 64);
  const unsigned long long nlkey = __shfl_down(lkey, 1, 64);
  const int ptid = __shfl_up(tid, 1, 64);
  const bool absorbed = !uniform && lane > 0 && ptid == lid;          // my first run went into the lane before
  if (lane < 63 && !nuni && nlid == tid) tkey = max(tkey, nlkey);
  const bool joins = uniform && lane > 0 && ptid == tid;              // my tail goes on from the lane before
  int start = joins ? 0 : lane;                                       // the lane where my chain starts: a max-scan
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int s = __shfl_up(start, o, 64);
    if (lane >= o) start = max(start, s);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long other = __shfl_up(tkey, o, 64);
    if (lane - o >= start) tkey = max(tkey, other);
  }
  const int njoins = __shfl_down((int)joins, 1, 64);
  if (tid && (lane == 63 || !njoins)) bnd_peak_out(rows + (tid - 1), tkey);
  if constexpr (V > 1) {
#pragma unroll
    for (int k = 0; k < V - 1; ++k)
      if (idv[k] != idv[k + 1] && idv[k] && !(absorbed && k == lead)) bnd_peak_out(rows + (idv[k] - 1), key[k]);
  }
}

// The Euclidean column pass: boundary_col_kernel's tile and threads, the squared walk.  best starts at min(h, y + 1, H - y,
// cap)^2; round dy offers dy^2 + h(y +- dy, x)^2 where the column still holds v and dy^2 where it does not, and a pixel
// whose best is <= dy^2 takes nothing from it or any later round.  dy^2 < far <= min(y + 1, H - y, cap)^2: the rows exist
// and the walk ends after at most cap - 1 = dmax steps; dy^2 + h^2 <= 254^2 + 255^2.  P: the peaks of an id map, reduced
// per wave and round; no thread leaves before the last round then.
template <typename T, int V, bool P>
__global__ __launch_bounds__(256) void boundary_col2_kernel(const T* map, const uint8_t* hrow, uint16_t* dist, T* band,
                                                            unsigned long long* peaks, int H, int W, int cap, int d2,
                                                            int pcap) {
  constexpr int TX = kBndCols / V, TY = 256 / TX;
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
  const int x = blockIdx.x * kBndCols + tx * V;
  if (!P && x >= W) return;
  const size_t img = (size_t)blockIdx.z * H * W;
#pragma unroll
  for (int r = 0; r < kBndRows / TY; ++r) {
    const int y = blockIdx.y * kBndRows + r * TY + ty;
    if (!P && y >= H) return;
    const bool in = x < W && y < H;
    const size_t o = img + (size_t)(in ? y : 0) * W + (in ? x : 0);
    int v[V], best[V];
    if (in) {
      bnd_load<T, V>(map + o, v);
      bnd_load<uint8_t, V>(hrow + o, best);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] = best[k] = 0;
    }
    const int edge = min(min(y + 1, H - y), cap);
    int far = 0;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int b = min(best[k], edge);
      best[k] = v[k] ? b * b : 0;
      far = max(far, best[k]);
    }
    for (int dy = 1; dy * dy < far; ++dy) {
      const size_t s = (size_t)dy * W;
      int mu[V], hu[V], md[V], hd[V];
      bnd_load<T, V>(map + o - s, mu);
      bnd_load<uint8_t, V>(hrow + o - s, hu);
      bnd_load<T, V>(map + o + s, md);
      bnd_load<uint8_t, V>(hrow + o + s, hd);
      const int dd = dy * dy;
      far = 0;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const int cu = mu[k] == v[k] ? dd + hu[k] * hu[k] : dd, cd = md[k] == v[k] ? dd + hd[k] * hd[k] : dd;
        best[k] = min(best[k], min(cu, cd));
        far = max(far, best[k]);
      }
    }
    if (in) {
      bnd_store16<V>(dist + o, best);
      if (band) {
        int w[V];
#pragma unroll
        for (int k = 0; k < V; ++k) w[k] = best[k] <= d2 ? v[k] : 0;   // best == 0 only where v == 0
        bnd_store<T, V>(band + o, w);
      }
    }
    if constexpr (P) {
      int idv[V];
      unsigned long long key[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        idv[k] = (unsigned)(v[k] - 1) < (unsigned)pcap ? v[k] : 0;     // v == 0 outside the image
        key[k] = ((unsigned long long)best[k] << 32) | (0xFFFFFFFFu - (unsigned)(y * W + x + k));
      }
      bnd_peaks_wave<V>(peaks + (size_t)blockIdx.z * pcap, idv, key);
    }
  }
}

// ---- the nearest seed inside the object (version 125) ----
// The workspace of the seeded call: lab int32 [B * H * W] (the seed value the row pass found, 0 for none), rounded up to 16
// bytes, then h uint8 [B * H * W] (the distance along the row to it, 0..dmax, dmax + 1 for none).
inline size_t bnd_seed_lab_bytes(size_t n) { return (n * 4 + 15) & ~(size_t)15; }

// The row pass: boundary_row_kernel's window, breaks and scans, plus the same two scans over the positions that hold a
// seed.  For a position i of the block: the last seed at or before i counts when no break lies behind it (last seed >= last
// break), the next seed behind i when it lies before the next break -- both inside i's run of equal value.  The nearer one
// wins, the smaller seed value among two equally near; h = its distance, dmax + 1 (cap) when there is none within dmax.
// The halo of kBndHalo > dmax positions a side makes both final.  Seeds on background are found like any other and never
// read: the column pass looks at rows of its own non-zero value only.
__global__ __launch_bounds__(256) void seeds_row_kernel(const int32_t* map, const int32_t* seeds, int32_t* lab, uint8_t* hrow,
                                                        int HW, int W, int cap) {
  __shared__ __attribute__((aligned(16))) int val[kBndWin];
  __shared__ __attribute__((aligned(16))) int sd[kBndWin];
  __shared__ __attribute__((aligned(8))) uint8_t hb[kBndPos];
  __shared__ int wlast[4], wfirst[4], wslast[4], wsfirst[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int p0 = blockIdx.x * kBndPos, w0 = p0 - kBndHalo;
  const int32_t* mp = map + (size_t)blockIdx.y * HW;
  const int32_t* sp = seeds + (size_t)blockIdx.y * HW;
#pragma unroll
  for (int r = 0; r < (kBndWin / 4 + 255) / 256; ++r) {
    const int c = r * 256 + t;
    if (c < kBndWin / 4) {
      const int q = w0 + 4 * c;
      i32x4 w, z;
      if (q >= 0 && q + 4 <= HW && (((uintptr_t)(mp + q) | (uintptr_t)(sp + q)) & 15) == 0) {
        w = *(const i32x4*)(mp + q);
        z = *(const i32x4*)(sp + q);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool in = q + k >= 0 && q + k < HW;
          w[k] = in ? mp[q + k] : 0;
          z[k] = in ? sp[q + k] : 0;
        }
      }
      *(i32x4*)(val + 4 * c) = w;
      *(i32x4*)(sd + 4 * c) = z;
    }
  }
  __syncthreads();
  const int i0 = kBndOwn * t, q0 = w0 + i0;
  int v[kBndOwn + 1];
  v[0] = t ? val[i0 - 1] : 0;
#pragma unroll
  for (int j = 0; j < kBndOwn; ++j) v[j + 1] = val[i0 + j];
  int x = q0 >= 0 ? q0 % W : 0;
  int last = -1, first = kBndWin, slast = -1, sfirst = kBndWin, L[kBndOwn], S[kBndOwn];
  unsigned brk = 0u, sbit = 0u;
#pragma unroll
  for (int j = 0; j < kBndOwn; ++j) {
    const int q = q0 + j;
    if (q < 0 || q >= HW || x == 0 || v[j + 1] != v[j] || i0 + j == 0) {
      brk |= 1u << j;
      last = i0 + j;
      if (first == kBndWin) first = i0 + j;
    }
    if (sd[i0 + j] != 0) {                 // 0 outside the image
      sbit |= 1u << j;
      slast = i0 + j;
      if (sfirst == kBndWin) sfirst = i0 + j;
    }
    L[j] = last;
    S[j] = slast;
    if (q >= 0 && ++x == W) x = 0;
  }
  int ls = last, fs = first, lss = slast, fss = sfirst;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int a = __shfl_up(ls, o, 64), c = __shfl_down(fs, o, 64);
    const int sa = __shfl_up(lss, o, 64), sc = __shfl_down(fss, o, 64);
    if (lane >= o) ls = max(ls, a), lss = max(lss, sa);
    if (lane + o < 64) fs = min(fs, c), fss = min(fss, sc);
  }
  if (lane == 63) wlast[wave] = ls, wslast[wave] = lss;
  if (lane == 0) wfirst[wave] = fs, wsfirst[wave] = fss;
  int before = __shfl_up(ls, 1, 64), behind = __shfl_down(fs, 1, 64);
  int sbefore = __shfl_up(lss, 1, 64), sbehind = __shfl_down(fss, 1, 64);
  if (lane == 0) before = sbefore = -1;
  if (lane == 63) behind = sbehind = kBndWin;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (u < wave) before = max(before, wlast[u]), sbefore = max(sbefore, wslast[u]);
    if (u > wave) behind = min(behind, wfirst[u]), sbehind = min(sbehind, wsfirst[u]);
  }
  int nb = behind, ns = sbehind, out[kBndOwn];
#pragma unroll
  for (int j = kBndOwn - 1; j >= 0; --j) {
    const int i = i0 + j;
    const int lb = max(L[j], before), lsd = max(S[j], sbefore);
    const int dl = lsd >= lb ? i - lsd : cap, dr = ns < nb ? ns - i : cap;   // lb >= 0: the window's first position is a break
    int h = min(min(dl, dr), cap), lv = 0;
    if (h < cap) {
      if (dl < dr) lv = sd[lsd];
      else if (dr < dl) lv = sd[ns];
      else lv = min(sd[lsd], sd[ns]);
    }
    out[j] = lv;
    if (i >= kBndHalo && i < kBndHalo + kBndPos) hb[i - kBndHalo] = (uint8_t)h;
    if (brk & (1u << j)) nb = i;
    if (sbit & (1u << j)) ns = i;
  }
  __syncthreads();                         // every lookup of sd is done: it now carries the labels out
#pragma unroll
  for (int j = 0; j < kBndOwn; ++j) sd[i0 + j] = out[j];
  __syncthreads();
  const int p = p0 + 8 * t;
  uint8_t* hp = hrow + (size_t)blockIdx.y * HW;
  int32_t* lp = lab + (size_t)blockIdx.y * HW;
  if (p + 8 <= HW && ((uintptr_t)(hp + p) & 7) == 0) {
    *(u32x2*)(hp + p) = *(const u32x2*)(hb + 8 * t);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (p + k < HW) hp[p + k] = hb[8 * t + k];
  }
  if (p + 8 <= HW && ((uintptr_t)(lp + p) & 15) == 0) {
    *(i32x4*)(lp + p) = *(const i32x4*)(sd + kBndHalo + 8 * t);
    *(i32x4*)(lp + p + 4) = *(const i32x4*)(sd + kBndHalo + 8 * t + 4);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (p + k < HW) lp[p + k] = sd[kBndHalo + 8 * t + k];
  }
}

// The column pass: boundary_col2_kernel's tile and threads.  A pixel of value v starts from its own row's (h^2, label) and
// walks dy = 1, 2, ... up and down, each direction while the rows exist and the column holds v; row y +- dy offers (dy^2 +
// h^2, label) when h <= R and the sum is <= R^2.  The smaller (distance, label) pair wins.  A later row can still tie the
// best distance with a smaller label (only with h = 0 there), so the walk goes on while dy^2 <= the best so far, not <, and
// at most R steps; dy^2 + h^2 <= 2 * 254^2.  Labels come from the workspace only, never from `nearest`, which this launch
// writes: a repeat in place is safe.  LATER (passes 2..): a pixel whose own row distance is 0 holds a value already and keeps
// it and its dist -- its label is rewritten with itself, its old dist is read back and stored, by the one thread that owns
// the pixel -- and its walk is skipped.
template <int V, bool LATER>
__global__ __launch_bounds__(256) void seeds_col_kernel(const int32_t* map, const int32_t* lab, const uint8_t* hrow,
                                                        int32_t* nearest, uint16_t* dist, int H, int W, int R) {
  constexpr int TX = kBndCols / V, TY = 256 / TX;
  constexpr int kNone = 0x7fffffff;
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
  const int x = blockIdx.x * kBndCols + tx * V;
  if (x >= W) return;                               // V == 4 only with W % 4 == 0: x < W covers x + 3
  const size_t img = (size_t)blockIdx.z * H * W;
  const int R2 = R * R, none = (R + 1) * (R + 1);
#pragma unroll
  for (int r = 0; r < kBndRows / TY; ++r) {
    const int y = blockIdx.y * kBndRows + r * TY + ty;
    if (y >= H) return;
    const size_t o = img + (size_t)y * W + x;
    int v[V], h0[V], best[V], bl[V], keep[V];
    bool up[V], dn[V];
    bnd_load<int32_t, V>(map + o, v);
    bnd_load<uint8_t, V>(hrow + o, h0);
    bnd_load<int32_t, V>(lab + o, bl);
    if constexpr (LATER) {
      if constexpr (V == 4) {
        const u32x2 w = *(const u32x2*)(dist + o);
#pragma unroll
        for (int k = 0; k < 4; ++k) keep[k] = (int)((w[k >> 1] >> (16 * (k & 1))) & 65535u);
      } else {
        keep[0] = dist[o];
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const bool walk = v[k] != 0 && !(LATER && h0[k] == 0);
      best[k] = h0[k] <= R ? h0[k] * h0[k] : kNone;
      if (best[k] == kNone) bl[k] = 0;
      up[k] = dn[k] = walk;
    }
    for (int dy = 1; dy <= R; ++dy) {
      const int dd = dy * dy;
      const bool rowu = y - dy >= 0, rowd = y + dy < H;
      bool gu = false, gd = false;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        up[k] = up[k] && rowu && dd <= best[k];
        dn[k] = dn[k] && rowd && dd <= best[k];
        gu = gu || up[k];
        gd = gd || dn[k];
      }
      if (!gu && !gd) break;
      const size_t s = (size_t)dy * W;
      if (gu) {
        int m[V], hh[V], ll[V];
        bnd_load<int32_t, V>(map + o - s, m);
        bnd_load<uint8_t, V>(hrow + o - s, hh);
        bnd_load<int32_t, V>(lab + o - s, ll);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          up[k] = up[k] && m[k] == v[k];
          const int c = dd + hh[k] * hh[k];
          if (up[k] && hh[k] <= R && c <= R2 && (c < best[k] || (c == best[k] && ll[k] < bl[k]))) best[k] = c, bl[k] = ll[k];
        }
      }
      if (gd) {
        int m[V], hh[V], ll[V];
        bnd_load<int32_t, V>(map + o + s, m);
        bnd_load<uint8_t, V>(hrow + o + s, hh);
        bnd_load<int32_t, V>(lab + o + s, ll);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          dn[k] = dn[k] && m[k] == v[k];
          const int c = dd + hh[k] * hh[k];
          if (dn[k] && hh[k] <= R && c <= R2 && (c < best[k] || (c == best[k] && ll[k] < bl[k]))) best[k] = c, bl[k] = ll[k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (v[k] == 0) best[k] = 0, bl[k] = 0;
      else if (LATER && h0[k] == 0) best[k] = keep[k];
      else if (best[k] == kNone) best[k] = none;
    }
    bnd_store<int32_t, V>(nearest + o, bl);
    bnd_store16<V>(dist + o, best);
  }
}

__global__ __launch_bounds__(256) void boundary_zero_kernel(unsigned long long* words, int n) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) words[e] = 0ull;
}

// DT: the dist maps' element, uint8 distances (a pixel lies in the band when 1 <= dist <= lim = d) or uint16 squared
// distances (lim = d * d)
template <typename DT>
__global__ __launch_bounds__(256) void boundary_counts_kernel(const uint8_t* pred, const DT* pdist, const uint8_t* gt,
                                                              const DT* gdist, unsigned long long* counts, int HW, int lim,
                                                              int nlabels) {
  __shared__ unsigned hist[3 * 256];   // [inter | pred | gt][label byte]
  const int t = threadIdx.x;
  for (int i = t; i < 3 * 256; i += 256) hist[i] = 0u;
  __syncthreads();
  const size_t base = (size_t)blockIdx.y * HW;
  pred += base, pdist += base, gt += base, gdist += base;
  const seg_gt_byte bin = {nlabels};
  unsigned none = 0u;                  // kept pixels in neither band: bin 0 of all three
  auto count = [&](int p, int pd, int g, int gd) {
    if (bin(g) < 0) return;
    const int l = (unsigned)(pd - 1) < (unsigned)lim ? p : 0, gg = (unsigned)(gd - 1) < (unsigned)lim ? g : 0;
    if ((l | gg) == 0) {
      ++none;
      return;
    }
    atomicAdd(&hist[256 + l], 1u);
    atomicAdd(&hist[512 + gg], 1u);
    if (l == gg) atomicAdd(&hist[l], 1u);
  };
  const int p0 = blockIdx.x * kBndCountPix;
  if ((HW & 3) == 0 && (((uintptr_t)pred | (uintptr_t)gt) & 3) == 0 &&
      (((uintptr_t)pdist | (uintptr_t)gdist) & (4 * sizeof(DT) - 1)) == 0) {
#pragma unroll
    for (int r = 0; r < kBndCountPix / 1024; ++r) {
      const int q = p0 + 4 * (r * 256 + t);
      if (q < HW) {
        const uint32_t wp = *(const uint32_t*)(pred + q), wg = *(const uint32_t*)(gt + q);
        if constexpr (sizeof(DT) == 1) {
          const uint32_t wpd = *(const uint32_t*)(pdist + q), wgd = *(const uint32_t*)(gdist + q);
#pragma unroll
          for (int k = 0; k < 4; ++k)
            count((wp >> (8 * k)) & 255u, (wpd >> (8 * k)) & 255u, (wg >> (8 * k)) & 255u, (wgd >> (8 * k)) & 255u);
        } else {
          const u32x2 wpd = *(const u32x2*)(pdist + q), wgd = *(const u32x2*)(gdist + q);
#pragma unroll
          for (int k = 0; k < 4; ++k)
            count((wp >> (8 * k)) & 255u, (wpd[k >> 1] >> (16 * (k & 1))) & 65535u, (wg >> (8 * k)) & 255u,
                  (wgd[k >> 1] >> (16 * (k & 1))) & 65535u);
        }
      }
    }
  } else {
#pragma unroll 4
    for (int r = 0; r < kBndCountPix / 256; ++r) {
      const int q = p0 + r * 256 + t;
      if (q < HW) count(pred[q], pdist[q], gt[q], gdist[q]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) none += (unsigned)__shfl_xor((int)none, o, 64);
  if ((t & 63) == 0 && none) {
    atomicAdd(&hist[0], none);
    atomicAdd(&hist[256], none);
    atomicAdd(&hist[512], none);
  }
  __syncthreads();
  const int NB = nlabels + 1;
  seg_flush_counts(hist, counts + (size_t)blockIdx.y * 2 * NB, NB);
}

template <typename T, int V, bool P>
static void boundary_launch_col2(hipStream_t st, const dfw_seg_boundary_args* a, dim3 grid) {
  hipLaunchKernelGGL((boundary_col2_kernel<T, V, P>), grid, dim3(256), 0, st, (const T*)a->map, (const uint8_t*)a->ws,
                     (uint16_t*)a->dist, (T*)a->band, (unsigned long long*)a->peaks, a->H, a->W, a->dmax + 1,
                     a->band ? a->d * a->d : 0, a->cap);   // d is looked at with a band only
}

template <typename T>
static void boundary_launch(hipStream_t st, const dfw_seg_boundary_args* a, bool vec) {
  const int HW = a->H * a->W, cap = a->dmax + 1;
  hipLaunchKernelGGL(boundary_row_kernel<T>, dim3((HW + kBndPos - 1) / kBndPos, a->B), dim3(256), 0, st, (const T*)a->map,
                     (uint8_t*)a->ws, HW, a->W, cap);
  const dim3 grid((a->W + kBndCols - 1) / kBndCols, (a->H + kBndRows - 1) / kBndRows, a->B);
  if (a->metric == 1) {
    if constexpr (sizeof(T) == 4) {                   // peaks come with an id map only
      if (a->peaks) {
        if (vec) boundary_launch_col2<T, 4, true>(st, a, grid);
        else boundary_launch_col2<T, 1, true>(st, a, grid);
        return;
      }
    }
    if (vec) boundary_launch_col2<T, 4, false>(st, a, grid);
    else boundary_launch_col2<T, 1, false>(st, a, grid);
  } else if (vec)
    hipLaunchKernelGGL((boundary_col_kernel<T, 4>), grid, dim3(256), 0, st, (const T*)a->map, (const uint8_t*)a->ws,
                       (uint8_t*)a->dist, (T*)a->band, a->H, a->W, cap, a->d);
  else
    hipLaunchKernelGGL((boundary_col_kernel<T, 1>), grid, dim3(256), 0, st, (const T*)a->map, (const uint8_t*)a->ws,
                       (uint8_t*)a->dist, (T*)a->band, a->H, a->W, cap, a->d);
}

// The launches of the nearest-seed stage of dfw_seg_components (seeds non-null), which has validated everything: 2 * passes,
// pass k > 1 with seeds := nearest in place.
int seg_nearest_launch(const dfw_seg_components_args* a, void* stream) {
  const int HW = a->H * a->W;
  const size_t n = (size_t)a->B * HW;
  hipStream_t st = (hipStream_t)stream;
  // four pixels a thread: whole words of map, nearest, dist and both planes of the workspace, in every row of every image
  const bool vec = a->W % 4 == 0 && (((uintptr_t)a->map | (uintptr_t)a->nearest | (uintptr_t)a->ws) & 15) == 0 &&
                   ((uintptr_t)a->dist & 7) == 0;
  int32_t* lab = (int32_t*)a->ws;
  uint8_t* h = (uint8_t*)a->ws + bnd_seed_lab_bytes(n);
  const dim3 rgrid((HW + kBndPos - 1) / kBndPos, a->B);
  const dim3 grid((a->W + kBndCols - 1) / kBndCols, (a->H + kBndRows - 1) / kBndRows, a->B);
  uint16_t* dist = (uint16_t*)a->dist;
  for (int k = 0; k < a->passes; ++k) {
    hipLaunchKernelGGL(seeds_row_kernel, rgrid, dim3(256), 0, st, a->map, k ? (const int32_t*)a->nearest : a->seeds, lab, h, HW,
                       a->W, a->reach + 1);
    DFW_CHECK_LAUNCH();
    if (k == 0) {
      if (vec) hipLaunchKernelGGL((seeds_col_kernel<4, false>), grid, dim3(256), 0, st, a->map, lab, h, a->nearest, dist, a->H, a->W, a->reach);
      else hipLaunchKernelGGL((seeds_col_kernel<1, false>), grid, dim3(256), 0, st, a->map, lab, h, a->nearest, dist, a->H, a->W, a->reach);
    } else {
      if (vec) hipLaunchKernelGGL((seeds_col_kernel<4, true>), grid, dim3(256), 0, st, a->map, lab, h, a->nearest, dist, a->H, a->W, a->reach);
      else hipLaunchKernelGGL((seeds_col_kernel<1, true>), grid, dim3(256), 0, st, a->map, lab, h, a->nearest, dist, a->H, a->W, a->reach);
    }
    DFW_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace dfw

using namespace dfw;

extern "C" size_t dfw_seg_boundary_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t elem) {
  if ((elem != 1 && elem != 4) || seg_map_size_error(B, H, W)) return 0;
  return ((size_t)B * H * W + 15) & ~(size_t)15;   // h, one byte a pixel
}

extern "C" size_t dfw_seg_nearest_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  if (seg_map_size_error(B, H, W)) return 0;
  const size_t n = (size_t)B * H * W;
  return bnd_seed_lab_bytes(n) + ((n + 15) & ~(size_t)15);   // lab, four bytes a pixel, and h, one
}

extern "C" int dfw_seg_boundary_block(int32_t* rows, int32_t* cols, int32_t* positions) {
  if (!rows || !cols || !positions) return DFW_EINVAL;
  *rows = kBndRows, *cols = kBndCols, *positions = kBndPos;
  return 0;
}

extern "C" int dfw_seg_boundary(const dfw_seg_boundary_args* a, dfw_stream_t stream) {
  if (!a || !a->map || !a->dist || !a->ws) return DFW_EINVAL;
  if (a->elem != 1 && a->elem != 4) return DFW_EINVAL;
  if (a->dmax < 1 || a->dmax > 254) return DFW_EINVAL;
  if (a->band && (a->d < 1 || a->d > a->dmax)) return DFW_EINVAL;
  if (a->metric != 0 && a->metric != 1) return DFW_EINVAL;
  if (a->peaks && (a->metric == 0 || a->elem != 4 || a->cap < 1)) return DFW_EINVAL;
  if (int e = seg_map_size_error(a->B, a->H, a->W)) return e;
  if (a->peaks && (long long)a->B * a->cap > 0x7fffffffll) return DFW_ERANGE;
  const size_t wsb = dfw_seg_boundary_workspace_bytes(a->B, a->H, a->W, a->elem);
  if (a->ws_bytes < wsb) return DFW_EWORKSPACE;
  const size_t n = (size_t)a->B * a->H * a->W, el = (size_t)a->elem, de = a->metric == 1 ? 2 : 1;
  const size_t rows = a->peaks ? (size_t)a->B * a->cap : 0;
  const seg_buf bufs[] = {seg_in(a->map, n * el, el), seg_out(a->dist, n * de, de), seg_out(a->band, n * el, el),
                          seg_out(a->ws, wsb, 4), seg_out(a->peaks, rows * 8, 8)};
  if (int e = seg_check_buffers(bufs)) return e;
  hipStream_t st = (hipStream_t)stream;
  if (a->peaks) {
    hipLaunchKernelGGL(boundary_zero_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st,
                       (unsigned long long*)a->peaks, (int)rows);
    DFW_CHECK_LAUNCH();
  }
  // four pixels a thread in the column pass: whole words of every map, in every row of every image
  const uintptr_t al = 4 * el - 1;
  const bool vec = a->W % 4 == 0 && (((uintptr_t)a->map | (uintptr_t)a->band) & al) == 0 && ((uintptr_t)a->dist & (4 * de - 1)) == 0;
  if (a->elem == 1) boundary_launch<uint8_t>(st, a, vec);
  else boundary_launch<int32_t>(st, a, vec);
  DFW_CHECK_LAUNCH();
  return 0;
}

extern "C" int dfw_seg_boundary_counts(const dfw_seg_boundary_counts_args* a, dfw_stream_t stream) {
  if (!a || !a->pred || !a->pdist || !a->gt || !a->gdist || !a->counts) return DFW_EINVAL;
  if (a->d < 1 || a->d > 254) return DFW_EINVAL;
  if (a->nlabels < 1 || a->nlabels > 254) return DFW_EINVAL;
  if (a->dist_elem < 0 || a->dist_elem > 2) return DFW_EINVAL;
  if (int e = seg_map_size_error(a->B, a->H, a->W)) return e;
  const size_t n = (size_t)a->B * a->H * a->W, cb = (size_t)a->B * 2 * (a->nlabels + 1) * 8, de = a->dist_elem == 2 ? 2 : 1;
  const seg_buf bufs[] = {seg_in(a->pred, n), seg_in(a->pdist, n * de, de), seg_in(a->gt, n), seg_in(a->gdist, n * de, de),
                          seg_out(a->counts, cb, 8)};
  if (int e = seg_check_buffers(bufs)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int HW = a->H * a->W, words = a->B * 2 * (a->nlabels + 1);
  hipLaunchKernelGGL(boundary_zero_kernel, dim3((words + 255) / 256), dim3(256), 0, st, (unsigned long long*)a->counts, words);
  DFW_CHECK_LAUNCH();
  const dim3 grid((HW + kBndCountPix - 1) / kBndCountPix, a->B);
  if (de == 2)
    hipLaunchKernelGGL(boundary_counts_kernel<uint16_t>, grid, dim3(256), 0, st, a->pred, (const uint16_t*)a->pdist, a->gt,
                       (const uint16_t*)a->gdist, (unsigned long long*)a->counts, HW, a->d * a->d, a->nlabels);
  else
    hipLaunchKernelGGL(boundary_counts_kernel<uint8_t>, grid, dim3(256), 0, st, a->pred, (const uint8_t*)a->pdist, a->gt,
                       (const uint8_t*)a->gdist, (unsigned long long*)a->counts, HW, a->d, a->nlabels);
  DFW_CHECK_LAUNCH();
  return 0;
}
