// Outlines of labelled objects (objects.object_contours): ids int32 [B][H][W] -> per image the rings of corner points of
// every object 1..cap, a ring table grouped by id, an offset table over the ids, and n = (edges found, corners, rings,
// complete).  All integers: the result depends on no order of execution.
//
// v(y, x) is the id when 1 <= id <= cap and 0 otherwise; outside the image v is 0.  Pixel (x, y) is the unit square with
// the corners (x, y) and (x + 1, y + 1); vertices are the lattice points 0 <= X <= W, 0 <= Y <= H.
//
// An EDGE is a side of a pixel p with v(p) != 0 whose pixel across that side has a different v.  Edges are directed
// clockwise on screen (y down), the object on the right: side 0 is the top, heading east; 1 the right, heading south; 2 the
// bottom, heading west; 3 the left, heading north.  Its key is 4 * (y * W + x) + side.  Between two different objects both
// pixels own an edge.
//
// The SUCCESSOR of edge e of pixel p, side s, id i depends on `connectivity`, which must be the one the ids were made
// with.  A is the pixel ahead of p in the heading, L the pixel to the left of A relative to the heading.  A left turn goes
// to side (s + 3) % 4 of L, straight to side s of A, a right turn to side (s + 1) % 4 of p.
//   connectivity 8: left if v(L) == i, else straight if v(A) == i, else right
//   connectivity 4: right if v(A) != i, else left if v(L) == i, else straight
// This map is a bijection on the edges (also for ids that do not match the connectivity), so the edges split into cycles.
//
// A RING is a cycle; it belongs to one id.  Its leader is its smallest key, the rank of an edge the number of successor
// steps from the leader, its area the sum of X over its south edges minus the sum of X over its north edges, X the edge's
// column (the integral of x dy: positive for an outer ring, negative for a hole ring).  The CORNERS of a ring are the start
// vertices of the edges whose predecessor has another heading, in ascending rank; the leader's own start need not be one (a
// hole two pixels wide).  With connectivity 8 a ring may visit a vertex twice, where two pixels touch diagonally; it never
// crosses itself.
//
// rings [.., :rings] holds (id, first, count, area) sorted by id ascending and leader ascending within an id, first being
// the row of the ring's first corner in verts; object k's rings are rows ring_off[k-1] .. ring_off[k]; verts holds (X, Y),
// the corners of a ring contiguous and in rank order, the rings in the order of `rings`.  An image with more than max_edges
// edges is not complete: n = (found, 0, 0, 0), ring_off all zero, no row of rings or verts written -- a cut ring is not a
// ring.  Connectivity 8, cap = 1:
//   [[1,1,1,1],[1,0,0,1],[1,1,1,1]]  20 edges, rings (1, 0, 4, 12) with corners (0,0) (4,0) (4,3) (0,3) and (1, 4, 4, -2)
//                                    with corners (1,1) (1,2) (3,2) (3,1)
//   [[0,1,0],[1,0,1],[0,1,0]]        16 edges; the outer ring has 12 corners, starts at (1,0), area 5; the hole ring has
//                                    the corners (2,1) (1,1) (1,2) (2,2), area -1.  Under connectivity 4 with the ids 1..4
//                                    the same diamond gives four unit squares
//
// With E = max_edges, Q = E / 4 (a ring has at least 4 edges), R = ceil(log2 E) and passes = the bytes cap needs, the
// launches are a number fixed by the arguments, 14 + 2 R + 3 passes, with no host readback in between:
//
//   0   seg_zero_launch          ring_off (a library kernel, no memset node)
//   1   ct_count_kernel          the edges per block of kSegPix pixels: a pixel against its four neighbours, 16-byte loads
//                                where W is a multiple of 4 and the image 16-byte aligned, word loads otherwise
//   2   seg_scan_launch          the block sums in place; cnt = (min(found, E), found).  complete = found <= E, and every
//                                later kernel skips an image that is not (the counts the scans below read are then 0)
//   3   ct_emit_kernel           pre [HW], the edges before every pixel, and key [c] of every edge: c is monotone in the key
//   4   ct_link_kernel           per edge its id, its successor's index -- pre of the successor's pixel plus that pixel's
//                                lower sides -- and onto the successor whether it is a corner (a turn led to it)
//   5   ct_lead_kernel x R       pointer doubling on (jump, smallest index of the window), the window doubling a round,
//                                between two buffers in turn: 2^R >= E reaches every edge of the longest possible ring
//   6   ct_rank_init_kernel      cuts every cycle in front of its leader: (jump or -1, corner, area term, leader)
//   7   ct_rank_kernel x R       doubling again, corners and area summed to the cycle's end; at the leader they are the
//                                ring's.  The area wraps in 32 bits on the way (up to E * W); the ring's own, at most H * W
//                                in size, comes out exact
//   8   ct_ring_count_kernel     leaders per block of kCtEdge edges
//   9   seg_scan_launch          cnt[2..3] = rings
//   10  ct_ring_emit_kernel      (id, leader) of every ring, leaders ascending; each counts itself into ring_off[id - 1]
//                                (an integer atomic: a count, never a position)
//   11  seg_scan_launch          ring_off
//   12+ seg_sort                 stable by id, seg_rle's sort: hist, scan, seg_scatter_kernel<ct_pay> per key byte
//   ..  ct_corner_count_kernel   the corners of the rings in sorted order, 0 behind them
//   ..  seg_scan_launch          -> first, and the corners of the image
//   ..  ct_rows_kernel           rings' rows, every ring's first at its leader, and n
//   ..  ct_verts_kernel          every corner edge writes (X, Y) at first + (ring's corners - corners from it to the end)
//
// The workspace is, for all images, state [2][E] x 16 bytes | lead [2][E] x 8 | key, id, corner, succ [E] | cnt [4] |
// corners [2] | pre [HW] | blk | ring blk | ring key [2][Q], leader [2][Q], count [Q] | tab [256][chunks of Q]: 64 bytes per
// edge and 4 per pixel.  Every word is written before it is read (the caller initialises nothing).
//
// Termination: no thread waits for another thread or workgroup; every loop has a trip count fixed by the arguments, every
// cross-workgroup prefix is a scan in a launch of its own.  Any grid is correct at any residency.
#include "seg_args.h"
#include "seg_sort.h"

namespace dfw {

constexpr int kCtEdge = 2048;   // edges per block of the ring count, 8 per thread of 256

using i32x2 = int __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int ct_value(int id, int cap) { return (id >= 1 && id <= cap) ? id : 0; }

// v(y, x) of one image, 0 outside it
__device__ __forceinline__ int ct_at(const int32_t* a, int H, int W, int y, int x, int cap) {
  return ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? ct_value(a[(size_t)y * W + x], cap) : 0;
}

// The sides of pixel (y, x) that are edges, bit s = side s.
__device__ __forceinline__ int ct_sides(const int32_t* a, int H, int W, int y, int x, int cap) {
  const int c = ct_at(a, H, W, y, x, cap);
  if (c == 0) return 0;
  return (ct_at(a, H, W, y - 1, x, cap) != c) | (ct_at(a, H, W, y, x + 1, cap) != c) << 1 |
         (ct_at(a, H, W, y + 1, x, cap) != c) << 2 | (ct_at(a, H, W, y, x - 1, cap) != c) << 3;
}

// The sides of the eight pixels p0 .. p0 + 7 (positions y * W + x; 0 behind the image).  `vec`: W is a multiple of 4 and
// the image 16-byte aligned, so each group of four lies in one row and it, the row above and the row below load as one
// 16-byte word each.
__device__ __forceinline__ void ct_sides8(const int32_t* a, int H, int W, int cap, int p0, bool vec, int (&m)[8]) {
  const int HW = H * W;
  if (vec) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int q = p0 + 4 * g;
      if (q >= HW) {                       // HW is a multiple of 4 here: a group is inside or outside as a whole
#pragma unroll
        for (int j = 0; j < 4; ++j) m[4 * g + j] = 0;
        continue;
      }
      const int y = q / W, x = q - y * W;
      const i32x4 z = {0, 0, 0, 0};
      const i32x4 c = *(const i32x4*)(a + q);
      const i32x4 u = y > 0 ? *(const i32x4*)(a + q - W) : z;
      const i32x4 d = y + 1 < H ? *(const i32x4*)(a + q + W) : z;
      int row[6];
      row[0] = x > 0 ? ct_value(a[q - 1], cap) : 0;
      row[5] = x + 4 < W ? ct_value(a[q + 4], cap) : 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) row[1 + j] = ct_value(c[j], cap);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int v = row[1 + j];
        m[4 * g + j] = v == 0 ? 0
                              : (ct_value(u[j], cap) != v) | (row[2 + j] != v) << 1 | (ct_value(d[j], cap) != v) << 2 |
                                    (row[j] != v) << 3;
      }
    }
  } else {
    int y = p0 / W, x = p0 - y * W;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      m[j] = p0 + j < HW ? ct_sides(a, H, W, y, x, cap) : 0;
      if (++x == W) x = 0, ++y;
    }
  }
}

__device__ __forceinline__ bool ct_vec(const int32_t* a, int W) { return (W & 3) == 0 && ((uintptr_t)a & 15) == 0; }

__global__ __launch_bounds__(256) void ct_count_kernel(const int32_t* ids, int32_t* blk, int H, int W, int cap) {
  __shared__ int ws[4];
  const int32_t* a = ids + (size_t)blockIdx.y * H * W;
  int m[8];
  ct_sides8(a, H, W, cap, blockIdx.x * kSegPix + threadIdx.x * 8, ct_vec(a, W), m);
  int n = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) n += __popc(m[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) blk[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// cnt [B][4] = (min(found, E), found, rings, rings)
__device__ __forceinline__ int ct_found(const int32_t* cnt, int b, int E) {
  const int found = cnt[4 * b + 1];
  return found <= E ? found : 0;          // the edges the later kernels work on: none of an image that is not complete
}

__global__ __launch_bounds__(256) void ct_emit_kernel(const int32_t* ids, const int32_t* blk, const int32_t* cnt,
                                                      int32_t* pre, int32_t* key, int H, int W, int cap, int E) {
  __shared__ int wsum[4];
  const int b = blockIdx.y, HW = H * W, p0 = blockIdx.x * kSegPix + threadIdx.x * 8;
  if (ct_found(cnt, b, E) == 0) return;   // the whole workgroup
  const int32_t* a = ids + (size_t)b * HW;
  int m[8];
  ct_sides8(a, H, W, cap, p0, ct_vec(a, W), m);
  int n = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) n += __popc(m[j]);
  int total;
  int c = blk[(size_t)b * gridDim.x + blockIdx.x] + block_scan(n, wsum, &total);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (p0 + j >= HW) break;
    pre[(size_t)b * HW + p0 + j] = c;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (m[j] >> s & 1) {
        if (c < E) key[(size_t)b * E + c] = 4 * (p0 + j) + s;   // always: the image is complete
        ++c;
      }
  }
}

__global__ __launch_bounds__(256) void ct_link_kernel(const int32_t* ids, const int32_t* cnt, const int32_t* pre,
                                                      const int32_t* key, int32_t* eid, int32_t* succ, int32_t* corner,
                                                      i32x2* lead, int H, int W, int cap, int E, int conn) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x, found = ct_found(cnt, b, E);
  if (c >= found) return;
  const int HW = H * W;
  const int32_t* a = ids + (size_t)b * HW;
  const size_t r0 = (size_t)b * E;
  const int k = key[r0 + c], p = k >> 2, s = k & 3, y = p / W, x = p - y * W;
  const int i = ct_value(a[p], cap);
  const int dy = s == 1 ? 1 : s == 3 ? -1 : 0, dx = s == 0 ? 1 : s == 2 ? -1 : 0;
  const int ay = y + dy, ax = x + dx, ly = ay - dx, lx = ax + dy;   // ahead; left of ahead relative to the heading
  const bool sa = ct_at(a, H, W, ay, ax, cap) == i, sl = ct_at(a, H, W, ly, lx, cap) == i;
  const bool left = conn == 8 ? sl : sa && sl, straight = !left && sa;
  const int qy = left ? ly : straight ? ay : y, qx = left ? lx : straight ? ax : x;
  const int t = left ? (s + 3) & 3 : straight ? s : (s + 1) & 3;
  // the successor's pixel has v == i, so it lies inside the image
  int nx = pre[(size_t)b * HW + qy * W + qx] + __popc(ct_sides(a, H, W, qy, qx, cap) & ((1 << t) - 1));
  if ((unsigned)nx >= (unsigned)found) nx = c;   // never, by the bijection; an index stays inside the records all the same
  eid[r0 + c] = i;
  succ[r0 + c] = nx;
  corner[r0 + nx] = !straight;                   // every edge is the successor of exactly one
  lead[r0 + c] = i32x2{nx, c};                  // a window of one edge
}

// (jump, smallest index of the window) -> the same over twice the window
__global__ __launch_bounds__(256) void ct_lead_kernel(const i32x2* src, i32x2* dst, const int32_t* cnt, int E) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ct_found(cnt, b, E)) return;
  const size_t r0 = (size_t)b * E;
  const i32x2 u = src[r0 + c], w = src[r0 + u.x];
  dst[r0 + c] = i32x2{w.x, min(u.y, w.y)};
}

// state = (jump, or -1 at the last edge of the ring; corners from here to the end; area from here to the end; leader)
__global__ __launch_bounds__(256) void ct_rank_init_kernel(const i32x2* lead, const int32_t* key, const int32_t* succ,
                                                           const int32_t* corner, i32x4* state, const int32_t* cnt, int W,
                                                           int E) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ct_found(cnt, b, E)) return;
  const size_t r0 = (size_t)b * E;
  const int ld = lead[r0 + c].y, nx = succ[r0 + c], k = key[r0 + c], s = k & 3, x = (k >> 2) % W;
  state[r0 + c] = i32x4{nx == ld ? -1 : nx, corner[r0 + c], s == 1 ? x + 1 : s == 3 ? -x : 0, ld};
}

__global__ __launch_bounds__(256) void ct_rank_kernel(const i32x4* src, i32x4* dst, const int32_t* cnt, int E) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ct_found(cnt, b, E)) return;
  const size_t r0 = (size_t)b * E;
  i32x4 u = src[r0 + c];
  if (u.x >= 0) {
    const i32x4 w = src[r0 + u.x];
    u.x = w.x;
    u.y += w.y;
    u.z = (int)((unsigned)u.z + (unsigned)w.z);   // wraps on the way, see the header
  }
  dst[r0 + c] = u;
}

__global__ __launch_bounds__(256) void ct_ring_count_kernel(const i32x4* state, const int32_t* cnt, int32_t* rblk, int E) {
  __shared__ int ws[4];
  const int b = blockIdx.y, found = ct_found(cnt, b, E);
  int n = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = blockIdx.x * kCtEdge + threadIdx.x * 8 + j;
    n += c < found && state[(size_t)b * E + c].w == c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) rblk[(size_t)b * gridDim.x + blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

__global__ __launch_bounds__(256) void ct_ring_emit_kernel(const i32x4* state, const int32_t* eid, const int32_t* cnt,
                                                           const int32_t* rblk, int32_t* rkey, int32_t* rlead,
                                                           int32_t* ring_off, int cap, int E) {
  __shared__ int wsum[4];
  const int b = blockIdx.y, found = ct_found(cnt, b, E), Q = E / 4;
  if (blockIdx.x * kCtEdge >= found) return;   // the whole workgroup
  bool is[8];
  int n = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = blockIdx.x * kCtEdge + threadIdx.x * 8 + j;
    is[j] = c < found && state[(size_t)b * E + c].w == c;
    n += is[j];
  }
  int total;
  int r = rblk[(size_t)b * gridDim.x + blockIdx.x] + block_scan(n, wsum, &total);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (!is[j]) continue;
    const int c = blockIdx.x * kCtEdge + threadIdx.x * 8 + j;
    if (r < Q) {                               // always: a ring has at least four edges
      const int id = eid[(size_t)b * E + c];   // 1..cap
      rkey[(size_t)b * Q + r] = id;
      rlead[(size_t)b * Q + r] = c;
      atomicAdd(&ring_off[(size_t)b * (cap + 1) + id - 1], 1);
    }
    ++r;
  }
}

// src = (id, leader) -> dst = (id, leader)
struct ct_pay {
  const int32_t* sl;
  int32_t *dk, *dl;
  __device__ __forceinline__ void move(size_t i, size_t pos, int key) const {
    dk[pos] = key;
    dl[pos] = sl[i];
  }
};

__global__ __launch_bounds__(256) void ct_corner_count_kernel(const i32x4* state, const int32_t* rlead, const int32_t* cnt,
                                                              int32_t* rcount, int E) {
  const int b = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x, Q = E / 4;
  if (r >= Q) return;
  const size_t q0 = (size_t)b * Q;
  rcount[q0 + r] = r < cnt[4 * b + 2] ? state[(size_t)b * E + rlead[q0 + r]].y : 0;
}

__global__ __launch_bounds__(256) void ct_rows_kernel(const i32x4* state, const int32_t* rkey, const int32_t* rlead,
                                                      const int32_t* rfirst, const int32_t* cnt, const int32_t* ncorner,
                                                      int32_t* efirst, int32_t* rings, int32_t* n, int E) {
  const int b = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x, Q = E / 4, nr = cnt[4 * b + 2];
  if (r == 0) {
    const int found = cnt[4 * b + 1];
    *(i32x4*)(n + 4 * b) = i32x4{found, ncorner[2 * b + 1], nr, found <= E};
  }
  if (r >= nr) return;
  const size_t q0 = (size_t)b * Q;
  const int c = rlead[q0 + r], first = rfirst[q0 + r];
  const i32x4 u = state[(size_t)b * E + c];
  *(i32x4*)(rings + 4 * (q0 + r)) = i32x4{rkey[q0 + r], first, u.y, u.z};
  efirst[(size_t)b * E + c] = first;
}

__global__ __launch_bounds__(256) void ct_verts_kernel(const i32x4* state, const int32_t* key, const int32_t* corner,
                                                       const int32_t* efirst, const int32_t* cnt, int32_t* verts, int W,
                                                       int E) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ct_found(cnt, b, E)) return;
  const size_t r0 = (size_t)b * E;
  if (!corner[r0 + c]) return;
  const i32x4 u = state[r0 + c];
  const int at = efirst[r0 + u.w] + state[r0 + u.w].y - u.y;   // corners of the ring before this one
  const int k = key[r0 + c], s = k & 3, p = k >> 2, y = p / W, x = p - y * W;
  if ((unsigned)at < (unsigned)E)                              // always: the corners are edges
    *(i32x2*)(verts + 2 * (r0 + at)) = i32x2{x + (s == 1 || s == 2), y + (s >= 2)};
}

inline int ct_blocks(long long HW) { return (int)((HW + kSegPix - 1) / kSegPix); }
inline int ct_ring_blocks(long long E) { return (int)((E + kCtEdge - 1) / kCtEdge); }
inline int ct_doubling(long long E) {
  int r = 0;
  while ((1ll << r) < E) ++r;
  return r;
}

struct ct_layout {
  size_t state[2], lead[2], key, eid, corner, succ, pre, blk, rblk, cnt, ncorner, rkey[2], rlead[2], rcount, tab, words;
  int nblk, nrblk, passes, rounds;
};

// The sizes dfw_seg_contours refuses, and its rounds query with it: DFW_EINVAL before DFW_ERANGE.
static int ct_size_error(long long B, long long H, long long W, long long cap, long long E) {
  if (B < 1 || H < 1 || W < 1 || cap < 1) return DFW_EINVAL;
  if (E < 4 || (E & 3)) return DFW_EINVAL;
  // grid y carries B; a key is 4 * (y * W + x) + side < 4 * H * W, so 4 * H * W <= 2^31 - 1 keeps every key, every
  // position, HW itself and the block count in an int
  if (H > 65535 || W > 65535 || 4 * H * W > 0x7fffffffll || B > 65535) return DFW_ERANGE;
  // rows of verts and rings are addressed in words through a size_t; the scans and seg_zero_launch count in an int: E (so
  // E / 4, the ring rows, and 256 * chunks of them, the digit table) and B * (cap + 1), the words of ring_off
  if (B * E * 2 > 0x7fffffffll || B * (cap + 1) > 0x7fffffffll) return DFW_ERANGE;
  return 0;
}

static ct_layout ct_plan(long long B, long long HW, long long cap, long long E) {
  ct_layout l;
  const size_t Q = (size_t)(E / 4), BE = (size_t)B * E;
  l.nblk = ct_blocks(HW);
  l.nrblk = ct_ring_blocks(E);
  l.passes = seg_key_passes(cap + 1);
  l.rounds = ct_doubling(E);
  size_t w = 0;
  // the 16-byte and 8-byte records first: every one starts at a multiple of 16 bytes of an aligned workspace (E % 4 == 0)
  for (int i = 0; i < 2; ++i) l.state[i] = w, w += 4 * BE;
  for (int i = 0; i < 2; ++i) l.lead[i] = w, w += 2 * BE;
  l.key = w, w += BE;
  l.eid = w, w += BE;
  l.corner = w, w += BE;
  l.succ = w, w += BE;
  l.cnt = w, w += 4 * (size_t)B;
  l.ncorner = w, w += 2 * (size_t)B;
  l.pre = w, w += (size_t)B * HW;
  l.blk = w, w += (size_t)B * l.nblk;
  l.rblk = w, w += (size_t)B * l.nrblk;
  for (int i = 0; i < 2; ++i) l.rkey[i] = w, w += (size_t)B * Q;
  for (int i = 0; i < 2; ++i) l.rlead[i] = w, w += (size_t)B * Q;
  l.rcount = w, w += (size_t)B * Q;
  l.tab = w, w += (size_t)B * seg_table_words(Q);
  l.words = w;
  return l;
}

}  // namespace dfw

using namespace dfw;

extern "C" size_t dfw_seg_contours_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t cap, int32_t max_edges) {
  if (B < 1 || H < 1 || W < 1 || cap < 1 || max_edges < 4 || (max_edges & 3)) return 0;
  return ct_plan(B, (long long)H * W, cap, max_edges).words * 4;
}

extern "C" int dfw_seg_contours_block(int32_t* pixels, int32_t* edges) {
  if (!pixels || !edges) return DFW_EINVAL;
  *pixels = kSegPix;
  *edges = kCtEdge;
  return 0;
}

extern "C" int dfw_seg_contours_rounds(int32_t B, int32_t H, int32_t W, int32_t cap, int32_t max_edges,
                                       dfw_seg_contours_trips* out) {
  if (!out) return DFW_EINVAL;
  if (int e = ct_size_error(B, H, W, cap, max_edges)) return e;
  const ct_layout l = ct_plan(B, (long long)H * W, cap, max_edges);
  out->blocks = l.nblk;
  out->block_scan = seg_scan_rounds(l.nblk);
  out->doubling = l.rounds;
  out->ring_blocks = l.nrblk;
  out->ring_scan = seg_scan_rounds(l.nrblk);
  out->passes = l.passes;
  out->table_scan = seg_scan_rounds(seg_table_words(max_edges / 4));
  out->offsets_scan = seg_scan_rounds((long long)cap + 1);
  out->corners_scan = seg_scan_rounds(max_edges / 4);
  out->launches = 14 + 2 * l.rounds + 3 * l.passes;
  return 0;
}

extern "C" int dfw_seg_contours(const dfw_seg_contours_args* a, dfw_stream_t stream) {
  if (!a || !a->ids || !a->verts || !a->rings || !a->ring_off || !a->n || !a->ws) return DFW_EINVAL;
  if (a->connectivity != 4 && a->connectivity != 8) return DFW_EINVAL;
  if (int e = ct_size_error(a->B, a->H, a->W, a->cap, a->max_edges)) return e;
  const size_t need = dfw_seg_contours_workspace_bytes(a->B, a->H, a->W, a->cap, a->max_edges);
  if (a->ws_bytes < need) return DFW_EWORKSPACE;
  const seg_buf bufs[] = {seg_in(a->ids, (size_t)a->B * a->H * a->W * 4, 4),
                          seg_out(a->verts, (size_t)a->B * a->max_edges * 8, 8),               // rows of 8 bytes
                          seg_out(a->rings, (size_t)a->B * (a->max_edges / 4) * 16, 16),       // rows and records of 16
                          seg_out(a->ring_off, (size_t)a->B * ((size_t)a->cap + 1) * 4, 4),
                          seg_out(a->n, (size_t)a->B * 16, 16),
                          seg_out(a->ws, need, 16)};
  if (int e = seg_check_buffers(bufs)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int B = a->B, H = a->H, W = a->W, cap = a->cap, E = a->max_edges, Q = E / 4;
  const ct_layout l = ct_plan(B, (long long)H * W, cap, E);
  int32_t* ws = (int32_t*)a->ws;
  i32x4* state[2] = {(i32x4*)(ws + l.state[0]), (i32x4*)(ws + l.state[1])};
  i32x2* lead[2] = {(i32x2*)(ws + l.lead[0]), (i32x2*)(ws + l.lead[1])};
  int32_t *key = ws + l.key, *eid = ws + l.eid, *corner = ws + l.corner, *succ = ws + l.succ, *pre = ws + l.pre;
  int32_t *blk = ws + l.blk, *rblk = ws + l.rblk, *cnt = ws + l.cnt, *ncorner = ws + l.ncorner, *rcount = ws + l.rcount;
  const dim3 gpix(l.nblk, B), gedge((E + 255) / 256, B), gring(l.nrblk, B), grow((Q + 255) / 256, B), t(256);

  if (int e = seg_zero_launch(st, (uint32_t*)a->ring_off, B * (cap + 1), nullptr, 0)) return e;
  hipLaunchKernelGGL(ct_count_kernel, gpix, t, 0, st, a->ids, blk, H, W, cap);
  DFW_CHECK_LAUNCH();
  if (int e = seg_scan_launch(st, blk, 1, B, l.nblk, cnt, 4, E)) return e;
  hipLaunchKernelGGL(ct_emit_kernel, gpix, t, 0, st, a->ids, (const int32_t*)blk, (const int32_t*)cnt, pre, key, H, W, cap, E);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(ct_link_kernel, gedge, t, 0, st, a->ids, (const int32_t*)cnt, (const int32_t*)pre, (const int32_t*)key,
                     eid, succ, corner, lead[0], H, W, cap, E, a->connectivity);
  DFW_CHECK_LAUNCH();
  // the link left windows of one edge in lead[0]; every round doubles them, so R rounds reach 2^R >= E edges
  for (int r = 0; r < l.rounds; ++r) {
    hipLaunchKernelGGL(ct_lead_kernel, gedge, t, 0, st, (const i32x2*)lead[r & 1], lead[(r & 1) ^ 1], (const int32_t*)cnt, E);
    DFW_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(ct_rank_init_kernel, gedge, t, 0, st, (const i32x2*)lead[l.rounds & 1], (const int32_t*)key,
                     (const int32_t*)succ, (const int32_t*)corner, state[0], (const int32_t*)cnt, W, E);
  DFW_CHECK_LAUNCH();
  for (int r = 0; r < l.rounds; ++r) {
    hipLaunchKernelGGL(ct_rank_kernel, gedge, t, 0, st, (const i32x4*)state[r & 1], state[(r & 1) ^ 1], (const int32_t*)cnt, E);
    DFW_CHECK_LAUNCH();
  }
  const i32x4* fin = state[l.rounds & 1];
  hipLaunchKernelGGL(ct_ring_count_kernel, gring, t, 0, st, fin, (const int32_t*)cnt, rblk, E);
  DFW_CHECK_LAUNCH();
  if (int e = seg_scan_launch(st, rblk, 1, B, l.nrblk, cnt + 2, 4, Q)) return e;
  hipLaunchKernelGGL(ct_ring_emit_kernel, gring, t, 0, st, fin, (const int32_t*)eid, (const int32_t*)cnt, (const int32_t*)rblk,
                     ws + l.rkey[0], ws + l.rlead[0], a->ring_off, cap, E);
  DFW_CHECK_LAUNCH();
  if (int e = seg_scan_launch(st, a->ring_off, 1, B, cap + 1)) return e;
  const int32_t* const rkey[2] = {ws + l.rkey[0], ws + l.rkey[1]};
  int cur = 0;
  if (int e = seg_sort(st, rkey, ws + l.tab, cnt + 2, 4, B, Q, l.passes, &cur, [&](int p) {
        return ct_pay{ws + l.rlead[p & 1], ws + l.rkey[(p & 1) ^ 1], ws + l.rlead[(p & 1) ^ 1]};
      }))
    return e;
  const int32_t* rlead = ws + l.rlead[cur];
  hipLaunchKernelGGL(ct_corner_count_kernel, grow, t, 0, st, fin, rlead, (const int32_t*)cnt, rcount, E);
  DFW_CHECK_LAUNCH();
  if (int e = seg_scan_launch(st, rcount, 1, B, Q, ncorner, 2, 0x7fffffff)) return e;
  // succ is free since the rank began: it holds every ring's first corner row at its leader
  hipLaunchKernelGGL(ct_rows_kernel, grow, t, 0, st, fin, rkey[cur], rlead, (const int32_t*)rcount, (const int32_t*)cnt,
                     (const int32_t*)ncorner, succ, a->rings, a->n, E);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(ct_verts_kernel, gedge, t, 0, st, fin, (const int32_t*)key, (const int32_t*)corner, (const int32_t*)succ,
                     (const int32_t*)cnt, a->verts, W, E);
  DFW_CHECK_LAUNCH();
  return 0;
}
