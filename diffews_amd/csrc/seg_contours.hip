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
//
// The optional last stage, the SIMPLIFIED RINGS (three more launches when simp_verts / simp_rings / simp_n are given), is
// described in front of its kernels below; its loops are bounded by the ring's length and not by the arguments alone.
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

// ------------------------------------------------------------------------------------------------ simplified rings
// The optional last stage (simp_verts / simp_rings / simp_n / tol4 of the arguments; include/diffews_hip.h holds the
// definition): Douglas-Peucker on every ring in its level-synchronous form, all integers, three launches behind
// ct_verts_kernel and none when the stage is off:
//
//   sp_keep_kernel    one workgroup per ring row (grid-stride over the rings the image has).  Anchors 0 and f, then
//                     rounds: every active corner puts the packed key of its measure into the winner slot of its
//                     chain's left anchor with a 64-bit integer max (order-free; sp_slot_max folds a wave first), barrier,
//                     every active corner reads its chain's winner and is kept, dropped or narrows its chain, barrier
//                     with the workgroup-wide "any active", the kept winners clear the slot they won, barrier.  Corner i
//                     belongs to thread i % 256 in every loop, so a, b and the status are private to a thread; only the
//                     slots are shared.  A ring of at most kSpLds corners keeps coordinates, state and slots in LDS, a
//                     longer one in the workspace (the slots through device-scope atomics only).  Then rule 3, and the
//                     exclusive prefix of the keep flags inside the ring (block_scan, 256 corners a trip):
//                     pos [corner row] = its rank among the ring's kept corners or -1, kcount [ring row] = corners kept
//   sp_scan_kernel    kcount in place -> every ring's first', and the corners kept of the image: block_scan, 1024 rings
//                     a trip, over the rings the image has
//   sp_write_kernel   one workgroup per ring row: simp_rings' row, the kept corners at first' + pos, and simp_n
//
// The rounds end: a round leaves every live chain finished or with one more kept corner, at most count - 2 rounds.  The
// exit test is the barrier's own result, uniform over the workgroup.  The state lives in what was `state` and `lead`,
// 48 bytes per edge, dead since ct_verts_kernel: slot [E] x 8 | a, b, status, pos [E] | kcount [Q] | kept [2] per image.

constexpr int kSpLds = 1024;    // corners of a ring up to which its state lives in LDS
constexpr int kSpGrid = 8192;   // workgroups per image at the most; the rows beyond are reached by the stride

using u64 = unsigned long long;

enum { kSpActive = 0, kSpKept = 1, kSpDropped = 2, kSpWon = 3 };

// line mode (pa != pb): |cross| of (pb - pa, p - pa), twice the triangle's area; point mode: the squared distance to pa
__device__ __forceinline__ u64 sp_measure(i32x2 pa, i32x2 pb, i32x2 p) {
  const long long ux = pb.x - pa.x, uy = pb.y - pa.y, vx = p.x - pa.x, vy = p.y - pa.y;
  if (ux == 0 && uy == 0) return (u64)(vx * vx + vy * vy);
  const long long cr = ux * vy - uy * vx;
  return (u64)(cr < 0 ? -cr : cr);
}

// 16 m^2 > tol4^2 L, or 16 m > tol4^2 in point mode: below 2^64 by the bounds of the header
__device__ __forceinline__ bool sp_keeps(i32x2 pa, i32x2 pb, u64 m, u64 tol2) {
  const long long ux = pb.x - pa.x, uy = pb.y - pa.y;
  if (ux == 0 && uy == 0) return 16 * m > tol2;
  return 16 * m * m > tol2 * (u64)(ux * ux + uy * uy);
}

template <bool LDS>
__device__ __forceinline__ u64 sp_slot_load(u64* p) {
  if (LDS) return *p;
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // written by atomics: never from a stale line
}
template <bool LDS>
__device__ __forceinline__ void sp_slot_clear(u64* p) {
  if (LDS) *p = 0;
  else __hip_atomic_store(p, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// key into slot [a] by an integer max, for the lanes that are `on`.  A wave's lanes hold consecutive corners, so early on
// all of them belong to one or two chains and would queue at one address: the lanes that share the first pending lane's
// chain fold their keys with shuffles and that lane alone goes to memory, twice over; whoever is left (many small chains)
// goes by itself.  A maximum does not depend on how it is grouped.  Every lane of the wave calls it.
__device__ __forceinline__ void sp_slot_max(u64* slot, bool on, int a, u64 key) {
  const int lane = threadIdx.x & 63;
  bool pending = on;
  for (int it = 0; it < 2; ++it) {
    const unsigned long long act = __ballot(pending);
    if (act == 0) return;                               // the whole wave
    const int lead = __ffsll((long long)act) - 1;
    const int la = __shfl(a, lead, 64);
    const bool same = pending && a == la;
    if (__popcll(__ballot(same)) < 8) break;            // the whole wave: small chains from here on
    u64 v = same ? key : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (u64)__shfl_xor(v, o, 64));
    if (lane == lead) atomicMax(&slot[la], v);
    pending = pending && !same;
  }
  if (pending) atomicMax(&slot[a], key);
}

// The largest key of the workgroup; red is one LDS word.  Two barriers in front of the read, none behind it: the caller
// puts one between this and the next use of red.
__device__ __forceinline__ u64 sp_block_max(u64 v, u64* red) {
  if (threadIdx.x == 0) *red = 0;
  __syncthreads();
  atomicMax(red, v);
  __syncthreads();
  return *red;
}

// One ring of c >= 4 corners P[0..c); slot, sa, sb, sst are [c], in LDS or in the workspace; pos [c] and *kcount are the
// workspace's.  Every thread of the workgroup calls it.
template <bool LDS>
__device__ __forceinline__ void sp_ring(const i32x2* P, int c, u64* slot, int* sa, int* sb, int* sst, int32_t* pos,
                                        int32_t* kcount, u64 tol2, u64* red, int* wsum) {
  const int tid = threadIdx.x;
  const i32x2 p0 = P[0];
  u64 best = 0;
  for (int i = tid; i < c; i += 256) {
    sp_slot_clear<LDS>(&slot[i]);
    best = max(best, sp_measure(p0, p0, P[i]) << 31 | (u64)(0x7fffffff - i));
  }
  int f = 0x7fffffff - (int)(sp_block_max(best, red) & 0x7fffffff);            // the barriers also publish the slots
  if ((unsigned)f >= (unsigned)c) f = 0;                                        // never: a key carries a rank below c
  const i32x2 pf = P[f];
  for (int i = tid; i < c; i += 256) {
    const bool anchor = i == 0 || i == f;
    sst[i] = anchor ? kSpKept : kSpActive;
    sa[i] = i < f ? 0 : f;
    sb[i] = i < f ? f : c;
  }
  // every round every active corner is settled or its chain (a, b) narrows around it: fewer than c rounds, whatever
  // the slots hold
  for (int round = 0; round < c; ++round) {
    for (int base = 0; base < c; base += 256) {          // the same trips for every lane: sp_slot_max shuffles
      const int i = base + tid;
      const bool on = i < c && sst[i] == kSpActive;
      int a = -1;
      u64 key = 0;
      if (on) {
        a = sa[i];
        const int b = sb[i], s = 2 * i - (a + b);
        key = sp_measure(P[a], P[b == c ? 0 : b], P[i]) << 31 | (u64)(0x7fffffff - (2 * (s < 0 ? -s : s) + (s > 0)));
      }
      sp_slot_max(slot, on, a, key);
    }
    __syncthreads();
    int any = 0;
    for (int i = tid; i < c; i += 256) {
      if (sst[i] != kSpActive) continue;
      const int a = sa[i], b = sb[i];
      const u64 k = sp_slot_load<LDS>(&slot[a]);
      const int t = 0x7fffffff - (int)(k & 0x7fffffff), d = t >> 1, w = (a + b + ((t & 1) ? d : -d)) >> 1;
      if (w <= a || w >= b || !sp_keeps(P[a], P[b == c ? 0 : b], k >> 31, tol2)) sst[i] = kSpDropped;   // w is interior
      else if (i == w) sst[i] = kSpWon;                 // sa[i] still names the slot it won
      else if (i < w) sb[i] = w, any = 1;
      else sa[i] = w, any = 1;
    }
    const int more = __syncthreads_or(any);           // every slot of this round has been read
    for (int i = tid; i < c; i += 256)
      if (sst[i] == kSpWon) {
        sp_slot_clear<LDS>(&slot[sa[i]]);
        sst[i] = kSpKept;
      }
    if (!more) break;
    __syncthreads();
  }
  int mine = 0;
  for (int i = tid; i < c; i += 256) mine += sst[i] == kSpKept;
  int kept;
  block_scan(mine, wsum, &kept);
  if (kept == 2) {                                      // rule 3, the whole workgroup: a ring keeps three corners
    best = 0;
    for (int i = tid; i < c; i += 256)
      if (i != 0 && i != f) best = max(best, sp_measure(p0, pf, P[i]) << 31 | (u64)(0x7fffffff - i));
    const int g = 0x7fffffff - (int)(sp_block_max(best, red) & 0x7fffffff);
    if ((unsigned)g < (unsigned)c && (g & 255) == tid) sst[g] = kSpKept;
  }
  int carry = 0;
  for (int i0 = 0; i0 < c; i0 += 256) {
    const int i = i0 + tid;
    const int on = i < c && sst[i] == kSpKept;
    int total;
    const int ex = block_scan(on, wsum, &total);
    if (i < c) pos[i] = on ? carry + ex : -1;
    carry += total;
  }
  if (tid == 0) *kcount = carry;
}

__global__ __launch_bounds__(256) void sp_keep_kernel(const int32_t* verts, const int32_t* rings, const int32_t* n,
                                                      u64* slot, int32_t* sa, int32_t* sb, int32_t* sst, int32_t* pos,
                                                      int32_t* kcount, int E, int tol4) {
  __shared__ __attribute__((aligned(16))) i32x2 lp[kSpLds];
  __shared__ __attribute__((aligned(16))) u64 lslot[kSpLds];
  __shared__ __attribute__((aligned(16))) int la[kSpLds];
  __shared__ __attribute__((aligned(16))) int lb[kSpLds];
  __shared__ __attribute__((aligned(16))) int ls[kSpLds];
  __shared__ __attribute__((aligned(16))) u64 red[2];
  __shared__ __attribute__((aligned(16))) int wsum[4];
  const int b = blockIdx.y, Q = E / 4, nr = min(n[4 * b + 2], Q);
  const size_t r0 = (size_t)b * E, q0 = (size_t)b * Q;
  const u64 tol2 = (u64)tol4 * (u64)tol4;
  for (int r = blockIdx.x; r < nr; r += gridDim.x) {    // r and nr are the workgroup's: every barrier below is met by all
    const i32x4 ring = *(const i32x4*)(rings + 4 * (q0 + r));
    const int first = ring.y, c = ring.z;
    if (first < 0 || c < 4 || (long long)first + c > E) {   // never: a ring's corners are rows of verts
      if (threadIdx.x == 0) kcount[q0 + r] = 0;
      continue;
    }
    const i32x2* P = (const i32x2*)verts + r0 + first;
    if (c <= kSpLds) {
      for (int i = threadIdx.x; i < c; i += 256) lp[i] = P[i];
      __syncthreads();
      sp_ring<true>(lp, c, lslot, la, lb, ls, pos + r0 + first, kcount + q0 + r, tol2, red, wsum);
    } else {
      sp_ring<false>(P, c, slot + r0 + first, sa + r0 + first, sb + r0 + first, sst + r0 + first, pos + r0 + first,
                     kcount + q0 + r, tol2, red, wsum);
    }
    __syncthreads();                                    // the next ring of this workgroup takes the same LDS
  }
}

// kcount [rings of the image] -> its exclusive prefix in place, every ring's first', and kept [2 b .. 2 b + 1] = the corners
// kept of image b.  One workgroup per image, 1024 rows a trip, as seg_scan_kernel -- but over the rings the image has and
// not over the E / 4 rows it may have: at most ceil(E / 4096) trips.
__global__ __launch_bounds__(256) void sp_scan_kernel(const int32_t* n, int32_t* kcount, int32_t* kept, int E) {
  __shared__ __attribute__((aligned(16))) int wsum[4];
  const int b = blockIdx.x, Q = E / 4, nr = min(n[4 * b + 2], Q);
  int32_t* a = kcount + (size_t)b * Q;
  int carry = 0;
  for (int r0 = 0; r0 < nr; r0 += 1024) {
    const int r = r0 + 4 * threadIdx.x;
    int v[4], total;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = r + j < nr ? a[r + j] : 0;
    int ex = carry + block_scan(v[0] + v[1] + v[2] + v[3], wsum, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (r + j < nr) a[r + j] = ex;
      ex += v[j];
    }
    carry += total;
  }
  if (threadIdx.x == 0) kept[2 * b] = kept[2 * b + 1] = carry;
}

// kfirst = kcount after its scan; kept [2 b + 1] = the corners kept of image b
__global__ __launch_bounds__(256) void sp_write_kernel(const int32_t* verts, const int32_t* rings, const int32_t* n,
                                                       const int32_t* pos, const int32_t* kfirst, const int32_t* kept,
                                                       int32_t* simp_verts, int32_t* simp_rings, int32_t* simp_n, int E) {
  const int b = blockIdx.y, Q = E / 4;
  const i32x4 nn = *(const i32x4*)(n + 4 * b);
  const int nr = min(nn.z, Q), total = kept[2 * b + 1];
  const size_t r0 = (size_t)b * E, q0 = (size_t)b * Q;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *(i32x4*)(simp_n + 4 * b) = nn.w ? i32x4{nn.y, total, nr, 1} : i32x4{0, 0, 0, 0};
  for (int r = blockIdx.x; r < nr; r += gridDim.x) {
    const i32x4 ring = *(const i32x4*)(rings + 4 * (q0 + r));
    const int first = ring.y, c = ring.z, f2 = kfirst[q0 + r];
    if (first < 0 || c < 4 || (long long)first + c > E) continue;   // never, as in sp_keep_kernel
    if (threadIdx.x == 0)
      *(i32x4*)(simp_rings + 4 * (q0 + r)) = i32x4{ring.x, f2, (r + 1 < nr ? kfirst[q0 + r + 1] : total) - f2, ring.w};
    for (int i = threadIdx.x; i < c; i += 256) {
      const int p = pos[r0 + first + i];
      if (p >= 0 && (unsigned)(f2 + p) < (unsigned)E)   // always: the kept corners are corners
        *(i32x2*)(simp_verts + 2 * (r0 + f2 + p)) = *(const i32x2*)(verts + 2 * (r0 + first + i));
    }
  }
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
  // the simplification's state, inside state and lead (12 words per edge, dead by then)
  size_t sp_slot, sp_a, sp_b, sp_st, sp_pos, sp_kcount, sp_kept;
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
  // 2 + 4 words per edge, then Q + 2 per image: 6 E + E / 4 + 2 <= 12 E for every E >= 4
  l.sp_slot = l.state[0], l.sp_a = l.sp_slot + 2 * BE, l.sp_b = l.sp_a + BE, l.sp_st = l.sp_b + BE, l.sp_pos = l.sp_st + BE;
  l.sp_kcount = l.sp_pos + BE, l.sp_kept = l.sp_kcount + (size_t)B * Q;
  static_assert(sizeof(u64) == 8, "a winner slot is two words");
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

extern "C" int dfw_seg_contours_simplify_block(int32_t* lds_corners) {
  if (!lds_corners) return DFW_EINVAL;
  *lds_corners = kSpLds;
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
  out->simplify_launches = 3;
  return 0;
}

extern "C" int dfw_seg_contours(const dfw_seg_contours_args* a, dfw_stream_t stream) {
  if (!a || !a->ids || !a->verts || !a->rings || !a->ring_off || !a->n || !a->ws) return DFW_EINVAL;
  if (a->connectivity != 4 && a->connectivity != 8) return DFW_EINVAL;
  const bool simplify = a->simp_verts || a->simp_rings || a->simp_n;
  if (simplify ? (!a->simp_verts || !a->simp_rings || !a->simp_n || a->tol4 < 0 || a->tol4 > 32768) : a->tol4 != 0)
    return DFW_EINVAL;
  if (int e = ct_size_error(a->B, a->H, a->W, a->cap, a->max_edges)) return e;
  const size_t need = dfw_seg_contours_workspace_bytes(a->B, a->H, a->W, a->cap, a->max_edges);
  if (a->ws_bytes < need) return DFW_EWORKSPACE;
  const seg_buf bufs[] = {seg_in(a->ids, (size_t)a->B * a->H * a->W * 4, 4),
                          seg_out(a->verts, (size_t)a->B * a->max_edges * 8, 8),               // rows of 8 bytes
                          seg_out(a->rings, (size_t)a->B * (a->max_edges / 4) * 16, 16),       // rows and records of 16
                          seg_out(a->ring_off, (size_t)a->B * ((size_t)a->cap + 1) * 4, 4),
                          seg_out(a->n, (size_t)a->B * 16, 16),
                          seg_out(a->ws, need, 16),
                          seg_out(a->simp_verts, (size_t)a->B * a->max_edges * 8, 8),          // absent when the stage is off
                          seg_out(a->simp_rings, (size_t)a->B * (a->max_edges / 4) * 16, 16),
                          seg_out(a->simp_n, (size_t)a->B * 16, 16)};
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
  if (!simplify) return 0;
  // state and lead are dead from here on
  int32_t *pos = ws + l.sp_pos, *kcount = ws + l.sp_kcount, *kept = ws + l.sp_kept;
  const dim3 gsimp(Q < kSpGrid ? Q : kSpGrid, B);
  hipLaunchKernelGGL(sp_keep_kernel, gsimp, t, 0, st, (const int32_t*)a->verts, (const int32_t*)a->rings, (const int32_t*)a->n,
                     (u64*)(ws + l.sp_slot), ws + l.sp_a, ws + l.sp_b, ws + l.sp_st, pos, kcount, E, a->tol4);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_scan_kernel, dim3(B), t, 0, st, (const int32_t*)a->n, kcount, kept, E);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(sp_write_kernel, gsimp, t, 0, st, (const int32_t*)a->verts, (const int32_t*)a->rings, (const int32_t*)a->n,
                     (const int32_t*)pos, (const int32_t*)kcount, (const int32_t*)kept, a->simp_verts, a->simp_rings, a->simp_n, E);
  DFW_CHECK_LAUNCH();
  return 0;
}
