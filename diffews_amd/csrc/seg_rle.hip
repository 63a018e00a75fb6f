// Run-length encoding of labelled objects (objects.object_runs): ids int32 [B][H][W] -> per image the runs of every object
// 1..cap as (start, length) rows grouped by id, an offset table over the ids, and (runs kept, runs found).  All integers:
// the result depends on no order of execution.
//
// A pixel's position is q = y * W + x (order 0, rows) or q = x * H + y (order 1, columns: COCO's order); its value v(q) is
// its id when 1 <= id <= cap and 0 otherwise.  A run is a maximal interval [s, s + l) of positions with one equal non-zero
// value; runs do NOT stop at the end of a row or column.  Of the `found` runs of an image the first kept = min(found,
// max_runs) in ascending s are encoded; runs [.., :kept] holds them grouped by id ascending and ascending in s within an
// id, object k's rows being run_off[k-1] .. run_off[k].  Ids [[1,1,0],[2,1,1]] with cap = 2: rows give (0,2) (4,2) | (3,1)
// and run_off = [0,2,3]; columns read 1,2,1,1,0,1 and give (0,1) (2,2) (5,1) | (1,1), run_off = [0,3,4], so object 1's
// uncompressed COCO counts are [0,1,1,2,1,1].
//
// The workspace is, per image, blk [nblk] | plane [HW] (order 1 only) | key, start, end [max_runs] | key, start, length
// [max_runs] (two digit passes and more only) | tab [256][nchunk], every word of it written before it is read (the caller
// initialises nothing); nblk = seg_blocks(HW), nchunk = seg_chunks(max_runs).  The compaction and the sort are the shared
// ones of seg_sort.h, which explains them; this file supplies the source (rle_src: the ids of either order, and the count
// per id), the payload (rle_pay) and no tail: the last sort pass lands in runs.  Launches, a number fixed by the arguments
// (5 + order + 3 * passes, passes = the bytes cap needs): no host readback in between:
//
//   0  seg_zero_launch               run_off (a library kernel, no memset node)
//   1  rle_transpose_kernel          order 1 only: ids [H][W] -> plane [W][H] through padded 32 x 32 LDS tiles; from here on
//                                    both orders are one linear array A of HW positions
//   2  seg_count_kernel<rle_src>     the starts per block of kSegPix positions
//   3  seg_scan_launch               exclusive scan of the block sums in place, nruns = (kept, found)
//   4  seg_emit_kernel<rle_src>      (id, s, e) of every kept run.  Each kept start also counts itself into run_off[id - 1]
//                                    (an integer atomic: a count, never a position)
//   5  seg_scan_launch               run_off: the exclusive scan of the counts shifted by one is the inclusive offset table
//   6+ seg_sort                      per key byte hist, scan, seg_scatter_kernel<rle_pay>.  The first pass turns the end
//                                    into a length, the last one lands in runs as (s, l)
//
// Termination: no thread waits for another thread or workgroup; every loop has a trip count fixed by the arguments, every
// cross-workgroup prefix is a scan in a launch of its own.  Any grid is correct at any residency.
#include "seg_args.h"
#include "seg_sort.h"

namespace dfw {

constexpr int kRleTT = 32;      // transpose tile

__device__ __forceinline__ int rle_value(int id, int cap) { return (id >= 1 && id <= cap) ? id : 0; }

// The linear array A [B][HW] of either order; the value of a position is its id when 1 <= id <= cap and 0 otherwise.
struct rle_src {
  const int32_t* A;
  int cap;
  int32_t* run_off;   // [B][cap + 1]

  __device__ __forceinline__ void load9(int b, int HW, int p0, int (&v)[9]) const {
    const int32_t* a = A + (size_t)b * HW;
    v[0] = (p0 >= 1 && p0 - 1 < HW) ? rle_value(a[p0 - 1], cap) : 0;
    if (p0 + 8 <= HW && ((uintptr_t)(a + p0) & 15) == 0) {
      const i32x4 q0 = *(const i32x4*)(a + p0), q1 = *(const i32x4*)(a + p0 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[1 + j] = rle_value(q0[j], cap);
        v[5 + j] = rle_value(q1[j], cap);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[1 + j] = p0 + j < HW ? rle_value(a[p0 + j], cap) : 0;
    }
  }
  __device__ __forceinline__ void kept(int b, int key) const { atomicAdd(&run_off[(size_t)b * (cap + 1) + key - 1], 1); }
};

// src = (key, s, x): x is the run's end in the first pass, its length afterwards.  dst = (key, s, l) arrays, or (last) rows
// (s, l) of runs and no key: with one digit pass there is no second record buffer.
struct rle_pay {
  const int32_t *ss, *sx;
  int32_t *dkey, *ds, *dl, *runs;
  int first, last;

  __device__ __forceinline__ void move(size_t i, size_t pos, int key) const {
    const int s = ss[i], x = sx[i], l = first ? x - s : x;
    if (last) {
      runs[2 * pos] = s;
      runs[2 * pos + 1] = l;
    } else {
      dkey[pos] = key;
      ds[pos] = s;
      dl[pos] = l;
    }
  }
};

__global__ __launch_bounds__(256) void rle_transpose_kernel(const int32_t* ids, int32_t* plane, int H, int W) {
  __shared__ int t[kRleTT][kRleTT + 1];
  const size_t img = (size_t)blockIdx.z * H * W;
  const int x0 = blockIdx.x * kRleTT, y0 = blockIdx.y * kRleTT, lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = y0 + ly + 8 * k, x = x0 + lx;
    if (y < H && x < W) t[ly + 8 * k][lx] = ids[img + (size_t)y * W + x];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = x0 + ly + 8 * k, y = y0 + lx;
    if (x < W && y < H) plane[img + (size_t)x * H + y] = t[lx][ly + 8 * k];
  }
}

// Words of run_off per image, the scan behind the emit.
inline int rle_offsets(long long cap) { return (int)(cap + 1); }

struct rle_layout {
  size_t blk, plane, rec[2], tab, words;   // offsets in words, for all B images
  int nblk, passes;
};
// The sizes dfw_seg_rle refuses, and its rounds query with it: DFW_EINVAL before DFW_ERANGE.
static int rle_size_error(long long B, long long H, long long W, long long cap, long long max_runs, int order) {
  if (B < 1 || H < 1 || W < 1 || cap < 1 || max_runs < 1) return DFW_EINVAL;
  if (order != 0 && order != 1) return DFW_EINVAL;
  if (int e = seg_map_size_error(B, H, W)) return e;
  // rows of runs are addressed in words: B * max_runs * 2 < 2^31, which also bounds max_runs below 2^30 and the digit
  // table, 256 * nchunk <= 2^27 words an image, inside an int
  if (B * max_runs * 2 > 0x7fffffffll) return DFW_ERANGE;
  // seg_zero_launch counts run_off's B * (cap + 1) words in an int (so cap + 1 does not wrap either)
  if (B * (cap + 1) > 0x7fffffffll) return DFW_ERANGE;
  return 0;
}

static rle_layout rle_plan(long long B, long long HW, int cap, long long max_runs, int order) {
  rle_layout l;
  l.nblk = seg_blocks(HW);
  l.passes = seg_key_passes((long long)cap + 1);
  size_t w = 0;
  l.blk = w, w += (size_t)B * l.nblk;
  w = (w + 3) & ~(size_t)3;                // the plane at 16 bytes from an aligned workspace: vector loads
  l.plane = w, w += order == 1 ? (size_t)B * HW : 0;
  l.rec[0] = w, w += 3 * (size_t)B * max_runs;
  l.rec[1] = w, w += l.passes > 1 ? 3 * (size_t)B * max_runs : 0;
  l.tab = w, w += (size_t)B * 256 * seg_chunks(max_runs);
  l.words = w;
  return l;
}

}  // namespace dfw

using namespace dfw;

extern "C" size_t dfw_seg_rle_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t cap, int32_t max_runs, int32_t order) {
  if (B < 1 || H < 1 || W < 1 || cap < 1 || max_runs < 1 || (order != 0 && order != 1)) return 0;
  return rle_plan(B, (long long)H * W, cap, max_runs, order).words * 4;
}

extern "C" int dfw_seg_rle_block(int32_t* pixels, int32_t* records) {
  if (!pixels || !records) return DFW_EINVAL;
  *pixels = kSegPix;
  *records = kSegRec;
  return 0;
}

extern "C" int dfw_seg_rle_rounds(int32_t B, int32_t H, int32_t W, int32_t cap, int32_t max_runs, int32_t order,
                                  dfw_seg_sort_rounds* out) {
  if (!out) return DFW_EINVAL;
  if (int e = rle_size_error(B, H, W, cap, max_runs, order)) return e;
  const rle_layout l = rle_plan(B, (long long)H * W, cap, max_runs, order);
  out->blocks = l.nblk;
  out->block_scan = seg_scan_rounds(l.nblk);
  out->passes = l.passes;
  out->table_scan = seg_scan_rounds(seg_table_words(max_runs));
  out->offsets_scan = seg_scan_rounds(rle_offsets(cap));
  out->heads_scan = 0;
  return 0;
}

extern "C" int dfw_seg_rle(const dfw_seg_rle_args* a, dfw_stream_t stream) {
  if (!a || !a->ids || !a->runs || !a->run_off || !a->nruns || !a->ws) return DFW_EINVAL;
  if (int e = rle_size_error(a->B, a->H, a->W, a->cap, a->max_runs, a->order)) return e;
  const size_t need = dfw_seg_rle_workspace_bytes(a->B, a->H, a->W, a->cap, a->max_runs, a->order);
  if (a->ws_bytes < need) return DFW_EWORKSPACE;
  const seg_buf bufs[] = {seg_in(a->ids, (size_t)a->B * a->H * a->W * 4, 4),
                          seg_out(a->runs, (size_t)a->B * a->max_runs * 8, 4),
                          seg_out(a->run_off, (size_t)a->B * ((size_t)a->cap + 1) * 4, 4),
                          seg_out(a->nruns, (size_t)a->B * 8, 4),
                          seg_out(a->ws, need, 4)};
  if (int e = seg_check_buffers(bufs)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int B = a->B, H = a->H, W = a->W, cap = a->cap, M = a->max_runs, iHW = H * W;
  const rle_layout l = rle_plan(B, iHW, cap, M, a->order);
  int32_t* ws = (int32_t*)a->ws;
  int32_t* blk = ws + l.blk;
  int32_t* rec[2][3];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 3; ++j) rec[i][j] = ws + l.rec[i] + (size_t)j * B * M;
  if (int e = seg_zero_launch(st, (uint32_t*)a->run_off, B * (cap + 1), nullptr, 0)) return e;
  rle_src src = {a->ids, cap, a->run_off};
  if (a->order == 1) {
    hipLaunchKernelGGL(rle_transpose_kernel, dim3((W + kRleTT - 1) / kRleTT, (H + kRleTT - 1) / kRleTT, B), dim3(256), 0, st,
                       a->ids, ws + l.plane, H, W);
    DFW_CHECK_LAUNCH();
    src.A = ws + l.plane;
  }
  hipLaunchKernelGGL(seg_count_kernel<rle_src>, dim3(l.nblk, B), dim3(256), 0, st, src, blk, iHW);
  DFW_CHECK_LAUNCH();
  if (int e = seg_scan_launch(st, blk, 1, B, l.nblk, a->nruns, 2, M)) return e;
  hipLaunchKernelGGL(seg_emit_kernel<rle_src>, dim3(l.nblk, B), dim3(256), 0, st, src, (const int32_t*)blk, rec[0][0],
                     rec[0][1], rec[0][2], iHW, M);
  DFW_CHECK_LAUNCH();
  if (int e = seg_scan_launch(st, a->run_off, 1, B, rle_offsets(cap))) return e;
  const int32_t* const key[2] = {rec[0][0], rec[1][0]};
  return seg_sort(st, key, ws + l.tab, a->nruns, 2, B, M, l.passes, nullptr, [&](int p) {   // the last pass lands in runs
    int32_t** s = rec[p & 1];
    int32_t** d = rec[(p & 1) ^ 1];
    return rle_pay{s[1], s[2], d[0], d[1], d[2], a->runs, p == 0, p == l.passes - 1};
  });
}
