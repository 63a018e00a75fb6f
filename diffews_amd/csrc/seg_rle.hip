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
// initialises nothing).  nblk = (HW + 1) / kRlePix rounded up: position HW, behind the image, has value 0 and is always
// covered, which is what closes a run that reaches the image's end.  nchunk = max_runs / kRleRec rounded up.  Launches, a
// number fixed by the arguments (5 + order + 3 * passes, passes = the bytes cap needs): no host readback in between:
//
//   0  seg_zero_launch       run_off (a library kernel, no memset node)
//   1  rle_transpose_kernel  order 1 only: ids [H][W] -> plane [W][H] through padded 32 x 32 LDS tiles; from here on both
//                            orders are one linear array A of HW positions
//   2  rle_count_kernel      per block of kRlePix positions: the starts, v(q) != v(q-1) and v(q) != 0 (v(-1) = 0; the
//                            block's first position reads its predecessor across the border)
//   3  rle_scan_kernel       one workgroup per image: exclusive scan of the block sums in place, nruns = (kept, found)
//   4  rle_emit_kernel       every position with v(q) != v(q-1) holds c, the number of starts before q.  A start writes
//                            start[c] = q, key[c] = v(q); an end (v(q-1) != 0) writes end[c-1] = q, the run that ends at q
//                            being the most recent start -- so one compaction gives (id, s, e) of every run, runs over
//                            many blocks included.  Ranks >= max_runs are skipped.  Each kept start also counts itself
//                            into run_off[id - 1] (an integer atomic: a count, never a position)
//   5  rle_scan_kernel       run_off: the exclusive scan of the counts shifted by one is the inclusive offset table
//   6+ per key byte, lowest first -- a stable LSD radix sort of the kept records:
//        rle_hist_kernel     per chunk of kRleRec records the digit histogram -> tab [digit][chunk]
//        rle_scan_kernel     exclusive scan of tab in place, digit-major
//        rle_scatter_kernel  record i of the chunk goes to tab[digit][chunk] + its rank among the chunk's earlier records
//                            of that digit.  Ranks come from ballots inside a wave, per-wave counts across the four waves
//                            and a running count across the rounds of 256: a fixed order, no atomic decides a position.
//                            The first pass turns the end into a length, the last one lands in runs as (s, l)
//
// Termination: no thread waits for another thread or workgroup; every loop has a trip count fixed by the arguments, every
// cross-workgroup prefix is a scan in a launch of its own.  Any grid is correct at any residency.
#include "common.h"
#include "seg_scan.h"

namespace dfw {

constexpr int kRlePix = 2048;   // positions per scan block, 8 per thread of 256
constexpr int kRleRec = 2048;   // records per sort chunk, 8 rounds of 256
constexpr int kRleTT = 32;      // transpose tile

__device__ __forceinline__ int rle_value(int id, int cap) { return (id >= 1 && id <= cap) ? id : 0; }

// v[0] = v(p0 - 1), v[1 + j] = v(p0 + j) of the linear array A [HW]; positions outside [0, HW) have value 0.
__device__ __forceinline__ void rle_load9(const int32_t* A, int HW, int p0, int cap, int (&v)[9]) {
  v[0] = (p0 >= 1 && p0 - 1 < HW) ? rle_value(A[p0 - 1], cap) : 0;
  if (p0 + 8 <= HW && ((uintptr_t)(A + p0) & 15) == 0) {
    const i32x4 q0 = *(const i32x4*)(A + p0), q1 = *(const i32x4*)(A + p0 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[1 + j] = rle_value(q0[j], cap);
      v[5 + j] = rle_value(q1[j], cap);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[1 + j] = p0 + j < HW ? rle_value(A[p0 + j], cap) : 0;
  }
}

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

__global__ __launch_bounds__(256) void rle_count_kernel(const int32_t* A, int32_t* blk, int HW, int cap) {
  __shared__ int ws[4];
  int v[9];
  rle_load9(A + (size_t)blockIdx.y * HW, HW, blockIdx.x * kRlePix + threadIdx.x * 8, cap, v);
  int n = 0;
#pragma unroll
  for (int j = 1; j < 9; ++j) n += v[j] != v[j - 1] && v[j] != 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) blk[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// a [image][n]: exclusive scan in place, 4 consecutive words per thread and round.  nruns (optional) [image] = (min(sum,
// max_runs), sum).
__global__ __launch_bounds__(256) void rle_scan_kernel(int32_t* a, int n, int32_t* nruns, int max_runs) {
  __shared__ int wsum[4];
  int32_t* o = a + (size_t)blockIdx.x * n;
  int carry = 0;
  for (int base = 0; base < n; base += 1024) {
    const int i0 = base + 4 * threadIdx.x;
    int v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = i0 + j < n ? o[i0 + j] : 0;
      s += v[j];
    }
    int total;
    int e = carry + block_scan(s, wsum, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i0 + j < n) o[i0 + j] = e;
      e += v[j];
    }
    carry += total;
  }
  if (nruns && threadIdx.x == 0) {
    nruns[2 * blockIdx.x] = min(carry, max_runs);
    nruns[2 * blockIdx.x + 1] = carry;
  }
}

__global__ __launch_bounds__(256) void rle_emit_kernel(const int32_t* A, const int32_t* blk, int32_t* key, int32_t* start,
                                                       int32_t* end, int32_t* run_off, int HW, int cap, int max_runs) {
  __shared__ int wsum[4];
  const int b = blockIdx.y, p0 = blockIdx.x * kRlePix + threadIdx.x * 8;
  int v[9];
  rle_load9(A + (size_t)b * HW, HW, p0, cap, v);
  int n = 0;
#pragma unroll
  for (int j = 1; j < 9; ++j) n += v[j] != v[j - 1] && v[j] != 0;
  int total;
  int c = blk[(size_t)b * gridDim.x + blockIdx.x] + block_scan(n, wsum, &total);   // starts before p0
  const size_t r0 = (size_t)b * max_runs;
#pragma unroll
  for (int j = 1; j < 9; ++j) {
    if (v[j] == v[j - 1]) continue;
    const int q = p0 + j - 1;
    if (v[j - 1] != 0 && (unsigned)(c - 1) < (unsigned)max_runs) end[r0 + c - 1] = q;   // c >= 1: it started before q
    if (v[j] != 0) {
      if (c < max_runs) {
        start[r0 + c] = q;
        key[r0 + c] = v[j];
        atomicAdd(&run_off[(size_t)b * (cap + 1) + v[j] - 1], 1);
      }
      ++c;
    }
  }
}

__global__ __launch_bounds__(256) void rle_hist_kernel(const int32_t* key, int32_t* tab, const int32_t* nruns, int max_runs,
                                                       int shift) {
  __shared__ int hist[256];
  const int b = blockIdx.y, nchunk = gridDim.x, kept = min(nruns[2 * b], max_runs);
  hist[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRleRec / 256; ++r) {
    const int i = blockIdx.x * kRleRec + r * 256 + threadIdx.x;
    if (i < kept) atomicAdd(&hist[(key[(size_t)b * max_runs + i] >> shift) & 255], 1);
  }
  __syncthreads();
  tab[((size_t)b * 256 + threadIdx.x) * nchunk + blockIdx.x] = hist[threadIdx.x];
}

// src = (key, s, x): x is the run's end in the first pass, its length afterwards.  dst = (key, s, l) arrays, or (last) rows
// (s, l) of runs.
__global__ __launch_bounds__(256) void rle_scatter_kernel(const int32_t* skey, const int32_t* ss, const int32_t* sx,
                                                          int32_t* dkey, int32_t* ds, int32_t* dl, int32_t* runs,
                                                          const int32_t* tab, const int32_t* nruns, int max_runs, int shift,
                                                          int first, int last) {
  __shared__ int run[256];
  __shared__ int wcnt[4][256];
  const int b = blockIdx.y, nchunk = gridDim.x, kept = min(nruns[2 * b], max_runs);
  if (blockIdx.x * kRleRec >= kept) return;                            // the whole workgroup
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t r0 = (size_t)b * max_runs;
  run[threadIdx.x] = tab[((size_t)b * 256 + threadIdx.x) * nchunk + blockIdx.x];
#pragma unroll
  for (int w = 0; w < 4; ++w) wcnt[w][threadIdx.x] = 0;
  __syncthreads();
  for (int r = 0; r < kRleRec / 256; ++r) {
    const int i = blockIdx.x * kRleRec + r * 256 + threadIdx.x;
    const bool on = i < kept;
    const int k = on ? skey[r0 + i] : 0, d = (k >> shift) & 255;
    // the lanes of this wave that hold a record of the same digit
    unsigned long long m = __ballot(on);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool set = (d >> bit) & 1;
      const unsigned long long bal = __ballot(set);
      m &= set ? bal : ~bal;
    }
    const int rank = __popcll(m & ((1ull << lane) - 1ull));
    if (on && rank == 0) wcnt[wv][d] = __popcll(m);
    __syncthreads();
    int pos = 0;
    if (on) {
      pos = run[d] + rank;
      for (int w = 0; w < wv; ++w) pos += wcnt[w][d];
    }
    __syncthreads();
    run[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
#pragma unroll
    for (int w = 0; w < 4; ++w) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    if (on && (unsigned)pos < (unsigned)kept) {                        // always, with the table the two launches before made
      const int s = ss[r0 + i], x = sx[r0 + i], l = first ? x - s : x;
      if (last) {
        runs[2 * (r0 + pos)] = s;
        runs[2 * (r0 + pos) + 1] = l;
      } else {
        dkey[r0 + pos] = k;
        ds[r0 + pos] = s;
        dl[r0 + pos] = l;
      }
    }
  }
}

static int rle_passes(int cap) { return cap < (1 << 8) ? 1 : cap < (1 << 16) ? 2 : cap < (1 << 24) ? 3 : 4; }

struct rle_layout {
  size_t blk, plane, rec[2], tab, words;   // offsets in words, for all B images
  int nblk, nchunk, passes;
};
static rle_layout rle_plan(long long B, long long HW, int cap, long long max_runs, int order) {
  rle_layout l;
  l.nblk = (int)((HW + 1 + kRlePix - 1) / kRlePix);
  l.nchunk = (int)((max_runs + kRleRec - 1) / kRleRec);
  l.passes = rle_passes(cap);
  size_t w = 0;
  l.blk = w, w += (size_t)B * l.nblk;
  w = (w + 3) & ~(size_t)3;                // the plane at 16 bytes from an aligned workspace: vector loads
  l.plane = w, w += order == 1 ? (size_t)B * HW : 0;
  l.rec[0] = w, w += 3 * (size_t)B * max_runs;
  l.rec[1] = w, w += l.passes > 1 ? 3 * (size_t)B * max_runs : 0;
  l.tab = w, w += (size_t)B * 256 * l.nchunk;
  l.words = w;
  return l;
}

static bool rle_overlap(const void* p, size_t pn, const void* q, size_t qn) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + qn && b < a + pn;
}

}  // namespace dfw

using namespace dfw;

extern "C" size_t dfw_seg_rle_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t cap, int32_t max_runs, int32_t order) {
  if (B < 1 || H < 1 || W < 1 || cap < 1 || max_runs < 1 || (order != 0 && order != 1)) return 0;
  return rle_plan(B, (long long)H * W, cap, max_runs, order).words * 4;
}

extern "C" int dfw_seg_rle_block(int32_t* pixels, int32_t* records) {
  if (!pixels || !records) return DFW_EINVAL;
  *pixels = kRlePix;
  *records = kRleRec;
  return 0;
}

extern "C" int dfw_seg_rle(const dfw_seg_rle_args* a, dfw_stream_t stream) {
  if (!a || !a->ids || !a->runs || !a->run_off || !a->nruns || !a->ws) return DFW_EINVAL;
  if (a->B < 1 || a->H < 1 || a->W < 1 || a->cap < 1 || a->max_runs < 1) return DFW_EINVAL;
  if (a->order != 0 && a->order != 1) return DFW_EINVAL;
  // grid y / z carry B; H * W <= 2^30 keeps every position, HW itself and the padded block count in an int
  if (a->H > 65535 || a->W > 65535 || (long long)a->H * a->W > (1ll << 30) || a->B > 65535) return DFW_ERANGE;
  // rows of runs are addressed in words: B * max_runs * 2 < 2^31, which also bounds max_runs below 2^30 and the digit
  // table, 256 * nchunk <= 2^27 words an image, inside an int
  if ((long long)a->B * a->max_runs * 2 > 0x7fffffffll) return DFW_ERANGE;
  // seg_zero_launch counts run_off's B * (cap + 1) words in an int (so cap + 1 does not wrap either)
  if ((long long)a->B * ((long long)a->cap + 1) > 0x7fffffffll) return DFW_ERANGE;
  if (a->ws_bytes < dfw_seg_rle_workspace_bytes(a->B, a->H, a->W, a->cap, a->max_runs, a->order)) return DFW_EWORKSPACE;
  const size_t idb = (size_t)a->B * a->H * a->W * 4;
  if (rle_overlap(a->ids, idb, a->runs, (size_t)a->B * a->max_runs * 8) ||
      rle_overlap(a->ids, idb, a->run_off, (size_t)a->B * ((size_t)a->cap + 1) * 4) ||
      rle_overlap(a->ids, idb, a->nruns, (size_t)a->B * 8))
    return DFW_EINVAL;
  if (((uintptr_t)a->ids | (uintptr_t)a->runs | (uintptr_t)a->run_off | (uintptr_t)a->nruns | (uintptr_t)a->ws) & 3)
    return DFW_ESHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int B = a->B, H = a->H, W = a->W, cap = a->cap, M = a->max_runs, iHW = H * W;
  const rle_layout l = rle_plan(B, iHW, cap, M, a->order);
  int32_t* ws = (int32_t*)a->ws;
  int32_t* blk = ws + l.blk;
  int32_t* tab = ws + l.tab;
  int32_t* rec[2][3];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 3; ++j) rec[i][j] = ws + l.rec[i] + (size_t)j * B * M;
  if (int e = seg_zero_launch(st, (uint32_t*)a->run_off, B * (cap + 1), nullptr, 0)) return e;
  const int32_t* A = a->ids;
  if (a->order == 1) {
    hipLaunchKernelGGL(rle_transpose_kernel, dim3((W + kRleTT - 1) / kRleTT, (H + kRleTT - 1) / kRleTT, B), dim3(256), 0, st,
                       a->ids, ws + l.plane, H, W);
    DFW_CHECK_LAUNCH();
    A = ws + l.plane;
  }
  hipLaunchKernelGGL(rle_count_kernel, dim3(l.nblk, B), dim3(256), 0, st, A, blk, iHW, cap);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(rle_scan_kernel, dim3(B), dim3(256), 0, st, blk, l.nblk, a->nruns, M);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(rle_emit_kernel, dim3(l.nblk, B), dim3(256), 0, st, A, (const int32_t*)blk, rec[0][0], rec[0][1],
                     rec[0][2], a->run_off, iHW, cap, M);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(rle_scan_kernel, dim3(B), dim3(256), 0, st, a->run_off, cap + 1, (int32_t*)nullptr, 0);
  DFW_CHECK_LAUNCH();
  for (int p = 0; p < l.passes; ++p) {
    int32_t** src = rec[p & 1];
    int32_t** dst = rec[(p & 1) ^ 1];
    hipLaunchKernelGGL(rle_hist_kernel, dim3(l.nchunk, B), dim3(256), 0, st, (const int32_t*)src[0], tab,
                       (const int32_t*)a->nruns, M, 8 * p);
    DFW_CHECK_LAUNCH();
    hipLaunchKernelGGL(rle_scan_kernel, dim3(B), dim3(256), 0, st, tab, 256 * l.nchunk, (int32_t*)nullptr, 0);
    DFW_CHECK_LAUNCH();
    hipLaunchKernelGGL(rle_scatter_kernel, dim3(l.nchunk, B), dim3(256), 0, st, (const int32_t*)src[0],
                       (const int32_t*)src[1], (const int32_t*)src[2], dst[0], dst[1], dst[2], a->runs, (const int32_t*)tab,
                       (const int32_t*)a->nruns, M, 8 * p, p == 0, p == l.passes - 1);
    DFW_CHECK_LAUNCH();
  }
  return 0;
}
