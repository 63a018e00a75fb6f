// Matching of predicted objects to ground-truth objects (objects.match_objects): two id maps int32 [B][H][W] -> per image
// the overlap of every (predicted, ground-truth) pair that shares a pixel, the areas, the one-to-one matching on IoU and the
// panoptic-quality counts per class.  All integers: the result depends on no order of execution.
//
// p(q) = pid when 1 <= pid <= capP, else 0; g(q) likewise with capG.  A pixel has w(q) = (p, g) unless skip[q] == 255, then
// w(q) = (0, 0).  Position is q = y * W + x.  A record is a maximal interval of positions with one equal w != (0, 0); as in
// seg_rle it does not stop at a row's end.  key = p * (capG + 1) + g.  A pair is a distinct key over the kept records, inter
// the sum of the record lengths of that key.  Pairs with g = 0 or p = 0 are kept: row sums are areaP[p], the counted pixels
// of p, column sums areaG[g]; neither depends on stats, both respect skip.  union = areaP[p] + areaG[g] - inter.  p and g
// (both > 0) MATCH when their classes are equal, the class is in 1..nlabels and inter * den > num * union in 64-bit
// integers, strictly; the threshold num / den is at least 1/2, so each object has at most one partner and no assignment
// problem arises.  An object with area 0 (all its pixels skipped, or its id above cap) is absent: neither FP nor FN.
//
// Truncation: of the records the first max_records in ascending start are kept, of the pairs the first max_pairs in
// ascending key; every output is what the definition gives on the kept records and pairs, and n = (pairs kept, pairs found,
// records kept, records found) shows it.
//
// pids = [[1,1,0],[2,1,1]], gids = [[1,1,1],[0,2,2]], caps 2 and 2, threshold 1/2: records (1,1)x2 (0,1)x1 (2,0)x1 (1,2)x2;
// pairs (0,1,1) (1,1,2) (1,2,2) (2,0,1); pair_off = [0,1,3,4]; areaP = [1,4,1], areaG = [1,3,2]; IoU(1,1) = 2/5, IoU(1,2) =
// 2/4, which is not above 1/2: no match, pq[1] = (0, 2, 2, 0).
//
// The workspace is, for all B images, blk [nblk] | key, start, end [max_records] | key, length [max_records] | tab
// [256][nchunk] | heads, lengths [nhead] | first, last [max_pairs], every word of it written before it is read (the caller
// initialises nothing).  nblk = seg_blocks(HW), nchunk = seg_chunks(max_records), nhead = (max_records + 1) / kSegRec
// rounded up: the position behind the last record is covered, as the one behind the image is one step earlier.  The
// compaction and the sort are the shared ones of seg_sort.h, which explains them; this file supplies the source
// (match_maps: the key of two id maps and skip), the payload (match_pay) and the tail on the sorted records.  Launches, a
// number fixed by the arguments,
//
//     14 + 3 * passes,   passes = the bytes (capP + 1) * (capG + 1) - 1 needs (1..4),
//
// with no host readback in between:
//
//   0-3   seg_zero_launch               pair_off and pq | area | match | gmatch (a library kernel, no memset node)
//   4     seg_count_kernel<match_maps>  the record starts per block of kSegPix positions (16-byte loads of both maps,
//                                       8-byte loads of skip)
//   5     seg_scan_launch               exclusive scan of the block sums in place, n[2..3]
//   6     seg_emit_kernel<match_maps>   (key, start, end) of every kept record
//   7+    seg_sort                      per key byte hist, scan, seg_scatter_kernel<match_pay>.  The first pass turns (start,
//                                       end) into a length
//   then  match_heads_kernel     per chunk of sorted records: the heads, key[i] != key[i-1], and the sum of the lengths
//         seg_scan_launch        both, in one launch: n[0..1]
//         match_pairs_kernel     a head of rank c writes pairs[c] = (p, g, .), first[c] = the lengths before it, and counts
//                                itself into pair_off[p]; a head, or the position behind the last record, writes last[c-1]
//         match_inter_kernel     one thread per kept pair: inter = last - first into pairs, and into areaP[p] and areaG[g]
//                                (integer atomics: sums, never positions)
//         seg_scan_launch        pair_off: the exclusive scan of the counts is the offset table
//         match_rule_kernel      one thread per kept pair applies the match rule: match[p], gmatch[g] (the partner is
//                                unique: no race), TP and S into pq (integer atomics)
//         match_rest_kernel      one thread per object: present and without a partner -> FP or FN of its class
//
// Termination: no thread waits for another thread or workgroup; every loop has a trip count fixed by the arguments, every
// cross-workgroup prefix is a scan in a launch of its own.  Any grid is correct at any residency.
#include "seg_args.h"
#include "seg_sort.h"

namespace dfw {

// The two id maps and skip (optional), [B][HW]: the key of a position.
struct match_maps {
  const int32_t* P;
  const int32_t* G;
  const uint8_t* S;
  int capP, capG;

  __device__ __forceinline__ int key(int pid, int gid, int sk) const {
    const int p = (pid >= 1 && pid <= capP) ? pid : 0, g = (gid >= 1 && gid <= capG) ? gid : 0;
    return sk == 255 ? 0 : p * (capG + 1) + g;
  }
  __device__ __forceinline__ void load9(int b, int HW, int p0, int (&v)[9]) const {
    const int32_t* p = P + (size_t)b * HW;
    const int32_t* g = G + (size_t)b * HW;
    const uint8_t* sk = S ? S + (size_t)b * HW : nullptr;
    v[0] = (p0 >= 1 && p0 - 1 < HW) ? key(p[p0 - 1], g[p0 - 1], sk ? sk[p0 - 1] : 0) : 0;
    if (p0 + 8 <= HW && (((uintptr_t)(p + p0) | (uintptr_t)(g + p0)) & 15) == 0 && (!sk || ((uintptr_t)(sk + p0) & 7) == 0)) {
      const i32x4 a0 = *(const i32x4*)(p + p0), a1 = *(const i32x4*)(p + p0 + 4);
      const i32x4 b0 = *(const i32x4*)(g + p0), b1 = *(const i32x4*)(g + p0 + 4);
      const unsigned long long s = sk ? *(const unsigned long long*)(sk + p0) : 0ull;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[1 + j] = key(a0[j], b0[j], (int)((s >> (8 * j)) & 255));
        v[5 + j] = key(a1[j], b1[j], (int)((s >> (8 * j + 32)) & 255));
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[1 + j] = p0 + j < HW ? key(p[p0 + j], g[p0 + j], sk ? sk[p0 + j] : 0) : 0;
    }
  }
  __device__ __forceinline__ void kept(int, int) const {}
};

// src = (key, s, x): with `first`, s and x are the record's start and end; afterwards sx is its length and ss unused.
struct match_pay {
  const int32_t *ss, *sx;
  int32_t *dkey, *dl;
  int first;

  __device__ __forceinline__ void move(size_t i, size_t pos, int key) const {
    dkey[pos] = key;
    dl[pos] = first ? sx[i] - ss[i] : sx[i];
  }
};

// k[0] = key[i0 - 1] (-1 in front of the first record: never a key), k[1 + j] = key[i0 + j], l[j] = len[i0 + j], for the
// records below kept; behind them the key is -1 and the length 0, so that position `kept` reads as a head that only ends.
__device__ __forceinline__ void match_load_sorted(const int32_t* key, const int32_t* len, int i0, int kept, int (&k)[9],
                                                  int (&l)[8]) {
  k[0] = (i0 >= 1 && i0 - 1 < kept) ? key[i0 - 1] : -1;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bool on = i0 + j < kept;
    k[1 + j] = on ? key[i0 + j] : -1;
    l[j] = on ? len[i0 + j] : 0;
  }
}

// h = the heads among a thread's eight sorted records, s = the sum of their lengths.
__device__ __forceinline__ void match_heads(const int (&k)[9], const int (&l)[8], int i0, int kept, int& h, int& s) {
  h = s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    h += i0 + j < kept && k[1 + j] != k[j];
    s += l[j];
  }
}

// hd [2][image][nhead]: the heads and the sum of the lengths of each chunk of kSegRec sorted records.
__global__ __launch_bounds__(256) void match_heads_kernel(const int32_t* key, const int32_t* len, int32_t* hd,
                                                          const int32_t* n, int max_records) {
  __shared__ int ws[2][4];
  const int b = blockIdx.y, B = gridDim.y, kept = min(n[4 * b + 2], max_records), i0 = blockIdx.x * kSegRec + threadIdx.x * 8;
  const size_t r0 = (size_t)b * max_records;
  int k[9], l[8], h, s;
  match_load_sorted(key + r0, len + r0, i0, kept, k, l);
  match_heads(k, l, i0, kept, h, s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    h += __shfl_xor(h, o, 64);
    s += __shfl_xor(s, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    ws[0][threadIdx.x >> 6] = h;
    ws[1][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < 2)
    hd[((size_t)threadIdx.x * B + b) * gridDim.x + blockIdx.x] =
        ws[threadIdx.x][0] + ws[threadIdx.x][1] + ws[threadIdx.x][2] + ws[threadIdx.x][3];
}

__global__ __launch_bounds__(256) void match_pairs_kernel(const int32_t* key, const int32_t* len, const int32_t* hd,
                                                          int32_t* pairs, int32_t* pfirst, int32_t* plast, int32_t* pair_off,
                                                          const int32_t* n, int max_records, int max_pairs, int capP,
                                                          int capG) {
  __shared__ int wsum[4];
  const int b = blockIdx.y, B = gridDim.y, kept = min(n[4 * b + 2], max_records), i0 = blockIdx.x * kSegRec + threadIdx.x * 8;
  const size_t r0 = (size_t)b * max_records, q0 = (size_t)b * max_pairs;
  int k[9], l[8], h, s;
  match_load_sorted(key + r0, len + r0, i0, kept, k, l);
  match_heads(k, l, i0, kept, h, s);
  int total;
  int c = hd[(size_t)b * gridDim.x + blockIdx.x] + block_scan(h, wsum, &total);                  // heads before i0
  int at = hd[((size_t)B + b) * gridDim.x + blockIdx.x] + block_scan(s, wsum, &total);           // lengths before i0
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = i0 + j;
    if (i <= kept && k[1 + j] != k[j]) {                               // a head, or the position behind the last record
      if ((unsigned)(c - 1) < (unsigned)max_pairs) plast[q0 + c - 1] = at;
      if (i < kept) {
        if (c < max_pairs) {
          const int p = k[1 + j] / (capG + 1), g = k[1 + j] - p * (capG + 1);
          pairs[3 * (q0 + c)] = p;
          pairs[3 * (q0 + c) + 1] = g;
          pfirst[q0 + c] = at;
          atomicAdd(&pair_off[(size_t)b * (capP + 2) + p], 1);
        }
        ++c;
      }
    }
    at += l[j];
  }
}

__global__ __launch_bounds__(256) void match_inter_kernel(int32_t* pairs, const int32_t* pfirst, const int32_t* plast,
                                                          int32_t* area, const int32_t* n, int max_pairs, int capP, int capG) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= min(n[4 * b], max_pairs)) return;
  const size_t q = (size_t)b * max_pairs + c;
  const int inter = plast[q] - pfirst[q], p = pairs[3 * q], g = pairs[3 * q + 1];
  pairs[3 * q + 2] = inter;
  int32_t* ar = area + (size_t)b * (capP + capG + 2);
  atomicAdd(&ar[p], inter);
  atomicAdd(&ar[capP + 1 + g], inter);
}

struct match_rule {
  const int32_t* pstats;   // optional [B][capP][8]
  const int32_t* gstats;   // optional [B][capG][8]
  int capP, capG, nlabels, num, den;
};

// The class of object k (1..cap) of image b: column 0 of its stats row, 1 without a table.
__device__ __forceinline__ int match_class(const int32_t* stats, int b, int cap, int k) {
  return stats ? stats[((size_t)b * cap + k - 1) * 8] : 1;
}

__global__ __launch_bounds__(256) void match_rule_kernel(const int32_t* pairs, const int32_t* area, match_rule r,
                                                         int32_t* match, int32_t* gmatch, unsigned long long* pq,
                                                         const int32_t* n, int max_pairs) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= min(n[4 * b], max_pairs)) return;
  const size_t q = (size_t)b * max_pairs + c;
  const int p = pairs[3 * q], g = pairs[3 * q + 1], inter = pairs[3 * q + 2];
  if (p == 0 || g == 0) return;
  const int cls = match_class(r.pstats, b, r.capP, p);
  if (cls != match_class(r.gstats, b, r.capG, g) || cls < 1 || cls > r.nlabels) return;
  const int32_t* ar = area + (size_t)b * (r.capP + r.capG + 2);
  const long long uni = (long long)ar[p] + ar[r.capP + 1 + g] - inter;
  if ((long long)inter * r.den <= (long long)r.num * uni) return;
  int32_t* m = match + ((size_t)b * r.capP + p - 1) * 3;
  m[0] = g;
  m[1] = inter;
  m[2] = (int)uni;
  gmatch[(size_t)b * r.capG + g - 1] = p;
  unsigned long long* row = pq + ((size_t)b * (r.nlabels + 1) + cls) * 4;
  atomicAdd(&row[0], 1ull);
  atomicAdd(&row[3], ((unsigned long long)inter << 32) / (unsigned long long)uni);
}

__global__ __launch_bounds__(256) void match_rest_kernel(const int32_t* area, match_rule r, const int32_t* match,
                                                         const int32_t* gmatch, unsigned long long* pq) {
  const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= r.capP + r.capG) return;
  const int32_t* ar = area + (size_t)b * (r.capP + r.capG + 2);
  const bool pred = t < r.capP;
  const int k = pred ? t + 1 : t - r.capP + 1;
  const int a = pred ? ar[k] : ar[r.capP + 1 + k];
  const int partner = pred ? match[((size_t)b * r.capP + k - 1) * 3] : gmatch[(size_t)b * r.capG + k - 1];
  if (a == 0 || partner != 0) return;
  const int cls = pred ? match_class(r.pstats, b, r.capP, k) : match_class(r.gstats, b, r.capG, k);
  if (cls < 1 || cls > r.nlabels) return;
  atomicAdd(&pq[((size_t)b * (r.nlabels + 1) + cls) * 4 + (pred ? 1 : 2)], 1ull);
}

// Words of pair_off per image, the scan behind match_inter_kernel.
inline int match_offsets(long long capP) { return (int)(capP + 2); }

struct match_layout {
  size_t blk, rec[2], tab, hd, pfirst, plast, words;   // offsets in words, for all B images
  int nblk, nhead;
};
static match_layout match_plan(long long B, long long HW, long long max_records, long long max_pairs) {
  match_layout l;
  l.nblk = seg_blocks(HW);
  l.nhead = seg_chunks(max_records + 1);
  size_t w = 0;
  l.blk = w, w += (size_t)B * l.nblk;
  l.rec[0] = w, w += 3 * (size_t)B * max_records;
  l.rec[1] = w, w += 2 * (size_t)B * max_records;
  l.tab = w, w += (size_t)B * 256 * seg_chunks(max_records);
  l.hd = w, w += 2 * (size_t)B * l.nhead;
  l.pfirst = w, w += (size_t)B * max_pairs;
  l.plast = w, w += (size_t)B * max_pairs;
  l.words = w;
  return l;
}

// Digit passes of the sort: the bytes the highest key needs.
inline int match_passes(long long capP, long long capG) { return seg_key_passes((capP + 1) * (capG + 1)); }

// The sizes dfw_seg_match refuses, and its workspace query with it: DFW_EINVAL before DFW_ERANGE.
static int match_size_error(long long B, long long H, long long W, long long capP, long long capG, long long max_records,
                            long long max_pairs) {
  if (B < 1 || H < 1 || W < 1 || capP < 1 || capG < 1 || max_records < 1 || max_pairs < 1) return DFW_EINVAL;
  // H * W <= 2^30 also keeps every sum of lengths in an int, and inter * den below 2^46
  if (int e = seg_map_size_error(B, H, W)) return e;
  if ((capP + 1) * (capG + 1) - 1 > 0x7fffffffll) return DFW_ERANGE;   // the highest key is an int; capP + capG + 2 too, then
  // word counts the kernels and seg_zero_launch hold in an int: rows of pairs and match, the tables, the records
  if (B * max_pairs * 3 > 0x7fffffffll || B * max_records > 0x7fffffffll || B * capP * 3 > 0x7fffffffll ||
      B * (capP + capG + 2) > 0x7fffffffll)
    return DFW_ERANGE;
  return 0;
}

}  // namespace dfw

using namespace dfw;

extern "C" size_t dfw_seg_match_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t capP, int32_t capG,
                                                int32_t max_records, int32_t max_pairs) {
  if (match_size_error(B, H, W, capP, capG, max_records, max_pairs)) return 0;
  return match_plan(B, (long long)H * W, max_records, max_pairs).words * 4;
}

extern "C" int dfw_seg_match_block(int32_t* pixels, int32_t* records) {
  if (!pixels || !records) return DFW_EINVAL;
  *pixels = kSegPix;
  *records = kSegRec;
  return 0;
}

extern "C" int dfw_seg_match_rounds(int32_t B, int32_t H, int32_t W, int32_t capP, int32_t capG, int32_t max_records,
                                    int32_t max_pairs, dfw_seg_sort_rounds* out) {
  if (!out) return DFW_EINVAL;
  if (int e = match_size_error(B, H, W, capP, capG, max_records, max_pairs)) return e;
  const match_layout l = match_plan(B, (long long)H * W, max_records, max_pairs);
  out->blocks = l.nblk;
  out->block_scan = seg_scan_rounds(l.nblk);
  out->passes = match_passes(capP, capG);
  out->table_scan = seg_scan_rounds(seg_table_words(max_records));
  out->offsets_scan = seg_scan_rounds(match_offsets(capP));
  out->heads_scan = seg_scan_rounds(l.nhead);
  return 0;
}

extern "C" int dfw_seg_match(const dfw_seg_match_args* a, dfw_stream_t stream) {
  if (!a || !a->pids || !a->gids || !a->pairs || !a->pair_off || !a->area || !a->match || !a->gmatch || !a->pq || !a->n ||
      !a->ws)
    return DFW_EINVAL;
  if (a->num < 1 || a->num > a->den || a->den > 65535 || 2 * (long long)a->num < a->den) return DFW_EINVAL;
  if (a->nlabels < 1 || a->nlabels > 254) return DFW_EINVAL;
  if (int e = match_size_error(a->B, a->H, a->W, a->capP, a->capG, a->max_records, a->max_pairs)) return e;
  const size_t need = dfw_seg_match_workspace_bytes(a->B, a->H, a->W, a->capP, a->capG, a->max_records, a->max_pairs);
  if (a->ws_bytes < need) return DFW_EWORKSPACE;
  const size_t Bs = (size_t)a->B, px = Bs * a->H * a->W, cP = (size_t)a->capP, cG = (size_t)a->capG;
  const seg_buf bufs[] = {seg_in(a->pids, px * 4, 4),
                          seg_in(a->gids, px * 4, 4),
                          seg_in(a->pstats, Bs * cP * 32, 4),
                          seg_in(a->gstats, Bs * cG * 32, 4),
                          seg_in(a->skip, px),
                          seg_out(a->pairs, Bs * a->max_pairs * 12, 4),
                          seg_out(a->pair_off, Bs * (cP + 2) * 4, 4),
                          seg_out(a->area, Bs * (cP + cG + 2) * 4, 4),
                          seg_out(a->match, Bs * cP * 12, 4),
                          seg_out(a->gmatch, Bs * cG * 4, 4),
                          seg_out(a->pq, Bs * ((size_t)a->nlabels + 1) * 32, 8),
                          seg_out(a->n, Bs * 16, 4),
                          seg_out(a->ws, need, 4)};
  if (int e = seg_check_buffers(bufs)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int nB = a->B, iHW = a->H * a->W, capP = a->capP, capG = a->capG, M = a->max_records, MP = a->max_pairs;
  const match_layout l = match_plan(nB, iHW, M, MP);
  const int passes = match_passes(capP, capG);
  int32_t* ws = (int32_t*)a->ws;
  int32_t* blk = ws + l.blk;
  int32_t* hd = ws + l.hd;
  int32_t* rec[2][3];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 3; ++j) rec[i][j] = ws + l.rec[i] + (size_t)j * nB * M;   // rec[1][2] is never used
  const match_maps maps = {a->pids, a->gids, a->skip, capP, capG};
  const match_rule rule = {a->pstats, a->gstats, capP, capG, a->nlabels, a->num, a->den};
  if (int e = seg_zero_launch(st, (uint32_t*)a->pair_off, nB * (capP + 2), a->pq, nB * (a->nlabels + 1) * 4)) return e;
  if (int e = seg_zero_launch(st, (uint32_t*)a->area, nB * (capP + capG + 2), nullptr, 0)) return e;
  if (int e = seg_zero_launch(st, (uint32_t*)a->match, nB * capP * 3, nullptr, 0)) return e;
  if (int e = seg_zero_launch(st, (uint32_t*)a->gmatch, nB * capG, nullptr, 0)) return e;
  hipLaunchKernelGGL(seg_count_kernel<match_maps>, dim3(l.nblk, nB), dim3(256), 0, st, maps, blk, iHW);
  DFW_CHECK_LAUNCH();
  if (int e = seg_scan_launch(st, blk, 1, nB, l.nblk, a->n + 2, 4, M)) return e;
  hipLaunchKernelGGL(seg_emit_kernel<match_maps>, dim3(l.nblk, nB), dim3(256), 0, st, maps, (const int32_t*)blk, rec[0][0],
                     rec[0][1], rec[0][2], iHW, M);
  DFW_CHECK_LAUNCH();
  const int32_t* const key[2] = {rec[0][0], rec[1][0]};
  int cur;
  // the first pass reads (key, start, end) and every pass writes (key, length) into arrays 0 and 1 of the other buffer
  if (int e = seg_sort(st, key, ws + l.tab, a->n + 2, 4, nB, M, passes, &cur, [&](int p) {
        int32_t** s = rec[p & 1];
        int32_t** d = rec[(p & 1) ^ 1];
        return match_pay{s[1], p == 0 ? s[2] : s[1], d[0], d[1], p == 0};
      }))
    return e;
  const int32_t* skey = rec[cur][0];
  const int32_t* slen = rec[cur][1];
  int32_t* pfirst = ws + l.pfirst;
  int32_t* plast = ws + l.plast;
  hipLaunchKernelGGL(match_heads_kernel, dim3(l.nhead, nB), dim3(256), 0, st, skey, slen, hd, (const int32_t*)a->n, M);
  DFW_CHECK_LAUNCH();
  if (int e = seg_scan_launch(st, hd, 2, nB, l.nhead, a->n, 4, MP)) return e;
  hipLaunchKernelGGL(match_pairs_kernel, dim3(l.nhead, nB), dim3(256), 0, st, skey, slen, (const int32_t*)hd, a->pairs, pfirst,
                     plast, a->pair_off, (const int32_t*)a->n, M, MP, capP, capG);
  DFW_CHECK_LAUNCH();
  const dim3 pgrid((MP + 255) / 256, nB);
  hipLaunchKernelGGL(match_inter_kernel, pgrid, dim3(256), 0, st, a->pairs, (const int32_t*)pfirst, (const int32_t*)plast,
                     a->area, (const int32_t*)a->n, MP, capP, capG);
  DFW_CHECK_LAUNCH();
  if (int e = seg_scan_launch(st, a->pair_off, 1, nB, match_offsets(capP))) return e;
  hipLaunchKernelGGL(match_rule_kernel, pgrid, dim3(256), 0, st, (const int32_t*)a->pairs, (const int32_t*)a->area, rule,
                     a->match, a->gmatch, (unsigned long long*)a->pq, (const int32_t*)a->n, MP);
  DFW_CHECK_LAUNCH();
  hipLaunchKernelGGL(match_rest_kernel, dim3((capP + capG + 255) / 256, nB), dim3(256), 0, st, (const int32_t*)a->area, rule,
                     (const int32_t*)a->match, (const int32_t*)a->gmatch, (unsigned long long*)a->pq);
  DFW_CHECK_LAUNCH();
  return 0;
}
