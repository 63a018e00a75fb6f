// Run compaction and radix sort, shared by the stages behind a label map that are keyed by object (seg_rle.hip,
// seg_match.hip): the maximal runs of equal non-zero keys over a flattened image become (key, start, end) records, and a
// stable LSD radix sort, one key byte per pass, groups the kept records by key.  A stage supplies the SOURCE (where the
// key of a position comes from), the PAYLOAD (what a sort pass moves with the key) and its own tail on the sorted records.
//
//   seg_count_kernel<Src>   per block of kSegPix positions: the starts, key(q) != key(q-1) and key(q) != 0 (key(-1) = 0;
//                           the block's first position reads its predecessor across the border).  Position HW, behind the
//                           image, has key 0 and is always covered: it closes a run that reaches the image's end
//   seg_scan_launch         one workgroup per image: exclusive scan of the block sums in place, (kept, found)
//   seg_emit_kernel<Src>    every position with key(q) != key(q-1) holds c, the number of starts before q.  A start writes
//                           start[c] = q, key[c] = key(q); an end (key(q-1) != 0) writes end[c-1] = q, the run that ends
//                           at q being the most recent start -- so one compaction gives (key, s, e) of every run, runs over
//                           many blocks included.  Ranks >= max_records are skipped; each kept start calls Src::kept
//   seg_sort                per key byte, lowest first, over two record buffers in turn:
//     seg_hist_launch         per chunk of kSegRec records the digit histogram -> tab [digit][chunk]
//     seg_scan_launch         exclusive scan of tab in place, digit-major
//     seg_scatter_kernel<Pay> record i of the chunk goes to tab[digit][chunk] + its rank among the chunk's earlier records
//                             of that digit (chunk_rank, seg_scan.h): ranks come from ballots inside a wave, per-wave
//                             counts across the four waves and a running count across the rounds of 256 -- a fixed order,
//                             no atomic decides a position.  Pay::move writes the record at its destination
//
// "Records kept" is min(n[stride * image], max_records), n being where the first scan put it.  No thread waits for another
// thread or workgroup, every trip count is fixed by the arguments, every cross-workgroup prefix is a launch of its own.
#pragma once
#include "common.h"
#include "seg_scan.h"

namespace dfw {

constexpr int kSegPix = 2048;   // positions per scan block, 8 per thread of 256
constexpr int kSegRec = 2048;   // records per sort chunk, 8 rounds of 256

// The non-template kernels (seg_sort.hip), each defined once; both return the error.
// a [planes][images][n]: exclusive scan in place.  nout (optional, plane 0): nout[stride * image + 0..1] = (min(sum,
// limit), sum).
int seg_scan_launch(hipStream_t st, int32_t* a, int planes, int images, int n, int32_t* nout = nullptr, int stride = 0,
                    int limit = 0);
// tab [image][256][nchunk] = the histogram of byte `shift / 8` of the kept keys of every chunk of key [image][max_records].
int seg_hist_launch(hipStream_t st, const int32_t* key, int32_t* tab, const int32_t* n, int stride, int B, int max_records,
                    int shift);

inline int seg_blocks(long long HW) { return (int)((HW + 1 + kSegPix - 1) / kSegPix); }
inline int seg_chunks(long long max_records) { return (int)((max_records + kSegRec - 1) / kSegRec); }
// Trips of seg_scan_kernel's loop over the n words of one (plane, image): 256 threads scan 4 words each a round and carry
// the sum into the next one.  The grid, (images, planes), adds nothing to it.
inline int seg_scan_rounds(long long n) { return (int)((n + 1023) / 1024); }
// Words of the digit table of one image that seg_sort scans per pass.
inline int seg_table_words(long long max_records) { return 256 * seg_chunks(max_records); }
// Digit passes for keys 0 .. keys - 1.
inline int seg_key_passes(long long keys) {
  return keys <= (1ll << 8) ? 1 : keys <= (1ll << 16) ? 2 : keys <= (1ll << 24) ? 3 : 4;
}

// The starts among a thread's eight positions: v[0] is the predecessor's key.
__device__ __forceinline__ int seg_starts(const int (&v)[9]) {
  int n = 0;
#pragma unroll
  for (int j = 1; j < 9; ++j) n += v[j] != v[j - 1] && v[j] != 0;
  return n;
}

// Src, by value: load9(b, HW, p0, v) gives v[0] = key(p0 - 1), v[1 + j] = key(p0 + j) of image b, key 0 outside [0, HW);
// kept(b, key) is called once for every kept start.
template <class Src>
__global__ __launch_bounds__(256) void seg_count_kernel(Src src, int32_t* blk, int HW) {
  __shared__ int ws[4];
  int v[9];
  src.load9(blockIdx.y, HW, blockIdx.x * kSegPix + threadIdx.x * 8, v);
  int n = seg_starts(v);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) blk[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

template <class Src>
__global__ __launch_bounds__(256) void seg_emit_kernel(Src src, const int32_t* blk, int32_t* key, int32_t* start,
                                                       int32_t* end, int HW, int max_records) {
  __shared__ int wsum[4];
  const int b = blockIdx.y, p0 = blockIdx.x * kSegPix + threadIdx.x * 8;
  int v[9];
  src.load9(b, HW, p0, v);
  int total;
  int c = blk[(size_t)b * gridDim.x + blockIdx.x] + block_scan(seg_starts(v), wsum, &total);   // starts before p0
  const size_t r0 = (size_t)b * max_records;
#pragma unroll
  for (int j = 1; j < 9; ++j) {
    if (v[j] == v[j - 1]) continue;
    const int q = p0 + j - 1;
    if (v[j - 1] != 0 && (unsigned)(c - 1) < (unsigned)max_records) end[r0 + c - 1] = q;   // c >= 1: it started before q
    if (v[j] != 0) {
      if (c < max_records) {
        start[r0 + c] = q;
        key[r0 + c] = v[j];
        src.kept(b, v[j]);
      }
      ++c;
    }
  }
}

// Pay, by value: move(i, pos, key) writes record i of the source buffer, the key included, as record pos of the
// destination; both indices count over all images.
template <class Pay>
__global__ __launch_bounds__(256) void seg_scatter_kernel(const int32_t* skey, Pay pay, const int32_t* tab, const int32_t* n,
                                                          int stride, int max_records, int shift) {
  __shared__ int run[256];
  __shared__ int wcnt[4][256];
  const int b = blockIdx.y, nchunk = gridDim.x, kept = min(n[stride * b], max_records);
  if (blockIdx.x * kSegRec >= kept) return;                            // the whole workgroup
  const size_t r0 = (size_t)b * max_records;
  run[threadIdx.x] = tab[((size_t)b * 256 + threadIdx.x) * nchunk + blockIdx.x];
#pragma unroll
  for (int w = 0; w < 4; ++w) wcnt[w][threadIdx.x] = 0;
  __syncthreads();
  for (int r = 0; r < kSegRec / 256; ++r) {
    const int i = blockIdx.x * kSegRec + r * 256 + threadIdx.x;
    const bool on = i < kept;
    const int k = on ? skey[r0 + i] : 0;
    const int pos = chunk_rank(on, (k >> shift) & 255, run, wcnt);
    // always, with the table the two launches before made
    if (on && (unsigned)pos < (unsigned)kept) pay.move(r0 + i, r0 + pos, k);
  }
}

// The sort of the kept records of key[0] [B][max_records] on the key, `passes` bytes, lowest first.  Pass p reads buffer
// p & 1 and writes the other one through pay(p), the payload of that pass; key[1] is read only where a pass wrote it.
// Returns the error, and in *cur (optional) the buffer that holds the result.
template <class MakePay>
int seg_sort(hipStream_t st, const int32_t* const (&key)[2], int32_t* tab, const int32_t* n, int stride, int B,
             int max_records, int passes, int* cur, MakePay pay) {
  const int nchunk = seg_chunks(max_records);
  for (int p = 0; p < passes; ++p) {
    if (int e = seg_hist_launch(st, key[p & 1], tab, n, stride, B, max_records, 8 * p)) return e;
    if (int e = seg_scan_launch(st, tab, 1, B, seg_table_words(max_records))) return e;
    auto pl = pay(p);
    hipLaunchKernelGGL(seg_scatter_kernel<decltype(pl)>, dim3(nchunk, B), dim3(256), 0, st, key[p & 1], pl,
                       (const int32_t*)tab, n, stride, max_records, 8 * p);
    DFW_CHECK_LAUNCH();
  }
  if (cur) *cur = passes & 1;
  return 0;
}

}  // namespace dfw
