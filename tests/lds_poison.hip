// Test-side LDS poisoner (tests/lds_poison.py builds and loads it; not part of libdiffews_hip.so).
//
// LDS is not cleared between the dispatches of one process: a workgroup starts on what the previous kernel on its CU left
// there.  lds_poison_fill writes ONE word to all 160 KiB of every CU's LDS, lds_poison_probe counts how many words still
// hold it.  Both launch 256-thread workgroups with the full 160 KiB of dynamic LDS, so at most one is resident per CU, and
// each stays for a bounded time (s_memrealtime, 100 MHz, with a hard cap on the iterations) so that a grid of a small
// multiple of the CU count is dealt over all CUs instead of running through the first ones to come free.  No workgroup
// waits for another one and there is no barrier across workgroups: nothing here can hang.  Thread 0 records where its
// workgroup ran (XCC id, hardware id) with an ordinary store.
//
// The three lds_planted_* kernels are wrong on purpose, the way a product kernel could be: each reads LDS it never wrote.
// They read only their own LDS and write only their own output, so they are fault-free; they give the right result on
// zeroed LDS and a different one on poisoned LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

extern __shared__ uint32_t lds[];

namespace {

constexpr int kThreads = 256;
constexpr int kLdsBytes = 160 * 1024;
constexpr int kWords = kLdsBytes / 4;
constexpr int kSpinCap = 4096;               // iterations of the bounded stay, whatever the clock says

__device__ inline uint32_t hw_id() {
  uint32_t v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(v));
  return v;
}

__device__ inline uint32_t xcc_id() {
  uint32_t v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return v;
}

__device__ inline void stay(int ticks) {
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  for (int i = 0; i < kSpinCap; ++i) {
    if ((int64_t)(__builtin_amdgcn_s_memrealtime() - t0) >= (int64_t)ticks) break;
    __builtin_amdgcn_s_sleep(16);
  }
}

__device__ inline void record(uint32_t* where) {
  if (where != nullptr && threadIdx.x == 0) {
    where[2 * blockIdx.x] = xcc_id();
    where[2 * blockIdx.x + 1] = hw_id();
  }
}

__global__ void __launch_bounds__(kThreads) fill_kernel(uint32_t word, int ticks, uint32_t* where) {
  for (int i = threadIdx.x; i < kWords; i += kThreads) lds[i] = word;
  asm volatile("" ::: "memory");        // the stores are the kernel's whole effect: keep them
  __syncthreads();
  record(where);
  stay(ticks);
}

__global__ void __launch_bounds__(kThreads) probe_kernel(uint32_t word, int ticks, uint32_t* counts, uint32_t* where) {
  uint32_t n = 0;
  for (int i = threadIdx.x; i < kWords; i += kThreads) n += lds[i] == word;
  for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d);     // registers only: the probe writes no LDS
  if ((threadIdx.x & 63) == 0) atomicAdd(&counts[blockIdx.x], n);
  record(where);
  stay(ticks);
}

// (a) y = 2 x + 0 * (a word of LDS nobody wrote): exact on any finite leftover, NaN on a NaN or inf one.
__global__ void __launch_bounds__(kThreads) planted_zero_times_kernel(const float* x, float* y, int n) {
  const int i = threadIdx.x;
  if (i < n) y[i] = 2.0f * x[i] + 0.0f * __uint_as_float(lds[i]);
}

// (b) a 16-bin histogram of bytes, counted in LDS bins that are never zeroed.
__global__ void __launch_bounds__(kThreads) planted_histogram_kernel(const uint8_t* v, int32_t* hist, int n) {
  for (int i = threadIdx.x; i < n; i += kThreads) atomicAdd(&lds[v[i] & 15], 1u);
  __syncthreads();
  if (threadIdx.x < 16) hist[threadIdx.x] = (int32_t)lds[threadIdx.x];
}

// (c) a 16 x 64 tile staged through LDS, the rows past the ragged edge skipped, then all 16 staged rows summed per column.
__global__ void __launch_bounds__(kThreads) planted_staging_kernel(const float* x, float* colsum, int rows) {
  for (int i = threadIdx.x; i < 16 * 64; i += kThreads) {
    if (i / 64 < rows) lds[i] = __float_as_uint(x[i]);
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    float acc = 0.0f;
    for (int r = 0; r < 16; ++r) acc += __uint_as_float(lds[r * 64 + threadIdx.x]);
    colsum[threadIdx.x] = acc;
  }
}

template <typename K>
int whole_lds(K kernel) {
  return (int)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
}

}  // namespace

extern "C" {

int lds_poison_fill(uint32_t word, int32_t grid, int32_t ticks, uint32_t* where, hipStream_t stream) {
  if (grid <= 0 || ticks < 0) return -1;
  if (int rc = whole_lds(fill_kernel)) return rc;
  fill_kernel<<<grid, kThreads, kLdsBytes, stream>>>(word, ticks, where);
  return (int)hipGetLastError();
}

// counts[grid] must be zero: every wave adds the matches it saw.
int lds_poison_probe(uint32_t word, int32_t grid, int32_t ticks, uint32_t* counts, uint32_t* where, hipStream_t stream) {
  if (grid <= 0 || ticks < 0 || counts == nullptr) return -1;
  if (int rc = whole_lds(probe_kernel)) return rc;
  probe_kernel<<<grid, kThreads, kLdsBytes, stream>>>(word, ticks, counts, where);
  return (int)hipGetLastError();
}

int32_t lds_poison_words(void) { return kWords; }

int lds_planted_zero_times(const float* x, float* y, int32_t n, hipStream_t stream) {
  if (n < 0 || n > kThreads) return -1;
  planted_zero_times_kernel<<<1, kThreads, 4096, stream>>>(x, y, n);
  return (int)hipGetLastError();
}

int lds_planted_histogram(const uint8_t* v, int32_t* hist, int32_t n, hipStream_t stream) {
  if (n < 0) return -1;
  planted_histogram_kernel<<<1, kThreads, 4096, stream>>>(v, hist, n);
  return (int)hipGetLastError();
}

int lds_planted_staging(const float* x, float* colsum, int32_t rows, hipStream_t stream) {
  if (rows < 0 || rows > 16) return -1;
  planted_staging_kernel<<<1, kThreads, 4096, stream>>>(x, colsum, rows);
  return (int)hipGetLastError();
}

}  // extern "C"
