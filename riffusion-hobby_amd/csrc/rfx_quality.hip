// rfx_quality.hip - the per-row spectral sums of rfx_spectral_error (N = 2: sum (a - m)^2, sum m^2) and rfx_spectral_loss (N = 3:
// those and sum | ln max(a, f) - ln max(m, f) |; include/rfx.h) over two magnitude tensors in the plan's slot layout, every bin of
// every frame once, in double.  The arithmetic and the shape of the reduction are rfx_quality_core.h (shared with the emulators
// tests/emu/rfx_quality_emu.cpp and tests/emu/rfx_spec_loss_emu.cpp): what the kernels add is the barrier between the tree's levels.
// One tree, one partial kernel and one combine kernel, templates of N: the N = 2 instantiation holds 16 bytes per thread in LDS.
#include <hip/hip_runtime.h>
#include "rfx_kernels.h"
#include "rfx_quality_core.h"

namespace rfx {
namespace {

// the halving tree over the workgroup's kQualThreads sums; the result is s[0] (valid in thread 0 after the last barrier)
template <int N>
__device__ __forceinline__ void qual_tree(SpecSums<N>* s, int tid) {
  __syncthreads();
#pragma unroll
  for (int stride = kQualThreads / 2; stride > 0; stride >>= 1) {
    if (tid < stride) qual_tree_step(s, tid, stride);
    __syncthreads();
  }
}

// workgroup (row, chunk) = blockIdx.x: frames [kQualFrames chunk, ...) of row `row` -> partials[row * chunks + chunk]
template <int N, bool PLAIN, bool LOG>
__global__ __launch_bounds__(kQualThreads) void qual_partial_kernel(const float* __restrict__ a, const float* __restrict__ m,
                                                                     SpecSums<N>* __restrict__ partials, int T, int fs, int n_stft, int chunks,
                                                                     float floor) {
  __shared__ SpecSums<N> s[kQualThreads];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x / (unsigned)chunks;
  const int chunk = (int)(blockIdx.x - row * (unsigned)chunks);
  const int f0 = chunk * kQualFrames, f1 = f0 + kQualFrames < T ? f0 + kQualFrames : T;
  const size_t row_at = row * (size_t)T * (size_t)fs;
  s[tid] = qual_walk<N, PLAIN, LOG>(a + row_at, m + row_at, f0, f1, fs, n_stft, floor, tid);
  qual_tree(s, tid);
  if (tid == 0) partials[blockIdx.x] = s[0];
}

// workgroup `row`: the row's partials -> sums[N row .. N row + N - 1]
template <int N>
__global__ __launch_bounds__(kQualThreads) void qual_combine_kernel(const SpecSums<N>* __restrict__ partials, double* __restrict__ sums, int chunks) {
  __shared__ SpecSums<N> s[kQualThreads];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  s[tid] = qual_combine_partial(partials + row * (size_t)chunks, chunks, tid);
  qual_tree(s, tid);
  if (tid == 0) {
    sums[N * row] = s[0].num;
    sums[N * row + 1] = s[0].den;
    if constexpr (N == 3) sums[N * row + 2] = s[0].lsum;
  }
}

template <int N, bool LOG>
hipError_t sums_launch(const float* a, const float* m, int rows, int T, int fs, int n_stft, bool plain, float floor, void* partials, double* sums,
                       hipStream_t s) {
  const int chunks = qual_chunks(T);
  const dim3 grid((unsigned)((size_t)rows * chunks)), block(kQualThreads);
  SpecSums<N>* p = static_cast<SpecSums<N>*>(partials);
  if (plain) hipLaunchKernelGGL((qual_partial_kernel<N, true, LOG>), grid, block, 0, s, a, m, p, T, fs, n_stft, chunks, floor);
  else hipLaunchKernelGGL((qual_partial_kernel<N, false, LOG>), grid, block, 0, s, a, m, p, T, fs, n_stft, chunks, floor);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(qual_combine_kernel<N>, dim3((unsigned)rows), block, 0, s, p, sums, chunks);
  return hipGetLastError();
}

}  // namespace

size_t qual_partials_bytes(int rows, int T, int nsums) { return (size_t)rows * qual_chunks(T) * nsums * sizeof(double); }

hipError_t launch_spectral_sums(const float* a, const float* m, int rows, int T, int fs, int n_stft, bool plain, int nsums, float floor, void* partials,
                                double* sums, hipStream_t s) {
  if (nsums == 2) return sums_launch<2, false>(a, m, rows, T, fs, n_stft, plain, 0.f, partials, sums, s);
  return floor > 0.f ? sums_launch<3, true>(a, m, rows, T, fs, n_stft, plain, floor, partials, sums, s)
                     : sums_launch<3, false>(a, m, rows, T, fs, n_stft, plain, floor, partials, sums, s);
}

}  // namespace rfx
