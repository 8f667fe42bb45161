// rfx_quality.hip - spectral error of a decode (rfx_spectral_error, include/rfx.h): per row the two double sums
// sum (a - m)^2 and sum m^2 over two magnitude tensors in the plan's slot layout, every bin of every frame once.
// The arithmetic and the shape of the reduction are rfx_quality_core.h (shared with tests/emu/rfx_quality_emu.cpp): what
// the kernels add is the barrier between the tree's levels.  rfx_spectral_loss's three sums are a variant of the same reduction
// (rfx_spec_loss_core.h), below the two kernels of the pair.
#include <hip/hip_runtime.h>
#include "rfx_kernels.h"
#include "rfx_quality_core.h"
#include "rfx_spec_loss_core.h"

namespace rfx {
namespace {

// the halving tree over the workgroup's kQualThreads pairs; the result is s[0] (valid in thread 0 after the last barrier)
__device__ __forceinline__ void qual_tree(QualSums* s, int tid) {
  __syncthreads();
#pragma unroll
  for (int stride = kQualThreads / 2; stride > 0; stride >>= 1) {
    if (tid < stride) qual_tree_step(s, tid, stride);
    __syncthreads();
  }
}

// workgroup (row, chunk) = blockIdx.x: frames [kQualFrames chunk, ...) of row `row` -> partials[row * chunks + chunk]
template <bool PLAIN>
__global__ __launch_bounds__(kQualThreads) void qual_partial_kernel(const float* __restrict__ a, const float* __restrict__ m,
                                                                     QualSums* __restrict__ partials, int T, int fs, int n_stft, int chunks) {
  __shared__ QualSums s[kQualThreads];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x / (unsigned)chunks;
  const int chunk = (int)(blockIdx.x - row * (unsigned)chunks);
  const int f0 = chunk * kQualFrames, f1 = f0 + kQualFrames < T ? f0 + kQualFrames : T;
  const size_t row_at = row * (size_t)T * (size_t)fs;
  s[tid] = qual_thread_partial<PLAIN>(a + row_at, m + row_at, f0, f1, fs, n_stft, tid);
  qual_tree(s, tid);
  if (tid == 0) partials[blockIdx.x] = s[0];
}

// workgroup `row`: the row's partials -> sums[2 row], sums[2 row + 1]
__global__ __launch_bounds__(kQualThreads) void qual_combine_kernel(const QualSums* __restrict__ partials, double* __restrict__ sums, int chunks) {
  __shared__ QualSums s[kQualThreads];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  s[tid] = qual_combine_partial(partials + row * (size_t)chunks, chunks, tid);
  qual_tree(s, tid);
  if (tid == 0) {
    sums[2 * row] = s[0].num;
    sums[2 * row + 1] = s[0].den;
  }
}

// ---- the same reduction carrying a third sum (rfx_spectral_loss; rfx_spec_loss_core.h): sum | ln max(a, f) - ln max(m, f) |.  A
// variant of its own - the two kernels above are not touched, rfx_spectral_error's bits are pinned - that walks the same chunks in the
// same per-thread order and folds with the same tree, so its first two sums are the two above bit for bit.  LOG == false: f == 0, no
// logarithm is evaluated and the third sum is 0.
__device__ __forceinline__ void spec_loss_tree(SpecLossSums* s, int tid) {
  __syncthreads();
#pragma unroll
  for (int stride = kQualThreads / 2; stride > 0; stride >>= 1) {
    if (tid < stride) spec_loss_tree_step(s, tid, stride);
    __syncthreads();
  }
}

template <bool PLAIN, bool LOG>
__global__ __launch_bounds__(kQualThreads) void spec_loss_partial_kernel(const float* __restrict__ a, const float* __restrict__ m,
                                                                          SpecLossSums* __restrict__ partials, int T, int fs, int n_stft, int chunks,
                                                                          float floor) {
  __shared__ SpecLossSums s[kQualThreads];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x / (unsigned)chunks;
  const int chunk = (int)(blockIdx.x - row * (unsigned)chunks);
  const int f0 = chunk * kQualFrames, f1 = f0 + kQualFrames < T ? f0 + kQualFrames : T;
  const size_t row_at = row * (size_t)T * (size_t)fs;
  s[tid] = spec_loss_thread_partial<PLAIN, LOG>(a + row_at, m + row_at, f0, f1, fs, n_stft, floor, tid);
  spec_loss_tree(s, tid);
  if (tid == 0) partials[blockIdx.x] = s[0];
}

// workgroup `row`: the row's partials -> sums[3 row .. 3 row + 2]
__global__ __launch_bounds__(kQualThreads) void spec_loss_combine_kernel(const SpecLossSums* __restrict__ partials, double* __restrict__ sums, int chunks) {
  __shared__ SpecLossSums s[kQualThreads];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  s[tid] = spec_loss_combine_partial(partials + row * (size_t)chunks, chunks, tid);
  spec_loss_tree(s, tid);
  if (tid == 0) {
    sums[3 * row] = s[0].num;
    sums[3 * row + 1] = s[0].den;
    sums[3 * row + 2] = s[0].lsum;
  }
}

}  // namespace

size_t qual_partials_bytes(int rows, int T) { return (size_t)rows * qual_chunks(T) * sizeof(QualSums); }

hipError_t launch_spectral_sums(const float* a, const float* m, int rows, int T, int fs, int n_stft, bool plain, void* partials, double* sums,
                                hipStream_t s) {
  const int chunks = qual_chunks(T);
  const dim3 grid((unsigned)((size_t)rows * chunks)), block(kQualThreads);
  QualSums* p = static_cast<QualSums*>(partials);
  if (plain) hipLaunchKernelGGL(qual_partial_kernel<true>, grid, block, 0, s, a, m, p, T, fs, n_stft, chunks);
  else hipLaunchKernelGGL(qual_partial_kernel<false>, grid, block, 0, s, a, m, p, T, fs, n_stft, chunks);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(qual_combine_kernel, dim3((unsigned)rows), block, 0, s, p, sums, chunks);
  return hipGetLastError();
}

size_t spec_loss_partials_bytes(int rows, int T) { return (size_t)rows * qual_chunks(T) * sizeof(SpecLossSums); }

hipError_t launch_spec_loss_sums(const float* a, const float* m, int rows, int T, int fs, int n_stft, bool plain, float floor, void* partials, double* sums,
                                 hipStream_t s) {
  const int chunks = qual_chunks(T);
  const dim3 grid((unsigned)((size_t)rows * chunks)), block(kQualThreads);
  SpecLossSums* p = static_cast<SpecLossSums*>(partials);
  const bool lg = floor > 0.f;
  if (plain && lg) hipLaunchKernelGGL((spec_loss_partial_kernel<true, true>), grid, block, 0, s, a, m, p, T, fs, n_stft, chunks, floor);
  else if (plain) hipLaunchKernelGGL((spec_loss_partial_kernel<true, false>), grid, block, 0, s, a, m, p, T, fs, n_stft, chunks, floor);
  else if (lg) hipLaunchKernelGGL((spec_loss_partial_kernel<false, true>), grid, block, 0, s, a, m, p, T, fs, n_stft, chunks, floor);
  else hipLaunchKernelGGL((spec_loss_partial_kernel<false, false>), grid, block, 0, s, a, m, p, T, fs, n_stft, chunks, floor);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(spec_loss_combine_kernel, dim3((unsigned)rows), block, 0, s, p, sums, chunks);
  return hipGetLastError();
}

}  // namespace rfx
