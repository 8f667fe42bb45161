// rfx_guide.hip - staging of a guided Griffin-Lim call's guide waveforms (include/rfx.h: rfx_guided_call_options): the caller's
// (B, guide_samples) rows, fitted to the call's L samples and brought into the kernels' numeric range by exact powers of two, into
// the audio buffer the call's first launch analyses.  Arithmetic and the shape of the peak reduction: rfx_guide_core.h.
// Two launches over (chunk, row): the chunks' peaks, then the scaled copy.
#include <hip/hip_runtime.h>

#include "rfx_guide_core.h"
#include "rfx_kernels.h"

namespace rfx {

namespace {
using v4 = float __attribute__((ext_vector_type(4)));

// samples p .. p + 3 of the fitted row (p a multiple of four): one 16-byte load where the source allows it
template <bool VEC>
__device__ __forceinline__ v4 guide_load4(const float* __restrict__ row, int n_valid, int p) {
  if (VEC && p + 3 < n_valid) return *reinterpret_cast<const v4*>(row + p);
  return v4{guide_fit(row, n_valid, p), guide_fit(row, n_valid, p + 1), guide_fit(row, n_valid, p + 2), guide_fit(row, n_valid, p + 3)};
}

// the largest of the workgroup's values, in every thread
__device__ __forceinline__ float block_max(float x, float* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
  __syncthreads();
  float m = lds[0];
#pragma unroll
  for (int w = 1; w < kGuideThreads / 64; ++w) m = fmaxf(m, lds[w]);
  return m;
}

// first sample of thread `tid`'s i-th vector of chunk `chunk`
__device__ __forceinline__ int guide_vec_at(int chunk, int i, int tid) { return chunk * kGuideChunk + (i * kGuideThreads + tid) * 4; }
}  // namespace

// peaks[row * chunks + chunk] = max |sample| of the chunk's part of the fitted row
template <bool VEC>
__global__ void __launch_bounds__(kGuideThreads) guide_peak_kernel(const float* __restrict__ guide, long long stride, int n_valid, int row0,
                                                                   float* __restrict__ peaks) {
  __shared__ float lds[kGuideThreads / 64];
  const int chunk = blockIdx.x, row = row0 + (int)blockIdx.y;
  const float* __restrict__ src = guide + (long long)row * stride;
  float peak = 0.f;
#pragma unroll
  for (int i = 0; i < kGuideVecsPerThread; ++i) {
    const int p = guide_vec_at(chunk, i, threadIdx.x);
    if (p < n_valid) {  // (behind it the fitted row is zero)
      const v4 v = guide_load4<VEC>(src, n_valid, p);
      peak = guide_peak_step(guide_peak_step(guide_peak_step(guide_peak_step(peak, v.x), v.y), v.z), v.w);
    }
  }
  peak = block_max(peak, lds);
  if (threadIdx.x == 0) peaks[(size_t)row * gridDim.x + chunk] = peak;
}

// dst[row][p] = fitted sample x 2^n / row_scale[2 row] for p < Lpad; zero[row][p] = 0 (the buffer the first launch adds to dst)
template <bool VEC>
__global__ void __launch_bounds__(kGuideThreads) guide_stage_kernel(const float* __restrict__ guide, long long stride, int n_valid, int Lpad,
                                                                    int row0, const float* __restrict__ peaks, const float* __restrict__ row_scale,
                                                                    float* __restrict__ dst, float* __restrict__ zero) {
  __shared__ float lds[kGuideThreads / 64];
  const int chunk = blockIdx.x, chunks = gridDim.x, row = row0 + (int)blockIdx.y;
  float peak = 0.f;
  for (int c = threadIdx.x; c < chunks; c += kGuideThreads) peak = fmaxf(peak, peaks[(size_t)row * chunks + c]);
  peak = block_max(peak, lds);
  const GuideScale s = guide_scale(peak, row_scale ? row_scale[2 * (size_t)row] : 0.f);
  const float* __restrict__ src = guide + (long long)row * stride;
  const size_t out_at = (size_t)row * Lpad;
#pragma unroll
  for (int i = 0; i < kGuideVecsPerThread; ++i) {
    const int p = guide_vec_at(chunk, i, threadIdx.x);
    if (p >= Lpad) continue;  // (Lpad is a multiple of 64: a vector is inside the row or outside it)
    v4 v = {0.f, 0.f, 0.f, 0.f};
    if (p < n_valid) {
      v = guide_load4<VEC>(src, n_valid, p);
      v = v4{guide_apply(v.x, s), guide_apply(v.y, s), guide_apply(v.z, s), guide_apply(v.w, s)};
    }
    *reinterpret_cast<v4*>(dst + out_at + p) = v;
    if (zero) *reinterpret_cast<v4*>(zero + out_at + p) = v4{0.f, 0.f, 0.f, 0.f};
  }
}

hipError_t launch_guide_stage(const float* guide, long long stride, int guide_samples, int B, int L, int Lpad, const float* row_scale,
                              float* peaks, float* dst, float* zero, hipStream_t stream) {
  const int n_valid = guide_samples < L ? guide_samples : L;
  const int chunks = guide_chunks(Lpad);
  const bool vec = ((uintptr_t)guide & 15) == 0 && (stride & 3) == 0;
  for (int r0 = 0; r0 < B; r0 += 65535) {  // (grid y is 16 bits wide)
    const int n = B - r0 < 65535 ? B - r0 : 65535;
    const dim3 grid((unsigned)chunks, (unsigned)n);
    if (vec) hipLaunchKernelGGL(guide_peak_kernel<true>, grid, dim3(kGuideThreads), 0, stream, guide, stride, n_valid, r0, peaks);
    else hipLaunchKernelGGL(guide_peak_kernel<false>, grid, dim3(kGuideThreads), 0, stream, guide, stride, n_valid, r0, peaks);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (vec) hipLaunchKernelGGL(guide_stage_kernel<true>, grid, dim3(kGuideThreads), 0, stream, guide, stride, n_valid, Lpad, r0, peaks, row_scale, dst, zero);
    else hipLaunchKernelGGL(guide_stage_kernel<false>, grid, dim3(kGuideThreads), 0, stream, guide, stride, n_valid, Lpad, r0, peaks, row_scale, dst, zero);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace rfx
