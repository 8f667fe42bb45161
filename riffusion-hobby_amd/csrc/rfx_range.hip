// rfx_range.hip - numeric range (round 6, include/rfx.h "Numeric range"): the powers of two the InverseMelScale SGD and the
// Griffin-Lim kernels work in, per clip / per row, from the data's largest amplitude or the caller's magnitude_hint.
#include <hip/hip_runtime.h>

#include "rfx_core.h"
#include "rfx_kernels.h"

namespace rfx {

// max |x| per group as an integer key (the bits of a non-negative float order like the float; NaN is skipped, as fmaxf does)
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
  return x;
}
__global__ void __launch_bounds__(256) range_max_kernel(const float* __restrict__ x, size_t count, unsigned* __restrict__ keys) {
  const float* p = x + (size_t)blockIdx.y * count;
  float mx = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) mx = fmaxf(mx, fabsf(p[i]));
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(&keys[blockIdx.y], __float_as_uint(mx));
}
__global__ void __launch_bounds__(64) range_finish_kernel(const unsigned* __restrict__ keys, int groups, float hint, float* __restrict__ imel_scale,
                                                          float* __restrict__ gl_scale, int rows, int mel_units) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= groups) return;
  const float mx = hint > 0.f ? hint : __uint_as_float(keys[g]);
  int k = 0;  // mx in [2^(k-1), 2^k); an all-zero (or all-NaN) group works in the default units
  if (mx > 0.f) {
    if (mx < __builtin_inff()) (void)frexpf(mx, &k);
    else k = 129;
  }
  int e, j;
  range_exponents(k, mel_units, &e, &j);
  if (imel_scale) {
    // e = max(k + 35, 30): the clip's largest target near 2^-35 of the clamp's upper bound (2^-60 for max_value = 30e6, as in rounds
    // 2-5); never above 2^-30: the untouched bins start at U[0, 1) in the reference's units whatever the targets are
    imel_scale[2 * g] = ldexpf(1.f, -e);
    imel_scale[2 * g + 1] = ldexpf(1.f, e);
  }
  if (gl_scale) {
    // j = ks - 26: the row's largest magnitude near 2^25, what 30e6 gives unscaled (j = 0); ks = k, or max(k, 0) + 1 in mel units
    const float eps2 = fmaxf(ldexpf(1e-32f, -2 * j), 1.17549435e-38f);  // never zero: 0 * rsq(0 + 0) would be NaN where the reference gives 0
    for (int r = 0; r < rows; ++r) {
      gl_scale[2 * ((size_t)g * rows + r)] = ldexpf(1.f, -j);
      gl_scale[2 * ((size_t)g * rows + r) + 1] = eps2;
    }
  }
}
hipError_t launch_range_scale(const float* x, size_t count, int groups, float hint, unsigned* keys, float* imel_scale, float* gl_scale, int rows,
                              int mel_units, hipStream_t stream) {
  if (!(hint > 0.f)) {
    hipError_t e = hipMemsetAsync(keys, 0, sizeof(unsigned) * (size_t)groups, stream);
    if (e != hipSuccess) return e;
    size_t chunks = (count + 256 * 64 - 1) / (256 * 64);  // ~64 values per thread
    if (chunks > 256) chunks = 256;
    if (chunks < 1) chunks = 1;
    for (int g0 = 0; g0 < groups; g0 += 65535) {  // (grid y is 16 bits wide)
      const int n = groups - g0 < 65535 ? groups - g0 : 65535;
      hipLaunchKernelGGL(range_max_kernel, dim3((unsigned)chunks, (unsigned)n), dim3(256), 0, stream, x + (size_t)g0 * count, count, keys + g0);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  hipLaunchKernelGGL(range_finish_kernel, dim3((groups + 63) / 64), dim3(64), 0, stream, keys, groups, hint, imel_scale, gl_scale, rows, mel_units);
  return hipGetLastError();
}

}  // namespace rfx
