// rfx_holdmask.hip - the two streaming kernels of a masked Griffin-Lim call (include/rfx.h: rfx_masked_call_options; arithmetic in
// rfx_holdmask_core.h): the split of the call's magnitude slots by the bit mask into the array the iterations read, and the
// expansion of a per-mel-band mask to the bin mask.  Rows go on grid y in chunks of 65535; every offset is formed in 64 bits.
#include <hip/hip_runtime.h>

#include "rfx_holdmask_core.h"
#include "rfx_kernels.h"

namespace rfx {

// X[frame][p] = S[frame][p] where the position's bin is held (want_held) or free (!want_held), else 0; padding positions 0.
// One thread per position of the frame (consecutive lanes, consecutive floats), frames of the row on grid z
template <int LAYOUT>
__global__ void __launch_bounds__(kHoldMaskThreads) holdmask_split_kernel(const float* __restrict__ S, float* __restrict__ X,
                                                                          const uint32_t* __restrict__ mask, const int* __restrict__ bin_of,
                                                                          int row0, int T, int stride, int n_stft, int words, int want_held) {
  const int p = blockIdx.x * kHoldMaskThreads + threadIdx.x;
  if (p >= stride) return;
  const size_t row = (size_t)row0 + blockIdx.y;
  const int bin = holdmask_slot_bin(LAYOUT, p, n_stft, bin_of);
  for (int t = blockIdx.z; t < T; t += gridDim.z) {
    const size_t fr = row * (size_t)T + t, at = fr * (size_t)stride + p;
    X[at] = holdmask_split(S[at], bin, mask + fr * (size_t)words, want_held != 0);
  }
}

hipError_t launch_holdmask_split(int layout, const float* S, float* X, const uint32_t* mask, const int* bin_of, int B, int T, int stride,
                                 int n_stft, bool want_held, hipStream_t stream) {
  const int words = holdmask_words(n_stft);
  const unsigned gx = (unsigned)((stride + kHoldMaskThreads - 1) / kHoldMaskThreads), gz = (unsigned)(T < 65535 ? T : 65535);
  for (int r0 = 0; r0 < B; r0 += 65535) {  // (grid y is 16 bits wide)
    const int n = B - r0 < 65535 ? B - r0 : 65535;
    const dim3 grid(gx, (unsigned)n, gz);
    const int wh = want_held ? 1 : 0;
    if (layout == kHoldMaskSpec)
      hipLaunchKernelGGL(holdmask_split_kernel<kHoldMaskSpec>, grid, dim3(kHoldMaskThreads), 0, stream, S, X, mask, bin_of, r0, T, stride, n_stft, words, wh);
    else if (layout == kHoldMaskTable)
      hipLaunchKernelGGL(holdmask_split_kernel<kHoldMaskTable>, grid, dim3(kHoldMaskThreads), 0, stream, S, X, mask, bin_of, r0, T, stride, n_stft, words, wh);
    else
      hipLaunchKernelGGL(holdmask_split_kernel<kHoldMaskPlain>, grid, dim3(kHoldMaskThreads), 0, stream, S, X, mask, bin_of, r0, T, stride, n_stft, words, wh);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// out[row][t][word] from bands[row][m][t]: one thread per (word, t) of the row, consecutive lanes consecutive frames - the band
// bytes a wave reads are consecutive; the one word a lane writes lies `words` from its neighbour's
__global__ void __launch_bounds__(kHoldMaskThreads) holdmask_bands_kernel(const uint8_t* __restrict__ bands, const int16_t* __restrict__ lo,
                                                                          const int16_t* __restrict__ hi, uint32_t* __restrict__ out, int row0,
                                                                          int M, int T, int n_stft, int words) {
  const long long i = (long long)blockIdx.x * kHoldMaskThreads + threadIdx.x;
  if (i >= (long long)T * words) return;
  const int word = (int)(i / T), t = (int)(i - (long long)word * T);
  const size_t row = (size_t)row0 + blockIdx.y;
  out[(row * (size_t)T + t) * (size_t)words + word] = holdmask_band_word(bands + row * (size_t)M * (size_t)T, T, t, lo, hi, word, n_stft);
}

hipError_t launch_holdmask_bands(const uint8_t* bands, const int16_t* lo, const int16_t* hi, uint32_t* out, int B, int M, int T, int n_stft,
                                 hipStream_t stream) {
  const int words = holdmask_words(n_stft);
  const unsigned gx = (unsigned)(((long long)T * words + kHoldMaskThreads - 1) / kHoldMaskThreads);
  for (int r0 = 0; r0 < B; r0 += 65535) {
    const int n = B - r0 < 65535 ? B - r0 : 65535;
    hipLaunchKernelGGL(holdmask_bands_kernel, dim3(gx, (unsigned)n), dim3(kHoldMaskThreads), 0, stream, bands, lo, hi, out, r0, M, T, n_stft, words);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace rfx
