// rfx_istft.hip - the kernels of the inverse spectrogram (rfx_istft_core.h states the arithmetic; include/rfx.h: rfx_istft,
// rfx_istft_loop, rfx_istft_backward, rfx_istft_backward_loop).  Between them run kernels the library already has, unchanged: the
// engines' MODE 0 per-frame launches and the Griffin-Lim folds (forward); the engines' forward frame kernels (backward) - their
// zero-extension twins for the plain form (rfx_stft_kernels.hip.h and its three siblings, RFX_FWDK_LOOP 2), the loop twins for a loop.
//
//   istft_unit_slots_kernel  forward: the magnitude slots a MODE 0 launch multiplies the caller's spectrum by - 1 in every slot that
//                            holds a bin, 0 in the padding.  Never a range table: the synthesis is linear in X.
//   istft_stage_kernel       backward: g (rows, valid) -> u (rows, pitch): the gradient times the reciprocal-envelope table (or
//                            divided by the envelope); pitch == valid for the entries, and zeros from `valid` to `pitch` for the padded
//                            period of the twin's test route.  16-byte stores over the group's flat array; no atomics.
//   istft_grad_kernel        backward epilogue: the analysis frames t < T of every row (Tp per row: the test route's period has more) times c_k unit,
//                            imaginary part exactly 0 where c_k = 1, into gradient slots in rfx_pack_complex's layout.  The forward
//                            transform writes that layout - conjugate slots conjugated, both slots of a doubled bin - and a real
//                            factor keeps it; the padding gets 0.  16-byte loads and stores, two complex values per lane.
#include <hip/hip_runtime.h>

#include "rfx_istft_core.h"
#include "rfx_kernels.h"

namespace rfx {

constexpr int kIstftThreads = 256;
constexpr long long kIstftMaxBlocks = 1 << 16;

__global__ void __launch_bounds__(kIstftThreads) istft_unit_slots_kernel(float* __restrict__ S, const int* __restrict__ pos_bin, long long nframes,
                                                                        int sstride) {
  const int4* __restrict__ pb4 = reinterpret_cast<const int4*>(pos_bin);
  for (long long fr = blockIdx.x; fr < nframes; fr += gridDim.x) {
    float4* __restrict__ S4 = reinterpret_cast<float4*>(S + (size_t)fr * sstride);
    for (int i = (int)threadIdx.x; i < sstride / 4; i += (int)blockDim.x) {
      const int4 k = pb4[i];
      S4[i] = float4{k.x < 0 ? 0.f : 1.f, k.y < 0 ? 0.f : 1.f, k.z < 0 ? 0.f : 1.f, k.w < 0 ? 0.f : 1.f};
    }
  }
}

__global__ void __launch_bounds__(kIstftThreads) istft_stage_kernel(IstftStageArgs a) {
  const long long groups = (a.total + 3) / 4;  // the last group may reach past `total`: the buffer is a whole number of 16 bytes
  for (long long i4 = (long long)blockIdx.x * blockDim.x + threadIdx.x; i4 < groups; i4 += (long long)gridDim.x * blockDim.x) {
    float v[4];
    long long r = 4 * i4 / a.pitch;  // one division per group: the row and column of its first element, stepped from there
    int col = (int)(4 * i4 - r * a.pitch);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = 0.f;
      if (4 * i4 + e < a.total) {
        const int entry = istft_stage_entry(col, a.valid, a.period);
        if (entry >= 0) v[e] = istft_stage_value(a.g[(size_t)r * a.valid + col], a.tab[entry], a.divide != 0);
      }
      if (++col == a.pitch) {
        col = 0;
        ++r;
      }
    }
    reinterpret_cast<float4*>(a.u)[i4] = float4{v[0], v[1], v[2], v[3]};
  }
}

__global__ void __launch_bounds__(kIstftThreads) istft_grad_kernel(IstftGradArgs a) {
  const int2* __restrict__ xb2 = reinterpret_cast<const int2*>(a.xpos_bin);
  const long long nframes = (long long)a.rows * a.T;
  for (long long fr = blockIdx.x; fr < nframes; fr += gridDim.x) {
    const long long r = fr / a.T;
    const int t = (int)(fr - r * a.T);
    const float4* __restrict__ X4 = reinterpret_cast<const float4*>(a.spec + ((size_t)r * a.Tp + t) * a.xstride);
    float4* __restrict__ G4 = reinterpret_cast<float4*>(a.out + (size_t)fr * a.xstride);
    for (int i = (int)threadIdx.x; i < a.xstride / 2; i += (int)blockDim.x) {
      const float4 x = X4[i];
      const int2 k = xb2[i];
      float4 o = {0.f, 0.f, 0.f, 0.f};
      if (k.x >= 0) istft_grad_slot(k.x, a.n_fft, a.unit, x.x, x.y, o.x, o.y);
      if (k.y >= 0) istft_grad_slot(k.y, a.n_fft, a.unit, x.z, x.w, o.z, o.w);
      G4[i] = o;
    }
  }
}

hipError_t launch_istft_unit_slots(float* S, const int* pos_bin, long long nframes, int sstride, hipStream_t stream) {
  if (nframes <= 0) return hipSuccess;
  const unsigned grid = (unsigned)(nframes < kIstftMaxBlocks ? nframes : kIstftMaxBlocks);
  hipLaunchKernelGGL(istft_unit_slots_kernel, dim3(grid), dim3(kIstftThreads), 0, stream, S, pos_bin, nframes, sstride);
  return hipGetLastError();
}

hipError_t launch_istft_stage(const IstftStageArgs& a, hipStream_t stream) {
  if (a.total <= 0) return hipSuccess;
  const long long blocks = ((a.total + 3) / 4 + kIstftThreads - 1) / kIstftThreads;
  hipLaunchKernelGGL(istft_stage_kernel, dim3((unsigned)(blocks < kIstftMaxBlocks ? blocks : kIstftMaxBlocks)), dim3(kIstftThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_istft_grad(const IstftGradArgs& a, hipStream_t stream) {
  const long long nframes = (long long)a.rows * a.T;
  if (nframes <= 0) return hipSuccess;
  hipLaunchKernelGGL(istft_grad_kernel, dim3((unsigned)(nframes < kIstftMaxBlocks ? nframes : kIstftMaxBlocks)), dim3(kIstftThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace rfx
