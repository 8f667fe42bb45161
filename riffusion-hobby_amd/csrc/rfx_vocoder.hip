// rfx_vocoder.hip - the kernel of the time stretch (rfx_vocoder_core.h states the arithmetic; include/rfx.h "TIME STRETCH":
// rfx_phase_vocoder, rfx_time_stretch).  A complex spectrogram in slot layout, rows of T frames, to rows of T_out frames in the same
// layout: torchaudio.functional.phase_vocoder per bin.
//
//   vocoder_kernel   one thread per position of a frame, the row in blockIdx.y.  Adjacent lanes take adjacent positions, so a frame
//                    access of a wave is a run of whole lines (a position whose bin lives elsewhere - the second slot of a doubled
//                    bin, 440 of 9408 on the specialised engine - reads its bin's primary slot instead of its own).  The thread
//                    walks the T_out output frames serially (voc_walk): the frame pair stays in registers in polar form, the loads
//                    run two steps ahead of the phase accumulator.  A position writes its own slot: conjugated where exactly one of
//                    it and the primary slot holds the conjugate, so both slots of a doubled bin leave as one trajectory; padding
//                    positions are written zero.  No LDS, no atomics, nothing shared between threads.
#include <hip/hip_runtime.h>

#include "rfx_kernels.h"
#include "rfx_vocoder_core.h"

namespace rfx {

constexpr int kVocThreads = 256;
constexpr int kVocMaxRows = 65535;  // blockIdx.y

__global__ void __launch_bounds__(kVocThreads) vocoder_kernel(VocoderArgs a) {
  const int p = (int)(blockIdx.x * kVocThreads + threadIdx.x);
  if (p >= a.stride) return;
  const size_t stride = (size_t)a.stride;
  const cf* __restrict__ in = a.in + (size_t)blockIdx.y * (size_t)a.T * stride;
  cf* __restrict__ out = a.out + (size_t)blockIdx.y * (size_t)a.T_out * stride + p;
  const int2 e = a.table[p];
  if (e.x < 0) {  // padding
    for (int i = 0; i < a.T_out; ++i) out[(size_t)i * stride] = cf{0.f, 0.f};
    return;
  }
  const bool flip = (e.x & kVocFlip) != 0;
  const float adv = __int_as_float(e.y);
  in += e.x & (kVocFlip - 1);
  voc_walk(
      a.T, a.T_out, a.rate, flip ? -adv : adv, [=](int j) { return in[(size_t)j * stride]; },
      [=](int i, cf v) {
        if (flip) v.im = -v.im;
        out[(size_t)i * stride] = v;
      });
}

hipError_t launch_vocoder(const VocoderArgs& args, hipStream_t stream) {
  if (args.rows <= 0 || args.T <= 0 || args.T_out <= 0) return hipSuccess;
  const dim3 block(kVocThreads);
  for (int r0 = 0; r0 < args.rows; r0 += kVocMaxRows) {
    VocoderArgs a = args;
    a.rows = args.rows - r0 < kVocMaxRows ? args.rows - r0 : kVocMaxRows;
    a.in = args.in + (size_t)r0 * (size_t)args.T * (size_t)args.stride;
    a.out = args.out + (size_t)r0 * (size_t)args.T_out * (size_t)args.stride;
    hipLaunchKernelGGL(vocoder_kernel, dim3((unsigned)((a.stride + kVocThreads - 1) / kVocThreads), (unsigned)a.rows), block, 0, stream, a);
    if (const hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

}  // namespace rfx
