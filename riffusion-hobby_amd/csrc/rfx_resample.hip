// rfx_resample.hip - the kernel of the windowed-sinc resampler (rfx_resample_core.h states the arithmetic; include/rfx.h "SINC
// RESAMPLE": rfx_resample_sinc, and the third stage of rfx_pitch_shift).  Rows of float32 samples to rows of float32 samples:
// torchaudio.functional.resample's polyphase sum over the taps inside the window's support only.
//
//   resample_kernel  one thread per output sample j and block of kRsRows rows: blockIdx.x walks j, blockIdx.y the row blocks.  The
//                    thread reads its phase's first offset once and each of the ntaps weights once - tap-major, so the 64 lanes of a
//                    wave, which hold consecutive phases, read consecutive floats - and carries the kRsRows accumulators in registers:
//                    the 4 ntaps table bytes per output are shared by kRsRows outputs.  The input runs of neighbouring lanes overlap
//                    almost entirely (they start o / n samples apart), so a wave's input reads per tap fall into one or two lines;
//                    the span is not staged in LDS.  A row block's last rows past `rows` repeat the last row's reads and are not
//                    stored.  A run that leaves [0, valid) reads zeros there (rs_sample).  No LDS, no atomics, nothing shared between
//                    threads.
#include <hip/hip_runtime.h>

#include "rfx_kernels.h"
#include "rfx_resample_core.h"

namespace rfx {

constexpr int kRsThreads = 256;
constexpr int kRsMaxBlocksY = 65535;  // blockIdx.y

__global__ void __launch_bounds__(kRsThreads) resample_kernel(ResampleArgs a) {
  const int64_t j = (int64_t)blockIdx.x * kRsThreads + threadIdx.x;
  if (j >= a.K) return;
  const int r0 = (int)blockIdx.y * kRsRows, last = a.rows - 1;
  const float* rows[kRsRows];
#pragma unroll
  for (int r = 0; r < kRsRows; ++r) rows[r] = a.in + (size_t)(r0 + r < last ? r0 + r : last) * (size_t)a.in_stride;
  const RsStart s = rs_start(j, a.o, a.n, a.first);
  float acc[kRsRows];
  rs_accumulate<kRsRows>(rows, a.valid, s.at, a.taps + s.p, a.n, a.ntaps, acc);
#pragma unroll
  for (int r = 0; r < kRsRows; ++r)
    if (r0 + r <= last) a.out[(size_t)(r0 + r) * (size_t)a.out_stride + (size_t)j] = acc[r];
}

hipError_t launch_resample_sinc(const ResampleArgs& args, hipStream_t stream) {
  if (args.rows <= 0 || args.K <= 0) return hipSuccess;
  const int per_launch = kRsMaxBlocksY * kRsRows;
  for (int r0 = 0; r0 < args.rows; r0 += per_launch) {
    ResampleArgs a = args;
    a.rows = args.rows - r0 < per_launch ? args.rows - r0 : per_launch;
    a.in = args.in + (size_t)r0 * (size_t)args.in_stride;
    a.out = args.out + (size_t)r0 * (size_t)args.out_stride;
    const dim3 grid((unsigned)((a.K + kRsThreads - 1) / kRsThreads), (unsigned)((a.rows + kRsRows - 1) / kRsRows));
    hipLaunchKernelGGL(resample_kernel, grid, dim3(kRsThreads), 0, stream, a);
    if (const hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

}  // namespace rfx
