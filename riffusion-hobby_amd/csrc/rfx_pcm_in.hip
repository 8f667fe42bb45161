// rfx_pcm_in.hip - the int16 PCM front end of the encode on the device (riffusion/util/audio_util.py):
//   * set_channels + set_frame_rate of one (L, C_in) int16 recording -> (K, C_out) int16: audioop.tomono / tostereo applied to
//     the stored frames, then audioop.ratecv, byte for byte.  One streaming launch, no LDS: a thread produces kRatecvRun
//     consecutive output frames with audioop's recurrence (one 64-bit division for its first frame) and stores them as 16-byte
//     groups.  The input loads are NOT coalesced per instruction: lane j reads around input frame 8 j a / b, so one load of a
//     wave strides the lanes by 8 a / b frames (35 bytes for stereo 48 -> 44.1 kHz: about 18 cache lines per instruction).  Over
//     its run the wave consumes every byte of the one contiguous span of 64 * 8 * a / b frames those lines make up, out of L1 /
//     L2; DESIGN.md 4.4 has the measured rate next to a copy's.
//   * N clips of Lw frames, clip i starting at frame starts[i], out of one (L, C_in) int16 recording -> the (N * C_out, Lw)
//     float32 planar rows rfx_image_from_waveform reads, with the channel mix applied after the slice.  One launch, one frame
//     per thread and step: a wave loads 64 consecutive frames and stores 256 contiguous bytes per row.  (The rows of a clip
//     start wherever Lw puts them, so wider stores would need a per-row head and tail for 0.9 MB a row.)
// The arithmetic is rfx_pcm_in_core.h, shared with the CPU emulator of the tests.  Every index is int64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rfx_kernels.h"
#include "rfx_pcm_in_core.h"

namespace rfx {

namespace {

constexpr int kPcmInThreads = 256;

// the mixed frame `frame` (-1: ratecv's zero state) as CC = min(C_IN, C_OUT) channel values
template <int C_IN, int C_OUT>
__device__ __forceinline__ void load_mixed(const int16_t* __restrict__ pcm, int64_t frame, int (&v)[2]) {
  v[0] = v[1] = 0;
  if (frame < 0) return;
  if (C_IN == 1) {
    v[0] = pcm[frame];
  } else {
    // a stereo frame is one aligned dword (the entry point checks the pointer)
    const int w = *reinterpret_cast<const int*>(pcm + 2 * frame);
    const int l = (int)(int16_t)(w & 0xFFFF), r = w >> 16;
    if (C_OUT == 1) v[0] = pcm_tomono(l, r);
    else v[0] = l, v[1] = r;
  }
}

// ---- resample: thread i < n_runs produces output frames [head + 8 i, head + 8 i + 8) (fewer in the last run); the `head`
// frames before the first 16-byte boundary of the output, one each, go to threads n_runs .. n_runs + head - 1
template <int C_IN, int C_OUT>
__global__ void __launch_bounds__(kPcmInThreads) pcm_ratecv_kernel(const int16_t* __restrict__ in, int16_t* __restrict__ out, int64_t K,
                                                                   RatecvRates r, int64_t head, int64_t n_runs) {
  constexpr int CC = C_IN < C_OUT ? C_IN : C_OUT;  // channels interpolated (tostereo duplicates one)
  const int64_t i = (int64_t)blockIdx.x * kPcmInThreads + threadIdx.x;
  if (i >= n_runs + head) return;
  const int64_t k0 = i < n_runs ? head + kRatecvRun * i : i - n_runs;
  const int64_t left = K - k0;
  const int count = i < n_runs ? (left < kRatecvRun ? (int)left : kRatecvRun) : 1;
  int16_t res[kRatecvRun * C_OUT];
  ratecv_run<C_OUT, CC>(k0, count, r, [&](int64_t frame, int (&v)[2]) { load_mixed<C_IN, C_OUT>(in, frame, v); }, res);
  int16_t* dst = out + k0 * C_OUT;
  if (count == kRatecvRun) {  // a whole run starts on a 16-byte boundary: the launcher chose `head` so
#pragma unroll
    for (int q = 0; q < kRatecvRun * C_OUT / 8; ++q) {
      int w[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        w[e] = (int)(((unsigned)(uint16_t)res[8 * q + 2 * e]) | ((unsigned)(uint16_t)res[8 * q + 2 * e + 1] << 16));
      reinterpret_cast<int4*>(dst)[q] = int4{w[0], w[1], w[2], w[3]};
    }
  } else {
#pragma unroll
    for (int j = 0; j < kRatecvRun; ++j) {
      if (j < count) {
#pragma unroll
        for (int c = 0; c < C_OUT; ++c) dst[j * C_OUT + c] = res[j * C_OUT + c];
      }
    }
  }
}

// ---- clip gather: workgroups (x, y) walk frames x * 256 + lane (+ the grid's width) of clips y (+ the grid's height) -> rows
// n * C_OUT + c of the planar float32 output
template <int C_IN, int C_OUT>
__global__ void __launch_bounds__(kPcmInThreads) pcm_clips_kernel(const int16_t* __restrict__ pcm, const int64_t* __restrict__ starts,
                                                                  int N, int64_t Lw, float* __restrict__ wave) {
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const int64_t start = starts[n];
    float* row = wave + (int64_t)n * C_OUT * Lw;
    for (int64_t t = (int64_t)blockIdx.x * kPcmInThreads + threadIdx.x; t < Lw; t += (int64_t)gridDim.x * kPcmInThreads) {
      int v[2];
      load_mixed<C_IN, C_OUT>(pcm, start + t, v);
      row[t] = (float)v[0];  // |v| <= 2^15: exact
      if (C_OUT == 2) row[Lw + t] = (float)v[C_IN == 2 ? 1 : 0];
    }
  }
}

}  // namespace

hipError_t launch_pcm_ratecv(const int16_t* in, int C_in, int64_t in_rate, int C_out, int64_t out_rate, int16_t* out, int64_t K,
                             hipStream_t s) {
  const RatecvRates r = ratecv_rates(in_rate, out_rate);
  // frames before the output's first 16-byte boundary (frames are 2 * C_out bytes and the pointer is frame-aligned)
  const int64_t frame_bytes = 2 * C_out;
  int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15) / frame_bytes;
  if (head > K) head = K;
  const int64_t n_runs = (K - head + kRatecvRun - 1) / kRatecvRun;
  const int64_t blocks = (n_runs + head + kPcmInThreads - 1) / kPcmInThreads;
  const dim3 grid((unsigned)blocks), block(kPcmInThreads);
  if (C_in == 1 && C_out == 1) hipLaunchKernelGGL((pcm_ratecv_kernel<1, 1>), grid, block, 0, s, in, out, K, r, head, n_runs);
  else if (C_in == 2 && C_out == 2) hipLaunchKernelGGL((pcm_ratecv_kernel<2, 2>), grid, block, 0, s, in, out, K, r, head, n_runs);
  else if (C_in == 2) hipLaunchKernelGGL((pcm_ratecv_kernel<2, 1>), grid, block, 0, s, in, out, K, r, head, n_runs);
  else hipLaunchKernelGGL((pcm_ratecv_kernel<1, 2>), grid, block, 0, s, in, out, K, r, head, n_runs);
  return hipGetLastError();
}

hipError_t launch_pcm_clips(const int16_t* pcm, int C_in, const int64_t* starts, int N, int64_t Lw, int C_out, float* wave, hipStream_t s) {
  int64_t bx = (Lw + kPcmInThreads - 1) / kPcmInThreads;
  if (bx > 4096) bx = 4096;
  const dim3 grid((unsigned)bx, (unsigned)(N < 65535 ? N : 65535)), block(kPcmInThreads);
  if (C_in == 1 && C_out == 1) hipLaunchKernelGGL((pcm_clips_kernel<1, 1>), grid, block, 0, s, pcm, starts, N, Lw, wave);
  else if (C_in == 2 && C_out == 2) hipLaunchKernelGGL((pcm_clips_kernel<2, 2>), grid, block, 0, s, pcm, starts, N, Lw, wave);
  else if (C_in == 2) hipLaunchKernelGGL((pcm_clips_kernel<2, 1>), grid, block, 0, s, pcm, starts, N, Lw, wave);
  else hipLaunchKernelGGL((pcm_clips_kernel<1, 2>), grid, block, 0, s, pcm, starts, N, Lw, wave);
  return hipGetLastError();
}

}  // namespace rfx
