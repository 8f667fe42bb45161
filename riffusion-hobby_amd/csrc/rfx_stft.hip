// rfx_stft.hip - forward framed transform (replaces torchaudio.transforms.Spectrogram(power=None) +
// torch.abs, riffusion/spectrogram_converter.py:47-59, :179-182) and the layout converters between
// the reference's (B, n_stft, T) tensors and the slot-major frames the gfx950 kernels stream.
#define RFX_PK 1  // packed fp32 butterflies (rfx_core.h)
#include "rfx_frame.hip.h"
#include "rfx_kernels.h"
#include "rfx_loop_core.h"
#include "rfx_istft_core.h"

namespace rfx {

// one thread per slot position, 16 consecutive frames: reads 64 contiguous bytes of a bin row and
// writes position-contiguous (coalesced) floats into 16 frames
template <bool COMPLEX>
__global__ void __launch_bounds__(256) pack_kernel(const void* __restrict__ src_, void* __restrict__ dst_, int T) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= kFrameStride) return;
  const int tchunk = blockIdx.y * 16;
  const int clip = blockIdx.z;
  int q, kb;
  const bool real_slot = COMPLEX ? pos_c_to_slot(p, q, kb) : pos_f_to_slot(p, q, kb);
  if (!real_slot) {  // padding lane: keep it zero
    const int ntp = min(16, T - tchunk);
    for (int i = 0; i < ntp; ++i) {
      const size_t o = ((size_t)clip * T + tchunk + i) * kFrameStride + p;
      if (COMPLEX) reinterpret_cast<cf*>(dst_)[o] = cf{0.f, 0.f}; else reinterpret_cast<float*>(dst_)[o] = 0.f;
    }
    return;
  }
  bool cj;
  const int bin = slot_bin(q / 21, q % 21, kb, &cj);
  const int nt = min(16, T - tchunk);
  if (COMPLEX) {
    const cf* src = reinterpret_cast<const cf*>(src_) + ((size_t)clip * kBins + bin) * T + tchunk;
    cf* dst = reinterpret_cast<cf*>(dst_) + ((size_t)clip * T + tchunk) * kFrameStride + p;
    for (int i = 0; i < nt; ++i) {
      cf v = src[i];
      if (cj) v.im = -v.im;
      dst[(size_t)i * kFrameStride] = v;
    }
  } else {
    const float* src = reinterpret_cast<const float*>(src_) + ((size_t)clip * kBins + bin) * T + tchunk;
    float* dst = reinterpret_cast<float*>(dst_) + ((size_t)clip * T + tchunk) * kFrameStride + p;
    for (int i = 0; i < nt; ++i) dst[(size_t)i * kFrameStride] = src[i];
  }
}

// slots -> (B, n_stft, T) complex, reading each bin from its primary slot (test / debugging path)
__global__ void __launch_bounds__(256) unpack_complex_kernel(const cf* __restrict__ slots, cf* __restrict__ out, int T) {
  const int bin = blockIdx.x * blockDim.x + threadIdx.x;
  if (bin >= kBins) return;
  const int tchunk = blockIdx.y * 16;
  const int clip = blockIdx.z;
  int k = bin;
  bool cj = false;
  if (k % 40 > 20) { k = kNfft - k; cj = true; }
  const int k1 = k % 40, kp = k / 40;
  const int ka = kp % 21, kb = kp / 21;
  const int p = slot_pos_c(k1 * 21 + ka, kb);
  const int nt = min(16, T - tchunk);
  for (int i = 0; i < nt; ++i) {
    cf v = slots[((size_t)clip * T + tchunk + i) * kFrameStride + p];
    if (cj) v.im = -v.im;
    out[((size_t)clip * kBins + bin) * T + tchunk + i] = v;
  }
}

// float slots -> (B, n_stft, T), reading each bin from its primary slot
__global__ void __launch_bounds__(256) unpack_mag_kernel(const float* __restrict__ slots, float* __restrict__ out, int T) {
  const int bin = blockIdx.x * blockDim.x + threadIdx.x;
  if (bin >= kBins) return;
  const int tchunk = blockIdx.y * 16;
  const int clip = blockIdx.z;
  int k = bin;
  if (k % 40 > 20) k = kNfft - k;
  const int k1 = k % 40, kp = k / 40;
  const int p = slot_pos_f(k1 * 21 + kp % 21, kp / 21);
  const int nt = min(16, T - tchunk);
  for (int i = 0; i < nt; ++i)
    out[((size_t)clip * kBins + bin) * T + tchunk + i] = slots[((size_t)clip * T + tchunk + i) * kFrameStride + p];
}
hipError_t launch_unpack_mag(const float* slots, float* out_bft, int B, int T, hipStream_t stream) {
  dim3 grid((kBins + 255) / 256, (T + 15) / 16, B);
  hipLaunchKernelGGL(unpack_mag_kernel, grid, dim3(256), 0, stream, slots, out_bft, T);
  return hipGetLastError();
}

hipError_t launch_pack_mag(const float* lin_bft, float* S_slots, int B, int T, hipStream_t stream) {
  dim3 grid((kFrameStride + 255) / 256, (T + 15) / 16, B);
  hipLaunchKernelGGL(pack_kernel<false>, grid, dim3(256), 0, stream, (const void*)lin_bft, (void*)S_slots, T);
  return hipGetLastError();
}
hipError_t launch_pack_angles(const cf* ang_bft, cf* slots, int B, int T, hipStream_t stream) {
  dim3 grid((kFrameStride + 255) / 256, (T + 15) / 16, B);
  hipLaunchKernelGGL(pack_kernel<true>, grid, dim3(256), 0, stream, (const void*)ang_bft, (void*)slots, T);
  return hipGetLastError();
}
hipError_t launch_unpack_complex(const cf* slots, cf* out_bft, int B, int T, hipStream_t stream) {
  dim3 grid((kBins + 255) / 256, (T + 15) / 16, B);
  hipLaunchKernelGGL(unpack_complex_kernel, grid, dim3(256), 0, stream, slots, out_bft, T);
  return hipGetLastError();
}

#ifndef RFX_FWD_ABL
#define RFX_FWD_ABL 0  // timing ablations of -DRFX_ABLATION builds (wrong results): 2 no product scatter, 3 no segment sums, 4 transform +
#endif                 // table fetches only, 5 no mel tables either, 7 no slot weights, 8 no twiddle fetches (profiles/r05_forward_ablation.txt)
#ifndef RFX_FWD_OPT
#define RFX_FWD_OPT 15  // what each bit buys is in profiles/r05_forward_ablation.txt; bit 4 (0.503 -> 0.500 ms) is off: it costs the nine
#endif                  // registers the running maximum of rfx_image_from_waveform needs
constexpr bool kFwdTwShort = (RFX_FWD_OPT & 2) != 0;   // eleven twiddles fetched, nine derived (bit 0: the packed tables, see launch_stft_mel)
constexpr bool kFwdWinRegs = (RFX_FWD_OPT & 4) != 0;   // ten-slot forms: the ten Hann samples stay in registers over the run
constexpr bool kFwdSlide = (RFX_FWD_OPT & 8) != 0;     // ten-slot forms: sliding input window, one new sample per frame
constexpr bool kFwdIdxRegs = (RFX_FWD_OPT & 16) != 0;  // PK: the packed positions / padding / segments stay in registers over the run

// ---- the forward frame kernels (rfx_stft_kernels.hip.h), and their twins of a loop forward call: the row read modulo its length
#define RFX_FWDK_LOOP 0
#include "rfx_stft_kernels.hip.h"
#undef RFX_FWDK_LOOP
#define RFX_FWDK_LOOP 1
#include "rfx_stft_kernels.hip.h"
#undef RFX_FWDK_LOOP
#define RFX_FWDK_LOOP 2  // stft_zero_kernel: the zero-extended analysis of rfx_istft_backward
#include "rfx_stft_kernels.hip.h"
#undef RFX_FWDK_LOOP

// (B, T, Mpad) frame-major mel amplitudes -> the reference's (B, M, T): 64 x 64 tiles through LDS, both sides coalesced
__global__ void __launch_bounds__(256) mel_transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int T, int M, int Mpad) {
  __shared__ float tile[64][65];
  const int t0 = blockIdx.x * 64, m0 = blockIdx.y * 64, b = blockIdx.z;
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  for (int r = ly; r < 64; r += 4) {
    const int tt = t0 + r;
    tile[r][lx] = tt < T ? in[((size_t)b * T + tt) * Mpad + m0 + lx] : 0.f;  // m0 + lx < Mpad always (Mpad % 64 == 0)
  }
  __syncthreads();
  for (int r = ly; r < 64; r += 4) {
    const int m = m0 + r, tt = t0 + lx;
    if (m < M && tt < T) out[((size_t)b * M + m) * T + tt] = tile[lx][r];
  }
}

hipError_t launch_mel_transpose(const float* mel_tm, float* mel, int B, int T, int M, int Mpad, hipStream_t stream) {
  hipLaunchKernelGGL(mel_transpose_kernel, dim3((T + 63) / 64, Mpad / 64, B), dim3(256), 0, stream, mel_tm, mel, T, M, Mpad);
  return hipGetLastError();
}

hipError_t launch_stft_mel(const StftMelArgs& a, hipStream_t stream) {
  const int chunks = (a.T + a.frames_per_block - 1) / a.frames_per_block;
  const dim3 grid(a.B * chunks), block(kThreads);
  if (a.slot_tab && (a.kb_mask & ~kKbMaskLow) == 0 && a.pk_at && (RFX_FWD_OPT & 1))
    hipLaunchKernelGGL((stft_mel2_kernel<kKbMaskLow, true>), grid, block, kFrameDynLdsBytes, stream, a);
  else if (a.slot_tab && (a.kb_mask & ~kKbMaskLow) == 0)
    hipLaunchKernelGGL((stft_mel2_kernel<kKbMaskLow, false>), grid, block, kFrameDynLdsBytes, stream, a);
  else if (a.slot_tab)
    hipLaunchKernelGGL((stft_mel2_kernel<kKbMaskAll, false>), grid, block, kFrameDynLdsBytes, stream, a);
  else hipLaunchKernelGGL(stft_mel_kernel, grid, block, kFrameDynLdsBytes, stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || !a.mel) return e;  // (no (B, M, T) copy wanted: rfx_image_from_waveform encodes from the frame-major scratch)
  return launch_mel_transpose(a.mel_tm, a.mel, a.B, a.T, a.M, a.Mpad, stream);
}

// the same choice among the loop twins
hipError_t launch_stft_mel_loop(const StftMelArgs& a, hipStream_t stream) {
  const int chunks = (a.T + a.frames_per_block - 1) / a.frames_per_block;
  const dim3 grid(a.B * chunks), block(kThreads);
  if (a.slot_tab && (a.kb_mask & ~kKbMaskLow) == 0 && a.pk_at && (RFX_FWD_OPT & 1))
    hipLaunchKernelGGL((stft_mel2_loop_kernel<kKbMaskLow, true>), grid, block, kFrameDynLdsBytes, stream, a);
  else if (a.slot_tab && (a.kb_mask & ~kKbMaskLow) == 0)
    hipLaunchKernelGGL((stft_mel2_loop_kernel<kKbMaskLow, false>), grid, block, kFrameDynLdsBytes, stream, a);
  else if (a.slot_tab)
    hipLaunchKernelGGL((stft_mel2_loop_kernel<kKbMaskAll, false>), grid, block, kFrameDynLdsBytes, stream, a);
  else hipLaunchKernelGGL(stft_mel_loop_kernel, grid, block, kFrameDynLdsBytes, stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || !a.mel) return e;
  return launch_mel_transpose(a.mel_tm, a.mel, a.B, a.T, a.M, a.Mpad, stream);
}

hipError_t prepare_frame_kernels() {
  for (const void* fn : {(const void*)stft_kernel, (const void*)stft_mel_kernel, (const void*)stft_mel2_kernel<kKbMaskLow, true>,
                         (const void*)stft_mel2_kernel<kKbMaskLow, false>, (const void*)stft_mel2_kernel<kKbMaskAll, false>,
                         (const void*)stft_loop_kernel, (const void*)stft_mel_loop_kernel, (const void*)stft_mel2_loop_kernel<kKbMaskLow, true>,
                         (const void*)stft_mel2_loop_kernel<kKbMaskLow, false>, (const void*)stft_mel2_loop_kernel<kKbMaskAll, false>,
                         (const void*)stft_zero_kernel}) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kFrameDynLdsBytes);
    if (e != hipSuccess) return e;
  }
  return prepare_gl_kernels();
}

hipError_t launch_stft(const StftArgs& a, hipStream_t stream) {
  const size_t lds = kFrameDynLdsBytes;
  const int chunks = (a.T + a.frames_per_block - 1) / a.frames_per_block;
  hipLaunchKernelGGL(stft_kernel, dim3(a.B * chunks), dim3(kThreads), lds, stream, a);
  return hipGetLastError();
}

hipError_t launch_stft_loop(const StftArgs& a, hipStream_t stream) {
  const int chunks = (a.T + a.frames_per_block - 1) / a.frames_per_block;
  hipLaunchKernelGGL(stft_loop_kernel, dim3(a.B * chunks), dim3(kThreads), kFrameDynLdsBytes, stream, a);
  return hipGetLastError();
}

hipError_t launch_stft_zero(const StftArgs& a, hipStream_t stream) {
  const int chunks = (a.T + a.frames_per_block - 1) / a.frames_per_block;
  hipLaunchKernelGGL(stft_zero_kernel, dim3(a.B * chunks), dim3(kThreads), kFrameDynLdsBytes, stream, a);
  return hipGetLastError();
}

}  // namespace rfx
