// rfx_fam.hip - Griffin-Lim (torchaudio.transforms.GriffinLim as constructed at riffusion/spectrogram_converter.py:62-73,
// called at :204) and the forward STFT (Spectrogram(power=None), :47-59, :179; fam_fwd_kernel and its loop twin, rfx_fam_fwd_kernel.hip.h) for the ROW FAMILY of STFT geometries: n_fft = 40 h, win_length = 10 h, any hop - the reference's default
// 400 / 100 / 10 ms (spectrogram_params.py:24-27, :62-81) at 48, 32, 24, 16 and 8 kHz (cli.py:43 takes the sample rate from
// the input file).  Round 2 / 3 ran these on the generic engine (rfx_generic.hip: a complex FFT of n_fft / 2 points over a
// runtime digit list, eleven barrier-separated phases per frame, 587 tiles/s at 48 kHz against 1960 at 44.1 kHz); here they
// get the specialised engine's factorisation (rfx_core.h) with h in place of 441:
//     P1   thread n' < h          pruned 40-point transform of the ten windowed samples h j + n' (only the window's quarter of
//                                 the frame is ever touched), twiddle g(n')^k1 -> 21 rows x h in LDS
//     A    thread (row, i < RB)   radix-RA butterfly down the row, twiddle W_h^{i p}
//     B    thread (row, p < RA)   radix-RB butterfly -> RB slots in registers: Z = S a / (|a| + 1e-16), inverse butterfly
//     A'   inverse of A           P1'  pruned inverse -> ten windowed synthesis samples -> HBM
// Four barriers per frame.  `a` is the spectrum of x_k - m x_{k-1}: the momentum term of the reference's
// `rebuilt - m tprev` is applied in the time domain (the STFT is linear, rfx_gl.hip), so no spectrum ever reaches HBM.
// One frame per workgroup trip (grid-stride), gen_fold_kernel (rfx_generic.hip) overlap-adds the frames: two launches per
// iteration, same buffers and same random stream as the generic engine, which remains the fallback for every other geometry.
// |S| arrives in the plan's plain bin-ordered layout and is re-ordered ONCE per call into slot order (thread t's slot s at
// s * nthr + t: every wave-wide load is whole lines); duplicate slots get the same magnitude.
// This file is compiled TWICE (round 4).  Translation unit 0 (rfx_fam.hip itself, plain fp32 butterflies): the forward kernels,
// the 48 kHz Griffin-Lim kernel, the launchers.  Translation unit 1 (rfx_fam_pk.hip: `#define RFX_PK 1`, `#define RFX_FAM_TU 1`,
// then this file): the Griffin-Lim kernels of every other geometry with PACKED butterflies (rfx_core.h).  Measured, Griffin-Lim 32
// of 64 tiles, packed against plain: 32 kHz 30.3 / 33.0 ms, 24 kHz 22.4 / 22.9, 22.05 kHz 20.7 / 22.2, 16 kHz 16.4 / 17.2,
// 8 kHz 8.2 / 9.1 - no scratch left in those kernels - but 48 kHz 57.8 / 48.9 (the radix-24 pass spills 100 B with the packed
// complex product's aligned pairs) and the forward kernels spill more everywhere.  The kernel templates carry the unit's number so
// that the two instantiations of one geometry are different symbols.  (-DRFX_FAM_PK: packed in unit 0 as well, A/B runs.)
#ifndef RFX_FAM_TU
#define RFX_FAM_TU 0
#endif
#if defined(RFX_FAM_PK) && !defined(RFX_PK)
#define RFX_PK 1
#endif
#include <hip/hip_runtime.h>

#include "rfx_fam_core.h"
#include "rfx_frame.hip.h"  // buffer-descriptor loads / stores (SRD in SGPRs + one 32-bit lane offset: no 64-bit per-lane addresses)
#include "rfx_kernels.h"
#include "rfx_loop_core.h"
#include "rfx_istft_core.h"

namespace rfx {

constexpr int fam_threads(int ra, int rb, int nr = 40) {
  int n = ra * rb;
  if ((nr / 2 + 1) * rb > n) n = (nr / 2 + 1) * rb;
  if ((nr / 2 + 1) * ra > n) n = (nr / 2 + 1) * ra;
  return (n + 63) / 64 * 64;
}

// Measured at 48 kHz / 16 kHz, 64 tiles x 32 iterations (tools/probe_fam.py): 16-byte LDS accesses in pass B together with a
// raised issue priority for the B phase 52.6 -> 50.4 ms / 19.2 -> 18.2 ms (each alone: 51.0 / 52.6 ms); both halves of the
// forward pass-A twiddles requested before the butterfly: 57.6 ms (registers) - off.
#ifndef RFX_FAM_VEC
#define RFX_FAM_VEC 1
#endif
#ifndef RFX_FAM_PRIO
#define RFX_FAM_PRIO 1
#endif
#ifndef RFX_FAM_TW_EARLY
#define RFX_FAM_TW_EARLY 0
#endif
#ifndef RFX_FAM_GL_STREAM_FWD
#define RFX_FAM_GL_STREAM_FWD true  // 48 kHz Griffin-Lim kernel: streamed radix-24 pass A (rfx_fam_core.h) - forward 38.3 -> 37.7 ms per 64 tiles x 32 iterations, inverse 39.8: off
#endif
#ifndef RFX_FAM_GL_STREAM_INV
#define RFX_FAM_GL_STREAM_INV false
#endif
#ifndef RFX_FAM_STORE_AUX
#define RFX_FAM_STORE_AUX 0  // cache policy of the synthesis-frame stores (the fold reads them back once)
#endif
#ifndef RFX_FAM_STREAM_AUX
#define RFX_FAM_STREAM_AUX kAuxNT  // |S| is read once per iteration: streamed past L2
#endif

#if RFX_FAM_TU == 0
bool fam_row_stride_even(const FamGeom& g) { return RFX_FAM_VEC && g.rb % 2 == 0; }
size_t fam_lds_bytes(const FamGeom& g) { return sizeof(cf) * (size_t)g.rows * g.rs; }
#endif

// Where the pass-A twiddles W_h^{i p} live: in LDS (a static array next to the cube: the compiler then knows that cube stores
// never alias twiddle reads) wherever two workgroups still share a CU with it - every geometry but 48 kHz, whose cube leaves
// 1.2 KB - and in the L1-resident global table otherwise.
constexpr bool fam_twiddles_in_lds(int ra, int rb) { return ra * rb != 480; }
#if RFX_FAM_TU == 0
size_t fam_static_lds_bytes(const FamGeom& g) { return fam_twiddles_in_lds(g.ra, g.rb) ? sizeof(cf) * (size_t)g.rb * (g.ra - 1) : 0; }
#endif

// the thread's RA - 1 pass-A twiddles, fetched in two batches
template <int RA, int RB, bool LDS>
struct FamTwA {
  cf w[RA];
  rsrc_t src;
  unsigned voff;
  const cf* tab;  // LDS column of this thread (entry p - 1 at (p - 1) RB)
  template <bool INV, int BATCH, bool STREAM = false>  // the twiddles of batch BATCH of the forward / inverse pass (rfx_fam_core.h::fam_tw_in_batch)
  __device__ __forceinline__ void load() {
#pragma unroll
    for (int p = 1; p < RA; ++p) {
      if (!fam_tw_in_batch(RA, INV, STREAM, BATCH, p)) continue;
#if defined(RFX_FAM_ABL) && RFX_FAM_ABL >= 1  // timing ablation (wrong results): no pass-A twiddle fetches
      w[p] = cf{1.f, (float)p};
      continue;
#endif
      if (LDS) {
        w[p] = tab[(p - 1) * RB];
      } else {
        const v2f t = ld2(src, voff, (unsigned)(p - 1) * (RB * 8u));
        w[p] = cf{t.x, t.y};
      }
    }
  }
  template <bool INV, bool STREAM = false>
  __device__ __forceinline__ void load_batch(int b) {  // b >= 1 is a compile-time constant wherever this is called (unrolled stages)
    if (b == 1) load<INV, 1, STREAM>();
    if (fam_tw_batches(RA, INV, STREAM) > 2 && b == 2) load<INV, 2, STREAM>();
    if (fam_tw_batches(RA, INV, STREAM) > 3 && b == 3) load<INV, 3, STREAM>();
  }
};

// MODE 0: Z = S * angles0 (injected or drawn) -> synthesis; MODE 1 / 2: analysis of d = x_k - m x_{k-1} (x_0 in the first iteration;
// the two modes are the same code since the fold forms d)
// 128 VGPRs: two 512-thread workgroups per CU at 48 kHz.  Every table / HBM value is requested one barrier before its use:
//   before P1 | A : first half of the pass-A twiddles            before A | B : the frame's |S|
//   before B' | A': first half of the conjugate twiddles          before A'| P1': g(n')^k1 and the Hann samples (P1' and the NEXT
//   frame's P1 use the same values), and the next frame's ten input samples
// Phases are fenced for the compiler's scheduler (left alone it hoists the next phase's loads over the current butterfly and
// spills 70 registers).
#define RFX_GLK_LIST 0
#include "rfx_fam_gl_kernel.hip.h"
#undef RFX_GLK_LIST
#define RFX_GLK_LIST 1
#include "rfx_fam_gl_kernel.hip.h"
#undef RFX_GLK_LIST
#define RFX_GLK_LIST 0
#define RFX_GLK_LOOP 1
#include "rfx_fam_gl_kernel.hip.h"
#undef RFX_GLK_LOOP
#undef RFX_GLK_LIST

#if RFX_FAM_TU == 0
#define RFX_FWDK_LOOP 0
#include "rfx_fam_fwd_kernel.hip.h"
#undef RFX_FWDK_LOOP
#define RFX_FWDK_LOOP 1
#include "rfx_fam_fwd_kernel.hip.h"
#undef RFX_FWDK_LOOP
#define RFX_FWDK_LOOP 2  // fam_fwd_zero_kernel: the zero-extended analysis of rfx_istft_backward
#include "rfx_fam_fwd_kernel.hip.h"
#undef RFX_FWDK_LOOP

// |S| (or any per-bin float array) from plain bin order [nframes][fs_plain] to slot order [nframes][fsf]: one workgroup per
// frame, the row staged in LDS (whole-line loads; the first version gathered 4-byte values 160 bytes apart straight from
// global memory: 1.39 ms per 64 x 512 frames at 48 kHz), whole-line stores
__global__ void __launch_bounds__(512) fam_repack_kernel(const float* __restrict__ plain, float* __restrict__ slots,
                                                         const int* __restrict__ bin_of, int fs_plain, int fsf, int n_stft) {
  extern __shared__ float row_s[];  // [n_stft]
  const size_t fr = blockIdx.x;
  const float* __restrict__ row = plain + fr * fs_plain;
  for (int i = threadIdx.x; i < n_stft; i += blockDim.x) row_s[i] = row[i];
  __syncthreads();
  float* __restrict__ out = slots + fr * fsf;
  for (int i = threadIdx.x; i < fsf; i += blockDim.x) {
    const int b = bin_of[i];
    out[i] = b >= 0 ? row_s[b] : 0.f;
  }
}

#endif  // RFX_FAM_TU == 0

using FamGlFn = void (*)(FamGlArgs);
template <int RA, int RB, int NR = 40>
static FamGlFn fam_fn(int mode) {
  return mode == 0 ? fam_gl_kernel<0, RA, RB, NR> : fam_gl_kernel<1, RA, RB, NR>;  // (modes 1 and 2 are one kernel since the fold forms d)
}
using FamGlListFn = void (*)(FamGlArgs, const int*);
#if RFX_FAM_TU == 1
// ... and their twins over a held call's free-frame list
FamGlListFn fam_gl_list_fn_packed(const FamGeom& g) {
  if (g.nrad == 20) return g.h == 441 ? fam_gl_list_kernel<1, 21, 21, 20> : nullptr;  // 22.05 kHz
  switch (g.h) {
    case 80: return fam_gl_list_kernel<1, 10, 8>;
    case 160: return fam_gl_list_kernel<1, 16, 10>;
    case 240: return fam_gl_list_kernel<1, 16, 15>;
    case 320: return fam_gl_list_kernel<1, 20, 16>;
    case 441: return fam_gl_list_kernel<1, 21, 21>;
    default: return nullptr;
  }
}
// ... and over a loop call's period (launches 1 .. n_iter)
FamGlFn fam_gl_loop_fn_packed(const FamGeom& g) {
  if (g.nrad == 20) return g.h == 441 ? fam_gl_loop_kernel<1, 21, 21, 20> : nullptr;  // 22.05 kHz
  switch (g.h) {
    case 80: return fam_gl_loop_kernel<1, 10, 8>;
    case 160: return fam_gl_loop_kernel<1, 16, 10>;
    case 240: return fam_gl_loop_kernel<1, 16, 15>;
    case 320: return fam_gl_loop_kernel<1, 20, 16>;
    case 441: return fam_gl_loop_kernel<1, 21, 21>;
    default: return nullptr;
  }
}
// unit 1: the packed Griffin-Lim kernels (every geometry but 48 kHz)
FamGlFn fam_gl_fn_packed(const FamGeom& g, int mode) {
  if (g.nrad == 20) return g.h == 441 ? fam_fn<21, 21, 20>(mode) : nullptr;  // 22.05 kHz
  switch (g.h) {
    case 80: return fam_fn<10, 8>(mode);
    case 160: return fam_fn<16, 10>(mode);
    case 240: return fam_fn<16, 15>(mode);
    case 320: return fam_fn<20, 16>(mode);
    case 441: return fam_fn<21, 21>(mode);
    default: return nullptr;
  }
}
#else
FamGlFn fam_gl_fn_packed(const FamGeom& g, int mode);  // rfx_fam_pk.hip
static FamGlFn fam_fn(const FamGeom& g, int mode) {
#if !defined(RFX_NO_PK) && !defined(RFX_FAM_PK)
  if (g.h != 480) return fam_gl_fn_packed(g, mode);
#else
  if (g.nrad == 20) return g.h == 441 ? fam_fn<21, 21, 20>(mode) : nullptr;  // 22.05 kHz
#endif
  switch (g.h) {
#if defined(RFX_NO_PK) || defined(RFX_FAM_PK)
    case 80: return fam_fn<10, 8>(mode);
    case 160: return fam_fn<16, 10>(mode);
    case 240: return fam_fn<16, 15>(mode);
    case 320: return fam_fn<20, 16>(mode);
    case 441: return fam_fn<21, 21>(mode);
#endif
    case 480: return fam_fn<24, 20>(mode);
    default: return nullptr;
  }
}
FamGlListFn fam_gl_list_fn_packed(const FamGeom& g);  // rfx_fam_pk.hip
static FamGlListFn fam_list_fn(const FamGeom& g) {
#if !defined(RFX_NO_PK) && !defined(RFX_FAM_PK)
  if (g.h != 480) return fam_gl_list_fn_packed(g);
#else
  if (g.nrad == 20) return g.h == 441 ? fam_gl_list_kernel<1, 21, 21, 20> : nullptr;  // 22.05 kHz
#endif
  switch (g.h) {
#if defined(RFX_NO_PK) || defined(RFX_FAM_PK)
    case 80: return fam_gl_list_kernel<1, 10, 8>;
    case 160: return fam_gl_list_kernel<1, 16, 10>;
    case 240: return fam_gl_list_kernel<1, 16, 15>;
    case 320: return fam_gl_list_kernel<1, 20, 16>;
    case 441: return fam_gl_list_kernel<1, 21, 21>;
#endif
    case 480: return fam_gl_list_kernel<1, 24, 20>;
    default: return nullptr;
  }
}
FamGlFn fam_gl_loop_fn_packed(const FamGeom& g);  // rfx_fam_pk.hip
static FamGlFn fam_loop_fn(const FamGeom& g) {
#if !defined(RFX_NO_PK) && !defined(RFX_FAM_PK)
  if (g.h != 480) return fam_gl_loop_fn_packed(g);
#else
  if (g.nrad == 20) return g.h == 441 ? fam_gl_loop_kernel<1, 21, 21, 20> : nullptr;  // 22.05 kHz
#endif
  switch (g.h) {
#if defined(RFX_NO_PK) || defined(RFX_FAM_PK)
    case 80: return fam_gl_loop_kernel<1, 10, 8>;
    case 160: return fam_gl_loop_kernel<1, 16, 10>;
    case 240: return fam_gl_loop_kernel<1, 16, 15>;
    case 320: return fam_gl_loop_kernel<1, 20, 16>;
    case 441: return fam_gl_loop_kernel<1, 21, 21>;
#endif
    case 480: return fam_gl_loop_kernel<1, 24, 20>;
    default: return nullptr;
  }
}

using FamFwdFn = void (*)(FamFwdArgs);
template <int RA, int RB, int NR = 40>
static FamFwdFn fam_fwd_fn(int mode) {
  return mode == 0 ? fam_fwd_kernel<0, RA, RB, NR> : mode == 1 ? fam_fwd_kernel<1, RA, RB, NR> : fam_fwd_kernel<2, RA, RB, NR>;
}
static FamFwdFn fam_fwd_fn(const FamGeom& g, int mode) {
  if (g.nrad == 20) return g.h == 441 ? fam_fwd_fn<21, 21, 20>(mode) : nullptr;  // 22.05 kHz
  switch (g.h) {
    case 80: return fam_fwd_fn<10, 8>(mode);
    case 160: return fam_fwd_fn<16, 10>(mode);
    case 240: return fam_fwd_fn<16, 15>(mode);
    case 320: return fam_fwd_fn<20, 16>(mode);
    case 441: return fam_fwd_fn<21, 21>(mode);
    case 480: return fam_fwd_fn<24, 20>(mode);
    default: return nullptr;
  }
}

// ... and their twins of a loop forward call
template <int RA, int RB, int NR = 40>
static FamFwdFn fam_fwd_loop_fn(int mode) {
  return mode == 0 ? fam_fwd_loop_kernel<0, RA, RB, NR> : mode == 1 ? fam_fwd_loop_kernel<1, RA, RB, NR> : fam_fwd_loop_kernel<2, RA, RB, NR>;
}
static FamFwdFn fam_fwd_loop_fn(const FamGeom& g, int mode) {
  if (g.nrad == 20) return g.h == 441 ? fam_fwd_loop_fn<21, 21, 20>(mode) : nullptr;  // 22.05 kHz
  switch (g.h) {
    case 80: return fam_fwd_loop_fn<10, 8>(mode);
    case 160: return fam_fwd_loop_fn<16, 10>(mode);
    case 240: return fam_fwd_loop_fn<16, 15>(mode);
    case 320: return fam_fwd_loop_fn<20, 16>(mode);
    case 441: return fam_fwd_loop_fn<21, 21>(mode);
    case 480: return fam_fwd_loop_fn<24, 20>(mode);
    default: return nullptr;
  }
}

// ... and the zero-extension twin (complex spectrum only)
static FamFwdFn fam_fwd_zero_fn(const FamGeom& g) {
  if (g.nrad == 20) return g.h == 441 ? fam_fwd_zero_kernel<1, 21, 21, 20> : nullptr;  // 22.05 kHz
  switch (g.h) {
    case 80: return fam_fwd_zero_kernel<1, 10, 8>;
    case 160: return fam_fwd_zero_kernel<1, 16, 10>;
    case 240: return fam_fwd_zero_kernel<1, 16, 15>;
    case 320: return fam_fwd_zero_kernel<1, 20, 16>;
    case 441: return fam_fwd_zero_kernel<1, 21, 21>;
    case 480: return fam_fwd_zero_kernel<1, 24, 20>;
    default: return nullptr;
  }
}

hipError_t launch_fam_fwd(int mode, const FamFwdArgs& a, int nblocks, hipStream_t stream) {
  hipLaunchKernelGGL(fam_fwd_fn(a.g, mode), dim3(nblocks), dim3(a.g.nthr), fam_lds_bytes(a.g), stream, a);
  return hipGetLastError();
}

hipError_t launch_fam_fwd_loop(int mode, const FamFwdArgs& a, int nblocks, hipStream_t stream) {
  hipLaunchKernelGGL(fam_fwd_loop_fn(a.g, mode), dim3(nblocks), dim3(a.g.nthr), fam_lds_bytes(a.g), stream, a);
  return hipGetLastError();
}

hipError_t launch_fam_fwd_zero(const FamFwdArgs& a, int nblocks, hipStream_t stream) {
  hipLaunchKernelGGL(fam_fwd_zero_fn(a.g), dim3(nblocks), dim3(a.g.nthr), fam_lds_bytes(a.g), stream, a);
  return hipGetLastError();
}

hipError_t prepare_fam_kernels(const FamGeom& g) {
  const FamFwdFn zf = fam_fwd_zero_fn(g);
  if (!zf) return hipErrorInvalidValue;
  if (const hipError_t ez = hipFuncSetAttribute((const void*)zf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fam_lds_bytes(g)); ez != hipSuccess) return ez;
  for (int mode = 0; mode < 3; ++mode) {
    const hipError_t e = hipFuncSetAttribute((const void*)fam_fwd_fn(g, mode), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fam_lds_bytes(g));
    if (e != hipSuccess) return e;
    const FamFwdFn lf = fam_fwd_loop_fn(g, mode);
    if (!lf) return hipErrorInvalidValue;
    if (const hipError_t el = hipFuncSetAttribute((const void*)lf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fam_lds_bytes(g)); el != hipSuccess) return el;
  }
  for (int mode = 0; mode < 2; ++mode) {
    const FamGlFn fn = fam_fn(g, mode);
    if (!fn) return hipErrorInvalidValue;
    const hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fam_lds_bytes(g));
    if (e != hipSuccess) return e;
  }
  const FamGlFn pfn = fam_loop_fn(g);
  if (!pfn) return hipErrorInvalidValue;
  if (const hipError_t e = hipFuncSetAttribute((const void*)pfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fam_lds_bytes(g)); e != hipSuccess) return e;
  const FamGlListFn lfn = fam_list_fn(g);
  if (!lfn) return hipErrorInvalidValue;
  return hipFuncSetAttribute((const void*)lfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fam_lds_bytes(g));
}

int fam_blocks_per_cu(const FamGeom& g) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)fam_fn(g, 1), g.nthr, fam_lds_bytes(g)) != hipSuccess || n < 1) n = 1;  // (counts the static LDS too)
  return n;
}

hipError_t launch_fam_gl(int mode, const FamGlArgs& a, int nblocks, hipStream_t stream) {
  hipLaunchKernelGGL(fam_fn(a.g, mode), dim3(nblocks), dim3(a.g.nthr), fam_lds_bytes(a.g), stream, a);
  return hipGetLastError();
}

hipError_t launch_fam_gl_list(const FamGlArgs& a, const int* list, int nblocks, hipStream_t stream) {
  hipLaunchKernelGGL(fam_list_fn(a.g), dim3(nblocks), dim3(a.g.nthr), fam_lds_bytes(a.g), stream, a, list);
  return hipGetLastError();
}

hipError_t launch_fam_gl_loop(const FamGlArgs& a, int nblocks, hipStream_t stream) {
  hipLaunchKernelGGL(fam_loop_fn(a.g), dim3(nblocks), dim3(a.g.nthr), fam_lds_bytes(a.g), stream, a);
  return hipGetLastError();
}

hipError_t launch_fam_repack(const float* plain, float* slots, const int* bin_of, long long nframes, int fs_plain, int fsf, int n_stft,
                             hipStream_t stream) {
  hipLaunchKernelGGL(fam_repack_kernel, dim3((unsigned)nframes), dim3(512), sizeof(float) * (size_t)n_stft, stream, plain, slots, bin_of, fs_plain, fsf, n_stft);
  return hipGetLastError();
}

#endif  // RFX_FAM_TU

}  // namespace rfx
