// rfx_mel_bwd.hip - the kernels of the forward path's backward (rfx_mel_bwd_core.h states the arithmetic; include/rfx.h:
// rfx_stft_backward, rfx_mel_scale_backward, rfx_mel_from_waveform_backward).  Between them run the engines' existing MODE 0
// per-frame launches, unchanged: launch_gl_frame, launch_fam_gl, launch_gen_gl, launch_czt_gl synthesise S * angles0.
//
//   mel_bwd_spec_kernel   builds what that launch reads.  FORM: MAGNITUDE SLOTS.  It writes S' = weight[k] gS[k] / |X[k]| (0 where
//                         |X| == 0) in the layout the engine's launch reads its magnitudes in, and the launch takes the spectrum X
//                         ITSELF - as the forward transform left it in the workspace - as its angles0: S' X is the weighted G of
//                         step 2, conjugate slots included (the slot holds conj X, the factor is real).  Every magnitude slot is
//                         made from the very complex value it will multiply (both slots of a doubled bin from their own).  X is
//                         read once here and once by the frame launch; no second complex array is written.  For rfx_stft_backward (no X, no g_mel)
//                         S' is the one-sided weights alone and the angles are the caller's gradient.
//   mel_bwd_bank_kernel   step 1 alone into the reference's (B, n_stft, T) layout (rfx_mel_scale_backward)
//   mel_bwd_fold_kernel   step 4: a gather per output sample, no envelope, no atomics; 4-wide where alignment allows
// and, for the fused spectral losses, spec_loss_slots_kernel and spec_loss_loop_fold_kernel below.  The two slot kernels share one
// launch helper, the two folds one launcher.
#include <hip/hip_runtime.h>

#include "rfx_kernels.h"
#include "rfx_mel_bwd_core.h"
#include "rfx_spec_loss_core.h"

namespace rfx {

constexpr int kMelBwdThreads = 512;

// One frame per trip.  Phase 1: the frame's column of g_mel into LDS.  Phase 2: the spectrum, 16 bytes (two complex values) per lane
// in the order it lies in memory; the value of position x - from its own complex value and the gradient of its bin, xpos_bin[x] -
// goes to u[x] in LDS (every position has one writer).  Phase 3: the magnitude slots, 16 bytes (four floats) per lane: slot p takes
// u[s2x[p]], the value made from the complex number the frame launch will multiply it by (padding: 0).
__global__ void __launch_bounds__(kMelBwdThreads) mel_bwd_spec_kernel(MelBwdSpecArgs a) {
  extern __shared__ __attribute__((aligned(16))) float mb_lds[];
  float* __restrict__ u = mb_lds;              // [xstride]
  float* __restrict__ gm = mb_lds + a.xstride;  // [M]
  const long long nframes = (long long)a.B * a.T;
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  for (long long fr = blockIdx.x; fr < nframes; fr += gridDim.x) {
    if (a.g_mel) {
      const long long b = fr / a.T;
      const int t = (int)(fr - b * a.T);
      const float* __restrict__ gcol = a.g_mel + (size_t)b * a.M * a.T + t;
      for (int m = tid; m < a.M; m += nthr) gm[m] = gcol[(size_t)m * a.T];
      __syncthreads();
      const float4* __restrict__ X4 = reinterpret_cast<const float4*>(a.X + (size_t)fr * a.xstride);
      const int2* __restrict__ xb2 = reinterpret_cast<const int2*>(a.xpos_bin);
      auto value = [&](int k, float re, float im) {
        const float gs = mel_adjoint_bin<float>(a.first[k], a.count[k], a.wt + (size_t)k * a.width, [&](int m) { return gm[m]; });
        return mel_bwd_bin_weight(k, a.n_fft, a.unit) * mel_bwd_unit_scale(gs, re, im);
      };
      float2* __restrict__ u2 = reinterpret_cast<float2*>(u);
      for (int i = tid; i < a.xstride / 2; i += nthr) {
        const float4 v = X4[i];
        const int2 k = xb2[i];
        u2[i] = float2{k.x >= 0 ? value(k.x, v.x, v.y) : 0.f, k.y >= 0 ? value(k.y, v.z, v.w) : 0.f};
      }
      __syncthreads();
    }
    float4* __restrict__ S4 = reinterpret_cast<float4*>(a.S + (size_t)fr * a.sstride);
    const int4* __restrict__ pb4 = reinterpret_cast<const int4*>(a.g_mel ? a.s2x : a.pos_bin);
    // (with a gradient: the position of the spectrum the slot goes with; without: the slot's bin)
    auto slot = [&](int k) { return k < 0 ? 0.f : a.g_mel ? u[k] : mel_bwd_bin_weight(k, a.n_fft, a.unit); };
    for (int i = tid; i < a.sstride / 4; i += nthr) {
      const int4 k = pb4[i];
      S4[i] = float4{slot(k.x), slot(k.y), slot(k.z), slot(k.w)};
    }
    __syncthreads();  // the next trip rewrites gm and u
  }
}

// out[b][k][t] = sum_i wt[k][i] g[b][first[k] + i][t]: consecutive lanes take consecutive t of one bin
__global__ void __launch_bounds__(256) mel_bwd_bank_kernel(const float* __restrict__ g_mel, float* __restrict__ out, const int* __restrict__ first,
                                                           const int* __restrict__ count, const float* __restrict__ wt, int width, int M, int T,
                                                           int n_stft) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
  const size_t b = blockIdx.z;
  if (t >= T) return;
  const float* __restrict__ g = g_mel + b * M * (size_t)T + t;
  out[(b * n_stft + k) * (size_t)T + t] =
      mel_adjoint_bin<float>(first[k], count[k], wt + (size_t)k * width, [&](int m) { return g[(size_t)m * T]; });
}

// Step 4.  A thread folds the samples j0 .. j0 + 3 of row b.  gp(q): the chain of padded position q over the frames whose window
// covers it, oldest first - an fma chain y w + acc where the frames come un-windowed (specialised engine), a sum where the frame
// launch has applied the window.  VEC (the host has checked fpitch, hop and h - left + fshift to be multiples of four and the frames
// 16-byte aligned): a group none of whose samples has a reflect partner reads every covering frame 16 bytes at a time - a sample of
// the group that lies outside a frame's window reads the zero padding of the frame's row (x + 0 = x: the scalar sums, term for term).
template <bool VEC>
__global__ void __launch_bounds__(256) mel_bwd_fold_kernel(MelBwdFoldArgs a) {
  using v4 = float __attribute__((ext_vector_type(4)));
  const int j0 = 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const size_t b = blockIdx.y;
  if (j0 >= a.Lw) return;
  const float* __restrict__ rows = a.frames + b * a.T * (size_t)a.fpitch + a.fshift;
  float* __restrict__ out = a.out + b * (size_t)a.Lw;
  auto gp = [&](int q) {
    int tlo, thi;
    mel_bwd_frame_range(q, a.left, a.win_len, a.hop, a.T, tlo, thi);
    float acc = 0.f;
    for (int t = tlo; t <= thi; ++t) {
      const int i = q - a.left - a.hop * t;
      const float y = rows[(size_t)t * a.fpitch + i];
      acc = a.win ? __fmaf_rn(y, a.win[i], acc) : acc + y;
    }
    return acc;
  };
  if (VEC && j0 + 3 < a.Lw && !mel_bwd_group_has_partner(j0, a.h, a.Lw)) {
    const int q = a.h + j0;
    int tlo, thi, tmp;
    mel_bwd_frame_range(q, a.left, a.win_len, a.hop, a.T, tlo, tmp);
    mel_bwd_frame_range(q + 3, a.left, a.win_len, a.hop, a.T, tmp, thi);
    v4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int t = tlo; t <= thi; ++t) acc += *reinterpret_cast<const v4*>(rows + (size_t)t * a.fpitch + (q - a.left - a.hop * t));
    if (a.Lw % 4 == 0) {
      *reinterpret_cast<v4*>(out + j0) = acc;
    } else {
      out[j0] = acc.x;
      out[j0 + 1] = acc.y;
      out[j0 + 2] = acc.z;
      out[j0 + 3] = acc.w;
    }
    return;
  }
  for (int j = j0; j < j0 + 4 && j < a.Lw; ++j) out[j] = mel_bwd_sample<float>(j, a.h, a.Lw, gp);
}

// ---- fused spectral losses (rfx_spec_loss_core.h; include/rfx.h: rfx_spectral_loss_backward) ------------------------------------------
// The second magnitude-slot kernel: mel_bwd_spec_kernel's structure with a per-bin loss in the place of the bank adjoint.  One frame per
// trip.  Phase 1 has nothing to stage (no incoming-gradient column).  Phase 2: the spectrum, 16 bytes (two complex values) per lane in
// the order it lies in memory; a[x] = |X[x]| of position x goes to LDS (every position has one writer).  Phase 3: the magnitude slots,
// 16 bytes per lane: slot p takes a[s2x[p]] - the magnitude of the very complex value the frame launch will multiply it by - the
// target's slot and the row's two coefficients, and writes weight[k] (dL/da) / a (padding: 0).  BY_BIN: the target lies bin-ordered
// (plain layouts) and is read at the slot's bin; else it lies in the slots' own order and is read 16 bytes at a time.
template <bool BY_BIN>
__global__ void __launch_bounds__(kMelBwdThreads) spec_loss_slots_kernel(SpecLossSlotArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sl_lds[];
  float* __restrict__ u = sl_lds;  // [xstride]
  const long long nframes = (long long)a.B * a.T;
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  for (long long fr = blockIdx.x; fr < nframes; fr += gridDim.x) {
    const long long b = fr / a.T;
    const float c_sc = a.coef[2 * b], c_lg = a.coef[2 * b + 1];
    const float4* __restrict__ X4 = reinterpret_cast<const float4*>(a.X + (size_t)fr * a.xstride);
    float2* __restrict__ u2 = reinterpret_cast<float2*>(u);
    for (int i = tid; i < a.xstride / 2; i += nthr) {
      const float4 v = X4[i];
      u2[i] = float2{spec_loss_abs(v.x, v.y), spec_loss_abs(v.z, v.w)};
    }
    __syncthreads();
    const float* __restrict__ M = a.target + (size_t)fr * a.xstride;
    float4* __restrict__ S4 = reinterpret_cast<float4*>(a.S + (size_t)fr * a.sstride);
    const int4* __restrict__ pb4 = reinterpret_cast<const int4*>(a.pos_bin);
    const int4* __restrict__ sx4 = reinterpret_cast<const int4*>(a.s2x);
    auto slot = [&](int k, int x, float m) {
      return k < 0 || x < 0 ? 0.f : mel_bwd_bin_weight(k, a.n_fft, a.unit) * spec_loss_unit_scale(u[x], m, c_sc, c_lg, a.floor);
    };
    for (int i = tid; i < a.sstride / 4; i += nthr) {
      const int4 k = pb4[i], x = sx4[i];
      float4 m;
      if (BY_BIN) m = float4{k.x < 0 ? 0.f : M[k.x], k.y < 0 ? 0.f : M[k.y], k.z < 0 ? 0.f : M[k.z], k.w < 0 ? 0.f : M[k.w]};
      else m = reinterpret_cast<const float4*>(M)[i];
      S4[i] = float4{slot(k.x, x.x, m.x), slot(k.y, x.y, m.y), slot(k.z, x.z, m.z), slot(k.w, x.w, m.w)};
    }
    __syncthreads();  // the next trip rewrites u
  }
}

// The circular adjoint fold.  A thread folds the samples m0 .. m0 + 3 of row b, one chain each (spec_loss_loop_sample): an fma chain
// y w + acc over un-windowed frames (a.win: specialised engine), a chain of sums over frames the launch has windowed.  VEC (windowed
// frames; the host has checked the plain fold's conditions - fpitch, hop and h - left + fshift multiples of four, frames and out
// 16-byte aligned; Lw = hop T is then a multiple of four too): the four samples share the frames from the oldest of the first to the
// newest of the last and read each 16 bytes at a time - a sample outside a frame's window reads the zero padding of the frame's row
// (x + 0 = x: the scalar sums, term for term).
template <bool VEC>
__global__ void __launch_bounds__(256) spec_loss_loop_fold_kernel(MelBwdFoldArgs a) {
  using v4 = float __attribute__((ext_vector_type(4)));
  const int m0 = 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const size_t b = blockIdx.y;
  if (m0 >= a.Lw) return;
  const float* __restrict__ rows = a.frames + b * a.T * (size_t)a.fpitch;
  float* __restrict__ out = a.out + b * (size_t)a.Lw;
  if (VEC) {
    const int q = m0 + a.h - a.left;
    int tlo, thi, tmp;
    loop_fold_range(q, a.win_len, a.hop, tlo, tmp);
    loop_fold_range(q + 3, a.win_len, a.hop, tmp, thi);
    v4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int t = tlo; t <= thi; ++t)
      acc += *reinterpret_cast<const v4*>(rows + (size_t)loop_frame(t, a.T) * a.fpitch + a.fshift + (q - a.hop * t));
    *reinterpret_cast<v4*>(out + m0) = acc;
    return;
  }
  for (int m = m0; m < m0 + 4 && m < a.Lw; ++m)
    out[m] = spec_loss_loop_sample(rows, (size_t)a.fpitch, a.fshift, a.win, m, a.h, a.left, a.win_len, a.hop, a.T);
}

// a slot kernel's launch: one frame per trip, at most 2^16 workgroups, `lds` bytes of dynamic LDS (the attribute where it is over 48 KiB)
template <class Args>
static hipError_t launch_slots(void (*kernel)(Args), const Args& a, size_t lds, hipStream_t stream) {
  const long long nframes = (long long)a.B * a.T;
  if (nframes <= 0) return hipSuccess;
  if (lds > 48u * 1024u) {
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const long long cap = 1 << 16;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(nframes < cap ? nframes : cap)), dim3(kMelBwdThreads), lds, stream, a);
  return hipGetLastError();
}
hipError_t launch_mel_bwd_spec(const MelBwdSpecArgs& a, hipStream_t stream) {
  return launch_slots(mel_bwd_spec_kernel, a, sizeof(float) * ((size_t)a.xstride + (size_t)(a.M > 0 ? a.M : 0)), stream);
}
hipError_t launch_spec_loss_slots(const SpecLossSlotArgs& a, hipStream_t stream) {
  return launch_slots(a.target_by_bin ? spec_loss_slots_kernel<true> : spec_loss_slots_kernel<false>, a, sizeof(float) * (size_t)a.xstride, stream);
}

hipError_t launch_mel_bwd_bank(const float* g_mel, float* out_bft, const int* first, const int* count, const float* wt, int width, int B, int M,
                               int T, int n_stft, hipStream_t stream) {
  // blockIdx.z carries the row: at most 65535 rows per launch
  for (int b0 = 0; b0 < B; b0 += 65535) {
    const int rows = B - b0 < 65535 ? B - b0 : 65535;
    hipLaunchKernelGGL(mel_bwd_bank_kernel, dim3((T + 255) / 256, n_stft, rows), dim3(256), 0, stream, g_mel + (size_t)b0 * M * T,
                       out_bft + (size_t)b0 * n_stft * T, first, count, wt, width, M, T, n_stft);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_mel_bwd_fold(const MelBwdFoldArgs& a, bool circular, hipStream_t stream) {
  if (a.B <= 0 || a.Lw <= 0) return hipSuccess;
  // (the plain fold stores a group 16 bytes at once only where Lw is a multiple of four; the circular one's Lw = hop T always is)
  const uintptr_t out = reinterpret_cast<uintptr_t>(a.out);
  const bool out_ok = circular ? (out & 15) == 0 : (out & 3) == 0 && (a.Lw % 4 != 0 || (out & 15) == 0);
  const bool vec = !a.win && a.fpitch % 4 == 0 && a.hop % 4 == 0 && (a.h - a.left + a.fshift) % 4 == 0 &&
                   (reinterpret_cast<uintptr_t>(a.frames) & 15) == 0 && out_ok;
  const auto kernel = circular ? (vec ? spec_loss_loop_fold_kernel<true> : spec_loss_loop_fold_kernel<false>)
                               : (vec ? mel_bwd_fold_kernel<true> : mel_bwd_fold_kernel<false>);
  const unsigned gx = (unsigned)(((a.Lw + 3) / 4 + 255) / 256);
  for (int b0 = 0; b0 < a.B; b0 += 65535) {  // blockIdx.y carries the row
    MelBwdFoldArgs c = a;
    c.B = a.B - b0 < 65535 ? a.B - b0 : 65535;
    c.frames = a.frames + (size_t)b0 * a.T * a.fpitch;
    c.out = a.out + (size_t)b0 * a.Lw;
    hipLaunchKernelGGL(kernel, dim3(gx, c.B), dim3(256), 0, stream, c);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace rfx
